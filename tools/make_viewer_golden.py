"""Writes tests/golden/viewer/*.npz from the REAL reference (needs the checkout, TBVH_REFERENCE): tests/viewer_ref_shim.cpp compiled over tiny_bvh_gltf.cpp and
tiny_bvh_foliage.cpp, the fixture scene of tests/viewer_fixtures.py as a TLAS and its third BLAS alone (under one identity instance: the viewers always trace
a TLAS), the fixture camera at the files' 800 x 600.
  frame_<mode>_<kind>.npz   buf: WorkerThread's 800 x 600 words; pix: every 131st pixel; rays, occ: those pixels' final records and shadow flags of the CPU
                            frame (host twins over the reference's own traversal); rgb: the file's Trace on those pixels' camera rays
  sky.npz                   the file's SampleSky on the well-defined directions of the sky fixture (no NaN, |D.y| <= 1), per sky size
Before anything is written the tool asserts what tests/test_viewer_host.py asserts with the checkout present: Trace == the restatement on EVERY ray, buf ==
its pack on every pixel.
usage: python tools/make_viewer_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tinybvh_amd as tb  # noqa: E402
import shade_fixtures as SF  # noqa: E402
import viewer_fixtures as F  # noqa: E402
import viewer_lib as L  # noqa: E402
from native_build import have_reference  # noqa: E402


def main():
    if not have_reference(*L.REF_FILES):
        sys.exit("tools/make_viewer_golden.py needs the reference checkout (TBVH_REFERENCE)")
    os.makedirs(L.GOLDEN, exist_ok=True)
    sc = F.scene()
    sky = F.sky(F.FRAME_SKY)
    cam = sc.camera(800, 600)
    n = 800 * 600
    pix = np.arange(0, n, L.GOLDEN_STEP)
    with tempfile.TemporaryDirectory() as d:
        oracle = L.compile_oracle(d)
        light = F.default_light()
        for mode_name in ("gltf", "foliage"):
            mode = tb.VIEWER_GLTF if mode_name == "gltf" else tb.VIEWER_FOLIAGE
            sub = os.path.join(d, mode_name); os.makedirs(sub)
            ref = L.compile_ref_shim(sub, foliage=mode_name == "foliage")
            for kind in ("tlas", "blas"):
                verts, fat, inst, lib_inst = F.scene_kind(sc, kind)
                ref.scene(inst, verts, fat, sc.materials, sc.textures, sky)
                fr = L.cpu_frame(ref.intersect, ref.occluded, sc, fat, lib_inst, cam, mode, sky)
                want_rgb, _ = oracle.light(mode, sky, fr["rays"], fr["out"], fr["occ"], light, L.margins())
                ref_rgb, _ = ref.trace(tb.host_viewer_generate(cam))
                buf = ref.frame(cam)
                assert np.array_equal(want_rgb[:, :3].view(np.uint32), ref_rgb.view(np.uint32)), "the restatement differs from the file's Trace"
                assert np.array_equal(oracle.pack(want_rgb), buf.reshape(-1)), "the restatement differs from WorkerThread's buf"
                occ = np.zeros(n, np.uint8) if fr["occ"] is None else fr["occ"]
                path = os.path.join(L.GOLDEN, f"frame_{mode_name}_{kind}.npz")
                np.savez_compressed(path, buf=buf, pix=pix, rays=fr["rays"][pix], occ=occ[pix], rgb=ref_rgb[pix], per_round=np.array(fr["per_round"]))
                print(f"{path}: {os.path.getsize(path)} bytes, rays per round {fr['per_round']}")
                ref.release()
            if mode_name == "gltf":
                dirs, classes = F.sky_directions()
                ok = F.defined_directions(dirs)
                out = {"defined": ok}
                for h, w in F.SKY_SHAPES:
                    out[f"sky_{h}x{w}"] = ref.sky(F.sky((h, w)), dirs[ok])
                path = os.path.join(L.GOLDEN, "sky.npz")
                np.savez_compressed(path, **out)
                print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
