"""Regenerate tests/golden/shade/*.npz from the REAL reference's GetShadingData (tests/shade_ref_shim.cpp; needs the reference checkout, TBVH_REFERENCE).
The inputs are tests/shade_fixtures.py's deterministic scene and record sets; each file holds the records, the instance records as the host TLAS build
left them, and the expected 48-byte records: words 0..10 from the real reference for every record it can be asked about (an in-range hit whose texel reads
lie inside the textures), everything else — the texel word, misses, the records whose reference read is outside its texture — from the restatement
(tests/oracle_shade.c), with `from_reference` saying which is which.  pose_skin.npz / pose_morph.npz: the words of slot 0's
FatTri records that the real Mesh::SetPose writes.  tests/test_shade_host.py holds the files to the generators and to all three."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import shade_fixtures as F  # noqa: E402
import shade_lib as L  # noqa: E402
from oracle_lib import Oracle  # noqa: E402


def make(ref, orc, out_dir=L.GOLDEN):
    os.makedirs(out_dir, exist_ok=True)
    sc = F.scene()
    traced, inst = F.traced_on_the_cpu(Oracle(tie_rule=1))
    for name, r in (("traced", traced), ("synthetic", sc.synthetic_records())):
        out, flags = orc.shade(sc.materials, sc.textures, sc.fat, r, inst)
        ask = (flags & (L.NO_SURFACE | L.REF_OUT_OF_BOUNDS)) == 0
        real = ref.shade(sc.materials, sc.textures, sc.fat, r[ask], inst)
        want = out.copy()
        want[ask, :11] = real[:, :11]
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), records=r, instances=inst, want=want.view(np.uint32), from_reference=ask)
        print(name + ".npz", os.path.getsize(os.path.join(out_dir, name + ".npz")), "bytes;", int(ask.sum()), "of", r.shape[0], "records from the real reference")


def make_pose(ref, out_dir=L.GOLDEN):
    """the real Mesh::SetPose's FatTri arrays over slot 0's records: the words it can write (quarters 2 .. 7 of each record), frame 0 for the whole mesh,
    frame 1 for the first POSE_SMALL triangles"""
    sc, cases = F.scene(), F.pose_cases()
    k = L.POSE_SMALL
    s, m = cases["skin"], cases["morph"]
    a = ref.setpose_skin(sc.fat[0], s["rest"], s["joints"], s["weights"], s["normals"], s["mats"][0])
    b = ref.setpose_skin(sc.fat[0][:k], s["rest"][:3 * k], s["joints"][:3 * k], s["weights"][:3 * k], s["normals"][:3 * k], s["mats"][1])
    assert L.only_these_changed(sc.fat[0], a, L.skin_fields())
    np.savez_compressed(os.path.join(out_dir, "pose_skin.npz"), written=L.words(a)[:, L.WRITTEN_WORDS], written_b=L.words(b)[:, L.WRITTEN_WORDS])
    a = ref.setpose_morph(sc.fat[0], m["positions"], m["normals"], m["weights"][0])
    b = ref.setpose_morph(sc.fat[0][:k], m["positions"][:, :3 * k], m["normals"][:, :3 * k], m["weights"][1])
    assert L.only_these_changed(sc.fat[0], a, L.morph_fields())
    np.savez_compressed(os.path.join(out_dir, "pose_morph.npz"), written=L.words(a)[:, L.WRITTEN_WORDS], written_b=L.words(b)[:, L.WRITTEN_WORDS])
    for n in ("pose_skin", "pose_morph"):
        print(n + ".npz", os.path.getsize(os.path.join(out_dir, n + ".npz")), "bytes")


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        ref = L.compile_ref_shim(d)
        if ref is None:
            sys.exit("the reference checkout (TBVH_REFERENCE) is absent")
        make(ref, L.compile_oracle(d))
        make_pose(ref)
