"""examples/viewer_frame.cpp runs on the GPU box: the scene of examples/shaded_hits.cpp — a textured quad with masked squares in front of an untextured
pyramid under a TLAS — rendered by tbvh_viewer_render from the camera to the 0x00BBGGRR pixels on the device, C ABI only; the program itself checks what
it sees and writes a PPM."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_viewer_frame_example(tmp_path):
    exe = os.path.join(ROOT, "examples", "_build", "viewer_frame")
    assert os.path.exists(exe), "examples/_build/viewer_frame not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "viewer frame ok" in out.stdout and "round 0: 65536 rays traced" in out.stdout and "round 1:" in out.stdout and "round 2:" not in out.stdout
    ppm = (tmp_path / "viewer_frame.ppm").read_bytes()
    assert ppm.startswith(b"P6\n256 256\n255\n") and len(ppm) == 15 + 256 * 256 * 3
