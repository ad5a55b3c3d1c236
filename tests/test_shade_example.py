"""examples/shaded_hits.cpp runs on the GPU box: a textured quad with transparent squares in front of an untextured pyramid under a TLAS, traced, shaded
(tbvh_shade_hits_device) and stepped through the transparent texels (tbvh_shade_continue_device) on the device, C ABI only; the program itself checks
what it sees and writes a PPM."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_shaded_hits_example(tmp_path):
    exe = os.path.join(ROOT, "examples", "_build", "shaded_hits")
    assert os.path.exists(exe), "examples/_build/shaded_hits not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shaded hits ok" in out.stdout and "round 0:" in out.stdout and " 0 rays stepped" in out.stdout
    ppm = (tmp_path / "shaded_hits.ppm").read_bytes()
    assert ppm.startswith(b"P6\n256 256\n255\n") and len(ppm) == 15 + 256 * 256 * 3
