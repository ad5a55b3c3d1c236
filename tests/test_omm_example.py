"""examples/alpha_foliage.cpp runs on the GPU box: a few hundred leaf quads whose opacity micromaps are baked on the device from a procedural leaf texture
(tbvh_bake_set_opacity_micromaps, C ABI only); the program itself checks that the maps let shadow rays through, that clearing them gives the plain count
back, and that the device bake equals the host bake."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_alpha_foliage_example():
    exe = os.path.join(ROOT, "examples", "_build", "alpha_foliage")
    assert os.path.exists(exe), "examples/_build/alpha_foliage not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shadow rays blocked by the leaf quads" in out.stdout and "alpha foliage ok" in out.stdout
