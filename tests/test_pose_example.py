"""examples/skinned_mesh.cpp runs on the GPU box: a skinned tube posed and refitted on the device per frame (tbvh_pose_set_skin + tbvh_pose_refit, C ABI
only) under a TLAS that is uploaded once; the program itself checks that the tube is hit and that the hit count follows the animation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_skinned_mesh_example():
    exe = os.path.join(ROOT, "examples", "_build", "skinned_mesh")
    assert os.path.exists(exe), "examples/_build/skinned_mesh not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("camera rays hit the skinned tube") == 6 and "skinned mesh ok" in out.stdout
