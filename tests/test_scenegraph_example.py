"""examples/animated_scene.cpp: the animated frame with no host computation — tbvh_scenegraph_advance feeds tbvh_pose_set_skin and tbvh_rebuild_tlas_device from device
memory (C ABI only).  It compiles against the public header wherever the library is built; on the GPU box it runs, and checks itself that the tube is hit and
that the hit count follows the animation."""
import os
import subprocess

import pytest

import native_build as nb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_animated_scene_example_compiles(tmp_path):
    lib = os.path.join(ROOT, "tinybvh_amd")
    assert os.path.exists(os.path.join(lib, "libtinybvh_amd.so")), "the library is not built (run __graft_entry__.build())"
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "animated_scene.cpp"), "-L" + lib,
                           "-ltinybvh_amd", "-Wl,-rpath," + lib, "-lpthread", "-o", str(tmp_path / "animated_scene")])


@pytest.mark.gpu
def test_animated_scene_example():
    exe = os.path.join(ROOT, "examples", "_build", "animated_scene")
    assert os.path.exists(exe), "examples/_build/animated_scene not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("camera rays hit the animated tube") == 8 and "animated scene ok" in out.stdout


def test_tiny_hip_scenegraph_binding_compiles(tmp_path):
    """examples/scenegraph_binding.cpp instantiates every member of tinyhip::SceneGraph (tiny_hip.h needs tiny_bvh.h: skipped without the reference header).
    Compiled and linked against the library, which is more than native_build.syntax_check asks."""
    if not nb.have_reference():
        pytest.skip(nb.NO_REFERENCE)
    lib = os.path.join(ROOT, "tinybvh_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O2", *nb.REF_ISA, "-w", "-I" + nb.reference_dir(), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "scenegraph_binding.cpp"),
                           "-L" + lib, "-ltinybvh_amd", "-Wl,-rpath," + lib, "-lpthread", "-o", str(tmp_path / "scenegraph_binding")])


@pytest.mark.gpu
def test_tiny_hip_scenegraph_binding_runs():
    """the binding's verbs against the host twin, byte for byte (built by __graft_entry__.build() where the reference header is found)"""
    exe = os.path.join(ROOT, "examples", "_build", "scenegraph_binding")
    if not os.path.exists(exe):
        pytest.skip("examples/_build/scenegraph_binding not built (needs the reference header at build time)")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "scenegraph binding ok" in out.stdout, out.stdout + out.stderr
