"""tests/native_build.py itself: the header patch, the answers without a reference checkout, a broken shim, and a restatement's round trip.  No GPU and no
reference: TBVH_REFERENCE points at temp dirs holding one-line stand-ins."""
import ctypes as C
import subprocess

import pytest

import native_build as nb


@pytest.fixture
def fake_reference(tmp_path, monkeypatch):
    ref = tmp_path / "reference"
    ref.mkdir()
    monkeypatch.setenv("TBVH_REFERENCE", str(ref))
    return ref


@pytest.fixture
def no_compiler(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError(f"a compiler was started: {a}")
    monkeypatch.setattr(subprocess, "check_call", refuse)


def test_patched_scene_header_changes_the_bare_elif_lines_only(fake_reference, tmp_path):
    keep = [b"#if defined(A)", b"int a;\r", b"#elif defined(X)", b"// caf\xe9 #elif", b"#endif", b""]
    lines = keep[:2] + [b"#elif"] + keep[2:4] + [b"  #elif  \r"] + keep[4:]
    (fake_reference / "tiny_scene.h").write_bytes(b"\n".join(lines))
    out = tmp_path / "out"
    out.mkdir()
    assert nb.patched_scene_header(out) == str(out)
    got = (out / "tiny_scene.h").read_bytes().split(b"\n")
    assert got == keep[:2] + [b"#else"] + keep[2:4] + [b"  #else  \r"] + keep[4:]


def test_without_the_reference_nothing_is_compiled(fake_reference, tmp_path, no_compiler):
    assert not nb.have_reference()
    assert nb.compile_ref_shim(tmp_path, "sphere_ref_shim.cpp") is None
    (fake_reference / "tiny_bvh.h").write_text("// stand-in\n")
    assert nb.have_reference() and nb.have_reference("tiny_bvh.h")
    assert not nb.have_reference("tiny_bvh.h", "tiny_scene.h")
    assert nb.compile_ref_shim(tmp_path, "pose_ref_shim.cpp", scene_header=True, need=("tiny_bvh.h", "tiny_scene.h")) is None


def test_a_broken_shim_raises(fake_reference, tmp_path):
    (fake_reference / "tiny_bvh.h").write_text("// stand-in\n")
    shim = tmp_path / "broken_ref_shim.cpp"
    shim.write_text('#include "tiny_bvh.h"\nint f( { return 0; }\n')
    with pytest.raises(subprocess.CalledProcessError):
        nb.compile_ref_shim(tmp_path, str(shim))


def test_a_c_oracle_compiles_and_answers(tmp_path):
    (tmp_path / "oracle_tiny.c").write_text("#include <math.h>\n"
                                            "double orc_tiny(double x) { return sqrt(x) + 1.0; }\n")
    so = nb.compile_c_oracle(tmp_path, str(tmp_path / "oracle_tiny"))
    assert so == str(tmp_path / "liboracle_tiny.so")
    f = C.CDLL(so).orc_tiny
    f.restype, f.argtypes = C.c_double, [C.c_double]
    assert f(9.0) == 4.0
