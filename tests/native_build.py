"""Every native compile the tests and tools/ do apart from the product's own build: the plain-C restatements (tests/oracle_*.c), the shims over the real
reference (tests/*_ref_shim.cpp), the "this binding compiles" checks, and the session fixtures over them.  The flag sets are stated here once.  They
are part of what the bit-for-bit tests compare against (-O2 -ffp-contract=off rounds a restatement once per operation as written; -O3 -mavx2 -mfma,
oracle/Makefile's flags, is the build of the reference whose contractions the product restates), so no caller spells them out again.

This module is the only reader of TBVH_REFERENCE.  oracle_lib.have_reference() answers another question: was oracle/_ref built."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NO_REFERENCE = "the reference checkout (TBVH_REFERENCE) is absent"
REF_ISA = ("-mavx2", "-mfma")   # every build over the reference's headers, optimised or not

_vp, _u64, _u32, _i = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int


def _p(a):
    return C.c_void_p(a.ctypes.data)


def reference_dir():
    return os.environ.get("TBVH_REFERENCE", "/root/reference")


def have_reference(*files):
    """every one of the named files (default: tiny_bvh.h) is in the reference checkout"""
    return all(os.path.isfile(os.path.join(reference_dir(), f)) for f in files or ("tiny_bvh.h",))


def compile_c_oracle(d, stem, extra=("-std=c11",)):
    """d/lib<stem>.so from tests/<stem>.c (or from <stem>.c where stem is an absolute path).  extra holds what one file needs beyond the common flags;
    its default is the language level that every restatement but oracle_double.c is built with."""
    so = os.path.join(str(d), "lib" + os.path.basename(stem) + ".so")
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", *extra, os.path.join(HERE, stem + ".c"), "-o", so, "-lm"])
    return so


def patched_scene_header(d):
    """The reference's tiny_scene.h has a bare `#elif`, which g++ refuses.  Writes a copy with that directive turned into `#else`, and nothing else touched,
    into d; d then goes FIRST on the include path, so that the shim's `#include "tiny_scene.h"` finds the copy.  Nothing of it is kept."""
    with open(os.path.join(reference_dir(), "tiny_scene.h"), "rb") as f:
        lines = f.read().split(b"\n")
    for k, line in enumerate(lines):
        if line.strip() == b"#elif":
            lines[k] = line.replace(b"#elif", b"#else")
    with open(os.path.join(str(d), "tiny_scene.h"), "wb") as f:
        f.write(b"\n".join(lines))
    return str(d)


def compile_ref_shim(d, shim, out=None, defines=(), extra=(), scene_header=False, need=("tiny_bvh.h",)):
    """d/lib<out>.so (out defaults to the shim's name without `_shim.cpp`) from tests/<shim> (or from an absolute path) over the real reference, with
    oracle/Makefile's flags; None when the reference is absent, that is when one of `need` is.  A compiler error raises: a broken shim is no skip.
    scene_header: the shim includes tiny_scene.h, which takes the patched copy and the reference's external/ directory."""
    if not have_reference(*need):
        return None
    ref = reference_dir()
    inc = [patched_scene_header(d), ref, os.path.join(ref, "external")] if scene_header else [ref]
    so = os.path.join(str(d), "lib" + (out or os.path.basename(shim).replace("_shim.cpp", "")) + ".so")
    subprocess.check_call(["g++", "-std=c++20", "-O3", *REF_ISA, "-fPIC", "-shared", "-w", *("-D" + x for x in defines), *("-I" + x for x in inc), *extra,
                           os.path.join(HERE, shim), "-o", so, "-lpthread"])
    return so


def syntax_check(tmp_path, text, need=("tiny_bvh.h",)):
    """g++ -fsyntax-only over `text` with the reference and include/ on the include path: what a "this binding compiles" test asks.  Skips without the
    reference."""
    if not have_reference(*need):
        pytest.skip(NO_REFERENCE)
    src = os.path.join(str(tmp_path), "binding.cpp")
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(["g++", "-std=c++20", "-fsyntax-only", "-w", "-I" + reference_dir(), "-I" + os.path.join(ROOT, "include"), src])


def oracle_fixture(name, compile_oracle):
    """a session fixture: compile_oracle(d), a lib's two-line wrapper of compile_c_oracle, over a temp dir of that name"""
    @pytest.fixture(scope="session")
    def fixture(tmp_path_factory):
        return compile_oracle(tmp_path_factory.mktemp(name))
    return fixture


def ref_fixture(name, compile_shim):
    """a session fixture: compile_shim(d), a lib's two-line wrapper of compile_ref_shim, over a temp dir of that name; skips where that gives None"""
    @pytest.fixture(scope="session")
    def fixture(tmp_path_factory):
        r = compile_shim(tmp_path_factory.mktemp(name))
        if r is None:
            pytest.skip(NO_REFERENCE)
        return r
    return fixture
