"""BVH_Double scenes that move, the parts that need no GPU: the bindings of the new entry points against the header, the tiny_hip.h methods
against the real tiny_bvh.h when it is present, the entry points' refusals that come before any device work, and the numpy restatement
of the device TLAS builder (double_anim_lib.karras_tlas), which test_double_anim_gpu.py holds the device-built trees against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
from double_lib import odbl  # noqa: F401 (fixture)
from double_anim_lib import TREE_SHAPE_CAP, bounds_of, check_tlas_tree, karras_tlas, morton63, refit_boxes, tlas_rays, tlas_scene
from native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tbvh_rebuild_tlas_double_device", "tbvh_update_tlas_double", "tbvh_tlas_double_download", "tbvh_double_download", "tbvh_refit_double")


def header_arg_counts():
    src = open(os.path.join(ROOT, "include", "tinybvh_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tbvh_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_capi_declares_the_new_symbols_as_the_header_does():
    counts = header_arg_counts()
    raw = C.CDLL(_capi.LIB_PATH)
    for s in NEW:
        assert s in counts, f"{s} is not declared in include/tinybvh_amd.h"
        assert s in _capi.SYMBOLS, f"{s} is not bound in _capi.py"
        assert hasattr(raw, s), f"{s} is not exported"
        restype, argtypes = _capi.SYMBOLS[s]
        assert restype is C.c_int and len(argtypes) == counts[s], (s, len(argtypes), counts[s])
    assert _capi.lib.tbvh_abi_version() == 5   # additions only


def test_null_handles_are_refused_by_name():
    lib = _capi.lib
    buf = np.zeros(64, np.uint8)
    n = C.c_uint64(0)
    calls = {
        "tbvh_rebuild_tlas_double_device": lambda: lib.tbvh_rebuild_tlas_double_device(None, None, 0),
        "tbvh_update_tlas_double": lambda: lib.tbvh_update_tlas_double(None, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data, 1),
        "tbvh_tlas_double_download": lambda: lib.tbvh_tlas_double_download(None, None, 0, None, 0, None, 0, C.byref(n)),
        "tbvh_double_download": lambda: lib.tbvh_double_download(None, None, 0, C.byref(n)),
        "tbvh_refit_double": lambda: lib.tbvh_refit_double(None, buf.ctypes.data, 1, 0),
    }
    assert sorted(calls) == sorted(NEW)
    for name, call in calls.items():
        assert call() == -1 and name.encode() in lib.tbvh_last_error(), (name, lib.tbvh_last_error())


def test_tiny_hip_double_anim_binding_compiles(tmp_path):
    syntax_check(tmp_path, '#include "tiny_bvh.h"\n#include "tiny_hip.h"\n'
                 "void f(tinybvh::BVH_Double& b, tinybvh::BVH_Double& tlas, const double* xf, tinybvh::bvhdbl3* verts) {\n"
                 "    tinyhip::Scene s(b); std::vector<tinyhip::Scene*> v{&s}; tinyhip::Scene t(tlas, v);\n"
                 "    t.RebuildOnDevice(); t.RebuildOnDevice(xf); t.RebuildOnDevice(xf, true); t.Update(tlas);\n"
                 "    s.Refit(verts, b.triCount); s.Refit(verts, b.triCount, true);\n"
                 "    std::vector<tinybvh::BVH_Double::BVHNode> n = s.Download();\n"
                 "    std::vector<uint64_t> idx(tlas.idxCount); std::vector<tinybvh::BLASInstanceEx> inst(tlas.triCount); n.resize(2 * tlas.triCount);\n"
                 "    uint64_t used = t.Download(n.data(), n.size(), idx.data(), idx.size(), inst.data(), inst.size()); (void)used;\n}\n")


def test_morton_keys_resolve_a_cluster_far_from_the_rest():
    """Two instances 10 units apart, a third 1e7 units away: 21 bits per axis (cells of 4.8 units) tell the two apart, the 10 bits per axis
    of a 30-bit key (cells of 9766 units) would not."""
    lo = np.array([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0], [1e7, 1e7, 1e7]])
    k = morton63(lo, lo + 0.5)
    assert k[0] != k[1] and k[1] < k[2] and int(k.max()) < 1 << 63
    ext = 1e7
    assert (np.floor(lo[:2] / ext * 1023.0) == 0).all()   # what 10 bits per axis make of the pair


@pytest.mark.parametrize("n", [1, 2, 3, 27, 64, 65, 500])
def test_numpy_karras_tree_is_valid(n):
    from double_lib import instance_scene
    blas_verts, inst = instance_scene(n)
    if n == 27:
        inst[1::2] = inst[0:26:2]   # equal boxes, equal keys: told apart by position
    tb.host_build_tlas_double(inst, bounds_of(blas_verts))
    nodes, idx = karras_tlas(inst)
    check_tlas_tree(nodes, idx, inst)


def test_tree_shape_does_not_change_the_records(odbl):
    """The oracle walks the host-built (binned SAH) tree and a Karras tree over the same instance records: the records must agree on all
    but TREE_SHAPE_CAP of the 32768 rays test_double_anim_gpu.py traces (this is where its scene and ray seeds are checked)."""
    blas_verts, inst = tlas_scene()
    host = tb.host_build_tlas_double(inst, bounds_of(blas_verts))
    bl = []
    for v in blas_verts:
        h = tb.host_build_double(v)
        bl.append((h.nodes(), h.prim_idx(), v))
    rays = tlas_rays()
    want = odbl.intersect_tlas(host.nodes(), host.prim_idx(), inst, bl, rays, rule=1)
    kn, ki = karras_tlas(inst)
    check_tlas_tree(kn, ki, inst)
    got = odbl.intersect_tlas(kn, ki, inst, bl, rays, rule=1)
    a = got.view(np.uint8).reshape(-1, 128); b = want.view(np.uint8).reshape(-1, 128)
    differ = int((a != b).any(1).sum())
    hit = want["t"] < 1e299
    assert hit.sum() > 1000 and np.unique(want["inst"][hit]).size > 100
    assert differ <= TREE_SHAPE_CAP, f"{differ} of {rays.shape[0]} records differ between the two trees"


def test_refit_boxes_reproduces_the_host_builder():
    from double_lib import rotated_soup
    v = rotated_soup(300) + 1e7
    h = tb.host_build_double(v)
    nodes = h.nodes().copy()
    blank = nodes.copy(); blank["aabbMin"] = 0; blank["aabbMax"] = 0
    assert refit_boxes(blank, h.prim_idx(), v).tobytes() == nodes.tobytes()
