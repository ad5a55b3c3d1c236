"""The plan a live TLAS has stored (tinybvh_amd/csrc/tlas_plan.h; capi_scene.hip: reclassifyTlas) is never stale, and a TLAS's device_bytes is what it holds.

Part one: row d of tlas_edges_lib.CONFIGS (two BVH_GPU BLASes, variant 0) through everything that changes a fact the plan reads: the upload, the first
Intersect, the first IsOccluded (8-wide copies, a class of its own for any-hit queries), an update of BLAS 0 (its copies go: copy_policy.h), the queries
that bring them back, a pin on BLAS 1 (the closest-hit class is formed again without 4-wide copies: BVH8_CWBVH and BVH_GPU mixed), a refit of BLAS 0, a
device rebuild of the TLAS.  After each step the facts tbvh_debug_tlas_state reports, fed to tbvh_debug_tlas_plan, must give exactly the stored plan, and
the records of a query must be the oracle's under the rules of tests/test_tlas_edges_gpu.py (its Scene does the comparing).

Part two: device_bytes of the TLAS of rows a, b and f right after the upload equals the number after TLAS.Update with the same arrays (the wide trees the
TLAS still holds are still counted) and the number the commit before this test gave at the upload, recorded here."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
import tlas_edges_lib as E
from test_tlas_edges_gpu import Scene

pytestmark = pytest.mark.gpu


def consistent(tlas):
    """the stored plan equals the plan of the facts as they are now; returns (facts, plan) as dicts"""
    facts, plan = tlas.debug_plan()
    fw, out = facts["words"], np.full(plan["words"].size, 0xDEAD, np.uint32)
    tb.check(_capi.lib.tbvh_debug_tlas_plan(C.c_void_p(fw.ctypes.data), fw.size, C.c_void_p(out.ctypes.data), out.size), "tbvh_debug_tlas_plan")
    assert np.array_equal(out, plan["words"]), (facts, plan, out)
    return facts, plan


def test_stored_plan_is_never_stale(ctx, oracle_ties):
    seen = []

    def records(s, occluded=True):
        s.compare(s.tlas.Intersect(s.rays.copy()), s.want, s.rays)
        if occluded:
            assert s.occluded_differs(s.tlas.IsOccluded(s.rays.copy()), s.want, s.rays) <= 2

    def copies(facts):
        return [(b["has8"], b["has4"]) for b in facts["blas"]]

    def before_first_query(s):
        facts, plan = consistent(s.tlas)                                          # 1. upload
        assert copies(facts) == [(False, True)] * 2 and not facts["any_hit_seen"] and plan["closest"]["family"] == "Tlas4" and not plan["any_own"]
        records(s, occluded=False)                                                # 2. first Intersect
        facts, plan = consistent(s.tlas)
        assert not facts["any_hit_seen"] and plan["any"]["family"] == "Tlas4"
        seen.append(plan["words"])

    s = Scene(ctx, oracle_ties, None, "d", on_upload=before_first_query)          # 3. first IsOccluded (in the fixture, with its assertions)
    try:
        assert len(seen) == 1
        tl, b0, b1 = s.tlas, s.blas[0], s.blas[1]
        facts, plan = consistent(tl)
        assert facts["any_hit_seen"] and copies(facts) == [(True, True)] * 2 and plan["any_own"] and plan["want8"] and plan["want4"]
        E.assert_kernel(plan["closest"], "tlas4"); E.assert_kernel(plan["any"], "tlas8copy")
        records(s)
        h = b0.host                                                               # 4. tbvh_update_bvh_gpu of BLAS 0 with its own blob: its copies go
        b0.Update(h.blob(0, np.uint32, 16), h.blob(1, np.uint32, 1), h.verts)
        facts, plan = consistent(tl)
        assert copies(facts) == [(False, False), (True, True)]
        assert plan["closest"]["views"] == ["own", "copy8"] and plan["closest"]["mix"] and plan["closest"]["family"] == "Tlas8" and not plan["any_own"]
        records(s)                                                                # (two of the queries counted below)
        small, more = s.rays[:64], 0
        while copies(consistent(tl)[0])[0] == (False, False):                     # 5. copy_policy.h: recopyAfter = 4 queries without another update
            assert more < 4
            tl.Intersect(small.copy()); more += 1
        assert more >= 1, "the copies came back before the fourth query"
        facts, plan = consistent(tl)
        assert copies(facts) == [(True, True)] * 2
        E.assert_kernel(plan["closest"], "tlas4"); E.assert_kernel(plan["any"], "tlas8copy")
        records(s)
        b1.set_variant(1)                                                         # 6. BLAS 1 pinned: {4-wide copy, BVH_GPU} is no class, so without 4-wide copies
        facts, plan = consistent(tl)
        assert facts["blas"][1]["pinned"] and plan["closest"]["views"] == ["copy8", "own"] and not plan["any_own"]
        assert plan["closest"]["family"] == "Tlas8" and plan["closest"]["mix"]
        records(s)
        b0.Refit(s.tri_meshes[0])                                                 # 7. a device refit of BLAS 0 (the same vertices): its copies follow in place
        facts, plan = consistent(tl)
        assert copies(facts)[0] == (True, True)
        records(s)
        tl.RebuildOnDevice()                                                      # 8. the TLAS's shape does not change a record
        consistent(tl)
        records(s)
    finally:
        s.close()


# device_bytes of the TLAS right after TLAS.Build on the commit before this test (MI355X; the same on every device: counts times record sizes)
BYTES_AT_UPLOAD = {"a": 10320, "b": 10320, "f": 11540}


@pytest.mark.parametrize("key", list(BYTES_AT_UPLOAD))
def test_bytes_count_the_wide_trees_after_an_update(ctx, key):
    row, vs = E.CONFIGS[key], E.meshes()
    blas = []
    try:
        for k, (lay, var) in enumerate(zip(row.layouts, row.variants)):
            blas.append(tb.LAYOUT_CLASSES[lay](ctx).Build(vs[k]))
            if var:
                blas[-1].set_variant(var)
        inst, _ = E.families(len(blas))
        tl = tb.TLAS(ctx).Build(inst, blas)
        try:
            at_upload = tl.device_bytes
            assert at_upload == BYTES_AT_UPLOAD[key]
            tl.Update(tl.host.blob(0, np.uint32, 16), tl.host.blob(1, np.uint32, 1), inst)
            assert tl.device_bytes == at_upload
        finally:
            tl.free()
    finally:
        for b in blas:
            b.free()
