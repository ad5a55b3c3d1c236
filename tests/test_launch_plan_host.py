"""What a query launch of n rays on a scene of b bytes will do (tinybvh_amd/csrc/launch_plan.h; no GPU needed), driven through tbvh_debug_launch_plan,
which runs the two functions launchQuery runs.  The expected answers come from a model of the rule's sentences kept here:

The scene.  small: not a TLAS, no grid override, under 48 MB.  huge: not small and beyond 384 MB (exactly 384 MB is neither).
The grid.  One workgroup per raysPerBlock rays, at least 4 per CU, at most the persistent grid (24 per CU) — a third more on a small scene.
The probe.  probed: a single-level BVH8_CWBVH scene neither small nor huge, 2^21 rays and more, variant 0 or 88, debug flag 64 not set; such a batch that
fills the persistent grid gets a third more workgroups unless the grid is overridden.  probedSmall: such a scene that IS small or huge, variant 0, a
size the host knows, from 3 * 2^18 rays (small) or 6 * 2^20 (huge), no flag 64, no grid override — unless the schedule pinned for the context or settled
for the batch's size class is 1 or 2 (cancelled: the plan says so); 3 keeps it.
The size class.  3: a small scene and fewer than 3 * 2^19 rays; otherwise 0 below 6 * 2^20, 1 below 12 * 2^20, 2 from there.
The tuner may measure a probed or probedSmall launch while nothing is pinned and its class is undecided.
The kernels of a BVH8_CWBVH launch.  Variant 90 with both copies, 91, 92: the diagnostic kernels.  Two flavors: a probe, variant 0, not flag 4, and either
the hybrid node copy and the 64-byte triangle records without a padded node copy, or probedSmall (then the unprobed kernel runs behind).  Else one kernel.
The padded copy is walked (autoPad) at variant 0 where it exists.
A launch may ever go solo (soloCandidate): probed, variant 0, no padded copy, both other copies, no debug flag at all, nothing pinned, no grid override;
it asks for a verdict slot when the memory is on, the launch is timed and the host knows its size."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi

MB = 1 << 20
CWBVH, BVH_GPU, BVH4_GPU = tb.LAYOUT_CWBVH, tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU
FACTS = ("isTlas", "layout", "variant", "blobBytes", "n", "sizeKnown", "any", "gridOverride", "numCUs", "blocks", "raysPerBlock", "expFlags", "cohTunerMode",
         "decided0", "decided1", "decided2", "decided3", "hasPadded", "hasHybrid", "hasTrisPadded", "probeMemoryOn", "skipTiming")
PLAN = ("small", "huge", "probed", "probedSmall", "probedSmallCancelled", "sizeClass", "blocksBase", "blocks", "blocks7Tlas", "blocks7Cwbvh", "tunerMeasures",
        "soloCandidate", "wantsVerdictSlot", "shape", "autoPad")
ONE, TWO, BEHIND, V90, V91, V92 = range(6)


def facts(**kw):
    """a street-class BVH8_CWBVH scene with its copies on a 256-CU context as tbvh_init leaves it, 4 M rays"""
    f = dict(isTlas=0, layout=CWBVH, variant=0, blobBytes=196 * MB, n=1 << 22, sizeKnown=1, any=0, gridOverride=0, numCUs=256, blocks=256 * 24, raysPerBlock=128,
             expFlags=0, cohTunerMode=0, decided0=0, decided1=0, decided2=0, decided3=0, hasPadded=0, hasHybrid=1, hasTrisPadded=1, probeMemoryOn=1, skipTiming=0)
    assert set(kw) <= set(f), kw
    f.update(kw)
    return f


def plan(f):
    a = np.array([f[k] for k in FACTS], np.uint64)
    out = np.full(len(PLAN), 0xDEAD, np.uint32)
    tb.check(_capi.lib.tbvh_debug_launch_plan(C.c_void_p(a.ctypes.data), len(FACTS), C.c_void_p(out.ctypes.data), len(PLAN)), "tbvh_debug_launch_plan")
    return dict(zip(PLAN, (int(x) for x in out)))


def model(f):
    """the sentences of the docstring, one by one"""
    p = {}
    single_cwbvh = not f["isTlas"] and f["layout"] == CWBVH
    flag64 = bool(f["expFlags"] & 64)
    p["small"] = not f["isTlas"] and not f["gridOverride"] and f["blobBytes"] < 48 * MB
    p["huge"] = not p["small"] and f["blobBytes"] > 384 * MB
    ceiling = f["blocks"] + f["blocks"] // 3 if p["small"] else f["blocks"]
    p["blocksBase"] = min(max(-(-f["n"] // f["raysPerBlock"]), 4 * f["numCUs"]), ceiling)
    p["probed"] = single_cwbvh and not p["small"] and not p["huge"] and f["n"] >= 2 ** 21 and f["variant"] in (0, 88) and not flag64
    if p["small"] and f["n"] < 3 * 2 ** 19:
        p["sizeClass"] = 3
    else:
        p["sizeClass"] = 0 if f["n"] < 6 * 2 ** 20 else 1 if f["n"] < 12 * 2 ** 20 else 2
    schedule = f["cohTunerMode"] or f["decided%d" % p["sizeClass"]]
    by_size = (single_cwbvh and (p["small"] or p["huge"]) and f["variant"] == 0 and f["sizeKnown"] and not flag64 and not f["gridOverride"]
               and f["n"] >= (3 * 2 ** 18 if p["small"] else 6 * 2 ** 20))
    p["probedSmallCancelled"] = by_size and schedule in (1, 2)
    p["probedSmall"] = by_size and not p["probedSmallCancelled"]
    widen = p["probed"] and not f["gridOverride"] and p["blocksBase"] == f["blocks"]
    p["blocks"] = f["blocks"] + f["blocks"] // 3 if widen else p["blocksBase"]
    p["blocks7Tlas"] = 28 * f["numCUs"] if (not f["gridOverride"] and p["blocks"] == f["blocks"]) else p["blocks"]
    p["blocks7Cwbvh"] = 0xFFFFFFFF if f["gridOverride"] else 28 * f["numCUs"]
    p["tunerMeasures"] = (p["probed"] or p["probedSmall"]) and schedule == 0
    both = f["hasHybrid"] and f["hasTrisPadded"]
    p["autoPad"] = f["variant"] == 0 and f["hasPadded"]
    two = (p["probed"] or p["probedSmall"]) and f["variant"] == 0 and not f["expFlags"] & 4 and ((both and not p["autoPad"]) or p["probedSmall"])
    if f["variant"] == 90 and both:
        p["shape"] = V90
    elif f["variant"] in (91, 92):
        p["shape"] = V91 if f["variant"] == 91 else V92
    else:
        p["shape"] = ONE if not two else BEHIND if p["probedSmall"] else TWO
    p["soloCandidate"] = (p["probed"] and f["variant"] == 0 and not f["hasPadded"] and both and f["expFlags"] == 0 and f["cohTunerMode"] == 0
                          and not f["gridOverride"])
    p["wantsVerdictSlot"] = p["soloCandidate"] and f["probeMemoryOn"] and not f["skipTiming"] and f["sizeKnown"]
    return {k: int(v) for k, v in p.items()}


def check(**kw):
    f = facts(**kw)
    got, want = plan(f), model(f)
    assert got == want, (kw, {k: (got[k], want[k]) for k in PLAN if got[k] != want[k]})
    return got


def test_the_entry_refuses_other_word_counts_and_a_zero_divisor():
    a = np.array([facts()[k] for k in FACTS], np.uint64)
    out = np.zeros(len(PLAN), np.uint32)
    lib = _capi.lib
    assert lib.tbvh_debug_launch_plan(C.c_void_p(a.ctypes.data), len(FACTS) - 1, C.c_void_p(out.ctypes.data), len(PLAN)) == -1
    assert lib.tbvh_debug_launch_plan(C.c_void_p(a.ctypes.data), len(FACTS), C.c_void_p(out.ctypes.data), len(PLAN) + 1) == -1
    assert lib.tbvh_debug_launch_plan(None, len(FACTS), C.c_void_p(out.ctypes.data), len(PLAN)) == -1
    a[FACTS.index("raysPerBlock")] = 0
    assert lib.tbvh_debug_launch_plan(C.c_void_p(a.ctypes.data), len(FACTS), C.c_void_p(out.ctypes.data), len(PLAN)) == -1


def test_scene_classes_at_48_and_384_mb():
    p = check(blobBytes=48 * MB - 1)
    assert p["small"] and not p["huge"] and not p["probed"] and p["probedSmall"]
    p = check(blobBytes=48 * MB)
    assert not p["small"] and not p["huge"] and p["probed"] and not p["probedSmall"]
    p = check(blobBytes=384 * MB, n=6 << 20)
    assert not p["huge"] and p["probed"] and not p["probedSmall"]          # exactly 384 MB is still probed
    p = check(blobBytes=384 * MB + 1, n=6 << 20)
    assert p["huge"] and not p["probed"] and p["probedSmall"] and p["shape"] == BEHIND


def test_probed_from_2_pow_21_rays():
    assert not check(n=2 ** 21 - 1)["probed"]
    p = check(n=2 ** 21)
    assert p["probed"] and p["shape"] == TWO and p["soloCandidate"] and p["wantsVerdictSlot"] and p["tunerMeasures"]


def test_probed_small_thresholds():
    assert not check(blobBytes=10 * MB, n=3 * 2 ** 18 - 1)["probedSmall"]
    p = check(blobBytes=10 * MB, n=3 * 2 ** 18)
    assert p["probedSmall"] and p["shape"] == BEHIND and p["sizeClass"] == 3 and not p["soloCandidate"]
    assert not check(blobBytes=500 * MB, n=6 * 2 ** 20 - 1)["probedSmall"]
    p = check(blobBytes=500 * MB, n=6 * 2 ** 20)
    assert p["probedSmall"] and p["sizeClass"] == 1


def test_size_classes():
    for blob in (10 * MB, 196 * MB, 500 * MB):
        small = blob < 48 * MB
        assert check(blobBytes=blob, n=3 * 2 ** 19 - 1)["sizeClass"] == (3 if small else 0)
        assert check(blobBytes=blob, n=3 * 2 ** 19)["sizeClass"] == 0
        assert check(blobBytes=blob, n=6 * 2 ** 20 - 1)["sizeClass"] == 0
        assert check(blobBytes=blob, n=6 * 2 ** 20)["sizeClass"] == 1
        assert check(blobBytes=blob, n=12 * 2 ** 20 - 1)["sizeClass"] == 1
        assert check(blobBytes=blob, n=12 * 2 ** 20)["sizeClass"] == 2


@pytest.mark.parametrize("cus", [256, 304, 7])
def test_grid_floor_and_cap(cus):
    m = dict(numCUs=cus, blocks=24 * cus)
    floor_rays = 4 * cus * 128
    for blob in (10 * MB, 196 * MB):
        cap = 32 * cus if blob < 48 * MB else 24 * cus           # a third more on a small scene
        assert check(blobBytes=blob, n=1, **m)["blocksBase"] == 4 * cus
        assert check(blobBytes=blob, n=floor_rays, **m)["blocksBase"] == 4 * cus
        assert check(blobBytes=blob, n=floor_rays + 1, **m)["blocksBase"] == 4 * cus + 1
        assert check(blobBytes=blob, n=cap * 128 - 128, **m)["blocksBase"] == cap - 1
        assert check(blobBytes=blob, n=cap * 128, **m)["blocksBase"] == cap
        assert check(blobBytes=blob, n=cap * 128 + 1, **m)["blocksBase"] == cap
        assert check(blobBytes=blob, n=1 << 26, **m)["blocksBase"] == cap
    p = check(n=1 << 22, raysPerBlock=4096, gridOverride=1, **m)     # another divisor comes with the override
    assert p["blocksBase"] == {256: 1024, 304: 1216, 7: 168}[cus]    # 1024 wanted: as it is, raised to the floor, cut to the cap


def test_24_to_32_per_cu_only_for_a_probed_batch_that_fills_the_grid():
    p = check(n=2 ** 21)                                            # on 256 CUs every batch of 2^21 rays fills the 6144 workgroups (786432 rays do)
    assert p["probed"] and p["blocksBase"] == 6144 and p["blocks"] == 8192
    p = check(n=2 ** 21, gridOverride=1)
    assert p["probed"] and p["blocks"] == 6144 and p["blocks7Cwbvh"] == 0xFFFFFFFF and p["blocks7Tlas"] == 6144
    p = check(n=2 ** 21, expFlags=64)
    assert not p["probed"] and p["blocks"] == 6144
    p = check(n=2 ** 21, blobBytes=10 * MB)                         # a small scene has its 32 per CU from the cap, probed or not
    assert not p["probed"] and p["blocksBase"] == 8192 and p["blocks"] == 8192
    big = dict(numCUs=1024, blocks=1024 * 24)                       # a machine whose persistent grid a probed batch can fall short of
    full = 1024 * 24 * 128
    p = check(n=full, **big)
    assert p["probed"] and p["blocksBase"] == 24576 and p["blocks"] == 32768
    p = check(n=full - 128, **big)                                  # one workgroup short
    assert p["probed"] and p["blocksBase"] == 24575 and p["blocks"] == 24575
    p = check(n=full, isTlas=1, **big)
    assert p["blocks"] == 24576 and p["blocks7Tlas"] == 1024 * 28
    assert check(n=full - 128, isTlas=1, **big)["blocks7Tlas"] == 24575


def test_what_switches_the_probes_off():
    for blob, n in ((196 * MB, 1 << 22), (10 * MB, 1 << 22), (500 * MB, 1 << 23)):
        on = check(blobBytes=blob, n=n)
        assert on["probed"] != on["probedSmall"]
        for off in (dict(isTlas=1), dict(layout=BVH_GPU), dict(layout=BVH4_GPU), dict(expFlags=64), dict(expFlags=64 | 16), dict(variant=72), dict(variant=90),
                    dict(variant=91), dict(variant=92)):
            p = check(blobBytes=blob, n=n, **off)
            assert not p["probed"] and not p["probedSmall"] and not p["tunerMeasures"] and not p["soloCandidate"], (blob, off)
        p = check(blobBytes=blob, n=n, variant=88)                  # 88 keeps `probed` alone
        assert p["probed"] == on["probed"] and not p["probedSmall"] and p["shape"] == ONE and not p["soloCandidate"]
        p = check(blobBytes=blob, n=n, sizeKnown=0)                 # a device-side count: `probed` stays, probedSmall and the verdict slot go
        assert p["probed"] == on["probed"] and not p["probedSmall"] and not p["wantsVerdictSlot"]
        p = check(blobBytes=blob, n=n, gridOverride=1)              # (no scene is small under an override: the 10 MB scene is probed)
        assert not p["probedSmall"] and p["probed"] == (blob <= 384 * MB) and not p["soloCandidate"]


def test_a_per_lane_schedule_cancels_probed_small_and_packet_keeps_it():
    for blob, n, cls in ((10 * MB, 3 * 2 ** 18, 3), (10 * MB, 1 << 22, 0), (500 * MB, 1 << 23, 1), (500 * MB, 1 << 24, 2)):
        for m in (1, 2, 3):
            for how in (dict(cohTunerMode=m), {"decided%d" % cls: m}):
                p = check(blobBytes=blob, n=n, **how)
                assert p["sizeClass"] == cls and p["probedSmall"] == (m == 3) and p["probedSmallCancelled"] == (m != 3) and not p["tunerMeasures"]
                assert p["shape"] == (BEHIND if m == 3 else ONE)
            other = {"decided%d" % k: m for k in range(4) if k != cls}      # another class's decision says nothing about this one
            p = check(blobBytes=blob, n=n, **other)
            assert p["probedSmall"] and not p["probedSmallCancelled"] and p["tunerMeasures"]
    p = check(decided0=2)                                            # `probed` is never cancelled: the tuner's schedule is what its coherent flavor runs
    assert p["probed"] and not p["probedSmallCancelled"] and not p["tunerMeasures"] and p["soloCandidate"]


def test_two_flavor_shape_needs_both_copies_no_padded_copy_and_not_flag_4():
    assert check()["shape"] == TWO
    for off in (dict(hasHybrid=0), dict(hasTrisPadded=0), dict(hasPadded=1), dict(expFlags=4), dict(n=2 ** 21 - 1)):
        p = check(**off)
        assert p["shape"] == ONE and not p["soloCandidate"] and p["autoPad"] == off.get("hasPadded", 0), off
    for blob in (10 * MB, 500 * MB):                                 # probedSmall needs no copies, and walks the padded one behind where it exists
        for pad, hyb, tri in itertools.product((0, 1), repeat=3):
            p = check(blobBytes=blob, n=1 << 23, hasPadded=pad, hasHybrid=hyb, hasTrisPadded=tri)
            assert p["shape"] == BEHIND and p["autoPad"] == pad
        assert check(blobBytes=blob, n=1 << 23, expFlags=4)["shape"] == ONE
    for hyb, tri in itertools.product((0, 1), repeat=2):
        assert check(variant=90, hasHybrid=hyb, hasTrisPadded=tri)["shape"] == (V90 if hyb and tri else ONE)
    assert check(variant=91)["shape"] == V91 and check(variant=92, blobBytes=10 * MB)["shape"] == V92
    assert not check(variant=88, hasPadded=1)["autoPad"]


def test_each_condition_of_a_solo_candidate_and_of_its_verdict_slot():
    p = check()
    assert p["soloCandidate"] and p["wantsVerdictSlot"]
    for off in (dict(n=2 ** 21 - 1), dict(variant=88), dict(hasPadded=1), dict(hasHybrid=0), dict(hasTrisPadded=0), dict(expFlags=1), dict(expFlags=16),
                dict(expFlags=0x1C00), dict(cohTunerMode=1), dict(cohTunerMode=3), dict(gridOverride=1)):
        p = check(**off)
        assert not p["soloCandidate"] and not p["wantsVerdictSlot"], off
    for off in (dict(probeMemoryOn=0), dict(skipTiming=1), dict(sizeKnown=0)):
        p = check(**off)
        assert p["soloCandidate"] and not p["wantsVerdictSlot"], off
    assert check(any=1) == check(any=0)                              # the tuners' decisions are stated for the launch's kind of hit: `any` adds nothing


def test_a_sweep_agrees_with_the_model():
    rng = np.random.default_rng(5)
    blobs = (1, 48 * MB - 1, 48 * MB, 196 * MB, 384 * MB, 384 * MB + 1, 3000 * MB)
    ns = (1, 131072, 3 * 2 ** 18 - 64, 3 * 2 ** 18, 3 * 2 ** 19 - 1, 3 * 2 ** 19, 2 ** 21 - 1, 2 ** 21, 6 * 2 ** 20 - 1, 6 * 2 ** 20, 12 * 2 ** 20 - 1, 12 * 2 ** 20, 2 ** 24)
    for _ in range(4000):
        pick = lambda xs: xs[int(rng.integers(len(xs)))]
        bit = lambda p1: int(rng.random() < p1)
        check(isTlas=bit(0.1), layout=pick((CWBVH, CWBVH, CWBVH, BVH_GPU, BVH4_GPU)), variant=pick((0, 0, 0, 0, 88, 90, 91, 92, 72)), blobBytes=pick(blobs), n=pick(ns),
              sizeKnown=bit(0.8), any=bit(0.5), gridOverride=bit(0.15), numCUs=pick((256, 304)), blocks=pick((256 * 24, 304 * 24, 256 * 16)),
              raysPerBlock=pick((128, 128, 96)), expFlags=pick((0, 0, 0, 4, 16, 64, 0x1C00)), cohTunerMode=pick((0, 0, 0, 1, 2, 3)), decided0=pick((0, 0, 1, 2, 3)),
              decided1=pick((0, 1, 2, 3)), decided2=pick((0, 1, 2, 3)), decided3=pick((0, 1, 2, 3)), hasPadded=bit(0.3), hasHybrid=bit(0.7), hasTrisPadded=bit(0.7),
              probeMemoryOn=bit(0.8), skipTiming=bit(0.2))
