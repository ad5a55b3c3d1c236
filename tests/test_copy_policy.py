"""When a scene's derived copies are dropped, kept and made again is plain arithmetic (tinybvh_amd/csrc/copy_policy.h: CopyPolicy) that needs no device:
tests/copy_policy_driver.cpp, a host program that includes that header alone, replays events and prints the state after each.  The expected states below are
written out from the rules (four queries bring the copies back, a drop soon after a remake quadruples that up to 2^20, a refit drops the copies when fewer
than 8 Mi rays were traced since the previous one); none is read back from the struct.  The same rules on the device, by `device_bytes`:
test_bvh_gpu_wide_copy.py, test_refit_device.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tinybvh_amd", "csrc")
KEEP = 8 << 20      # kRefitKeepRays
CAP = 1 << 20       # where recopyAfter stops growing


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("copy_policy") / "copy_policy_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, os.path.join(HERE, "copy_policy_driver.cpp"), "-o", exe])
    return exe


def run(driver, events):
    """One fresh CopyPolicy per call.  Per event: (result, first, pendingCopies, recopyAfter, queriesSinceUpdate, remadeSinceUpdate, raysAtRefit, refitSeen)."""
    out = subprocess.run([driver], input="\n".join(events) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert len(rows) == len(events)
    return rows


def test_four_queries_bring_the_copies_back(driver):
    assert run(driver, ["d 3", "q", "q", "q", "q", "q"]) == [
        (0, 0, 3, 4, 0, 0, 0, 0),
        (0, 0, 3, 4, 1, 0, 0, 0),
        (0, 0, 3, 4, 2, 0, 0, 0),
        (0, 0, 3, 4, 3, 0, 0, 0),
        (3, 1, 0, 4, 4, 1, 0, 0),     # the fourth query returns both kinds, once
        (0, 0, 0, 4, 4, 1, 0, 0),     # nothing pending: a query counts nothing
    ]


def test_a_drop_straight_after_a_remake_quadruples_the_wait(driver):
    assert run(driver, ["d 3", "q 4", "d 3", "q 15", "q", "d 3", "q 63", "q"]) == [
        (0, 0, 3, 4, 0, 0, 0, 0),
        (3, 4, 0, 4, 4, 1, 0, 0),
        (0, 0, 3, 16, 0, 0, 0, 0),
        (0, 0, 3, 16, 15, 0, 0, 0),
        (3, 1, 0, 16, 16, 1, 0, 0),
        (0, 0, 3, 64, 0, 0, 0, 0),
        (0, 0, 3, 64, 63, 0, 0, 0),
        (3, 1, 0, 64, 64, 1, 0, 0),
    ]


def test_the_wait_stops_growing_at_2_to_the_20(driver):
    waits = [min(4 ** k, CAP) for k in range(1, 14)]
    assert waits[9] == CAP and waits[8] == CAP // 4 and waits[-1] == CAP
    events, want = [], []
    for w in waits:
        events += ["d 3", f"q {w}"]
        want += [(0, 0, 3, w, 0, 0, 0, 0), (3, w, 0, w, w, 1, 0, 0)]     # the w-th query, no earlier one, brings them back
    assert run(driver, events) == want


def test_drops_without_a_remake_between_them_do_not_grow_the_wait(driver):
    assert run(driver, ["d 1", "q 2", "d 2", "q 3", "q"]) == [
        (0, 0, 1, 4, 0, 0, 0, 0),
        (0, 0, 1, 4, 2, 0, 0, 0),
        (0, 0, 3, 4, 0, 0, 0, 0),     # the kinds add up, the count starts again, the wait stays
        (0, 0, 3, 4, 3, 0, 0, 0),
        (3, 1, 0, 4, 4, 1, 0, 0),
    ]


def test_nothing_to_drop_changes_nothing(driver):
    assert run(driver, ["d 0", "d 3", "q 4", "d 0", "d 1"]) == [
        (0, 0, 0, 4, 0, 0, 0, 0),
        (0, 0, 3, 4, 0, 0, 0, 0),
        (3, 4, 0, 4, 4, 1, 0, 0),
        (0, 0, 0, 4, 4, 1, 0, 0),     # not even "remade since the update" is forgotten ...
        (0, 0, 1, 16, 0, 0, 0, 0),        # ... so the next real drop still counts as one soon after a remake
    ]


def test_refit_keeps_or_drops_by_the_rays_traced_since_the_previous_one(driver):
    assert run(driver, ["r 1000 1", f"r {1000 + KEEP} 1", f"r {1000 + 2 * KEEP - 1} 1", f"r {1000 + 2 * KEEP} 0", f"r {1000 + 2 * KEEP + 1} 1"]) == [
        (0, 0, 0, 4, 0, 0, 1000, 1),                     # the first refit has nothing to compare with
        (0, 0, 0, 4, 0, 0, 1000 + KEEP, 1),              # exactly 8 Mi rays since: kept
        (1, 0, 0, 4, 0, 0, 1000 + 2 * KEEP - 1, 1),      # one ray fewer: dropped (the caller then reports the drop with dropped())
        (0, 0, 0, 4, 0, 0, 1000 + 2 * KEEP, 1),          # no copies: nothing to drop, the count is recorded all the same ...
        (1, 0, 0, 4, 0, 0, 1000 + 2 * KEEP + 1, 1),      # ... and is what the next refit compares with
    ]


def test_refit_without_copies_never_drops(driver):
    assert run(driver, ["r 5 0", "r 6 0", f"r {6 + KEEP} 0", "r 0 0"]) == [
        (0, 0, 0, 4, 0, 0, 5, 1),
        (0, 0, 0, 4, 0, 0, 6, 1),
        (0, 0, 0, 4, 0, 0, 6 + KEEP, 1),
        (0, 0, 0, 4, 0, 0, 0, 1),
    ]
