"""The hit branch of the pool kernel (npow_kernel.hip pool_body_ls2, ``if (hits != 0)``) under dense lane masks and a
fixed order of events: the floor-record read, the keep / stale split with its popcount, the win lane taken after the
split, and the armed rule of a search with a reserve.  The other GPU tests reach this branch with one hit lane per
wave and with the order "floor record written, then a wave hits" left to a sleep.  Run on an MI355X: ``pytest -m gpu``.

The method (tests/hit_branch_worker.py has the flow): a background search B is parked beside two endless foreground
searches in one counted launch -- its entry built with a LOW threshold T0 -- its threshold is moved while it is
parked (the slot's floor record is written), and the foreground searches are cancelled.  Every workgroup then joins
B once: a workgroup leaves a foreground entry only when it is dead, picks a live foreground entry ahead of any
background one, and never leaves the last live entry.  So each of the launch's W = 8 * grid waves hashes its first
block of B under the watch threshold T0 with the record already there, and what the branch does with that block is
derived from the code, not measured:

  T0 = 0, T1 = 2^64 - 1     all 64 lanes hit, none qualifies, the wave adopts T1: stale_hits == 64 * W exactly
  T0 = c000..., T1 = 2^64-1 the first block with a hit (all but (3/4)^64 of them) has Binomial(64, 1/4) hit lanes
  T0 = 0, T1 = f000...      a wave with a lane at or above T1 (all but (15/16)^64 = 1.6 % of them) wins with that lane

Each case runs with B as a table entry and as a dynamic entry: the branch re-reads the entry's threshold, reserve,
slot and generation through the cursor's pointer, from the kernel arguments in one and from pinned host memory in the
other.
"""
import json
import math
import os
import subprocess
import sys
import time

import pytest

import hit_branch_worker as hb
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = hb.M64
RMIN = 0xfffff00000000000  # NPOW_RESERVE_MIN
L = 0xffffff0000000000
HERE = os.path.dirname(os.path.abspath(__file__))
HOW = ["table", "dynamic"]


def _show(name, out):
    print(f"{name}: stale_hits {out['stale_hits']} (W {out['waves']}, 64 W {64 * out['waves']}, 16 W "
          f"{16 * out['waves']}), nonces_done {out['nonces_done']}, stale_wins {out['stale_wins']}, retargets "
          f"{out['retargets']}, status {out['status']}, value {out['value']:016x}; per device (launches, yields) at the "
          f"release {[(d['launches'], d['yields']) for d in out['release']]}, before the end "
          f"{[(d['launches'], d['yields']) for d in out['end']]}, after it "
          f"{[(d['launches'], d['yields']) for d in out['after']]}")


def _protocol_checks(out):
    for b, r, e, a in zip(out["before"], out["release"], out["end"], out["after"]):
        assert (e["launches"], e["yields"]) == (r["launches"], r["yields"]), "a launch ended under B, or a yield"
        assert a["yields"] == r["yields"]
        assert a["stale_missing"] == 0 and a["early_mismatches"] == 0 and a["dead"] == 0
        assert a["invalid_work"] == b["invalid_work"]


def _every_lane_stale(out):
    """What test 1 asserts, of one run of its flow."""
    assert out["held"] is True, "B was decided while it was parked: a parked entry was hashed"
    assert out["status"] == _lib.NPOW_CANCELLED and out["background"] == 1
    assert out["stale_hits"] == 64 * out["waves"]
    assert out["stale_wins"] == 0 and out["retargets"] == 1
    assert out["nonces_done"] >= out["stale_hits"] and out["nonces_done"] % 64 == 0
    _protocol_checks(out)


@pytest.mark.parametrize("how", HOW)
def test_every_lane_stale(gpu_engine, how):
    """T0 = 0, T1 = 2^64 - 1, B cancelled 20 ms after the release.  Every wave joins B once; its first block has 64
    hit lanes, none at or above T1, and the wave then adopts T1 and hits no more: stale_hits == 64 * W, exactly."""
    out = hb.raised_while_parked(gpu_engine, 121, how, 0, M64)
    _show(f"every lane stale, {how}", out)
    _every_lane_stale(out)


@pytest.mark.parametrize("how", HOW)
def test_partial_masks(gpu_engine, how):
    """T0 = c000000000000000 (a lane hits with p = 1/4), T1 = 2^64 - 1.  A wave's stale count is the popcount of the
    first block in which it has a hit; values are BLAKE2b output, so the sum over W waves is Binomial(64 W, 1/4) but
    for the (3/4)^64 = 1e-8 of blocks without a hit: mean 16 W, variance 12 W, bound 5 sigma.  A count of 1 per wave,
    or of all 64 lanes, is hundreds of sigma away."""
    out = hb.raised_while_parked(gpu_engine, 122, how, 0xc000000000000000, M64)
    _show(f"partial masks, {how}", out)
    w = out["waves"]
    assert out["held"] is True, "B was decided while it was parked: a parked entry was hashed"
    assert out["status"] == _lib.NPOW_CANCELLED
    assert abs(out["stale_hits"] - 16 * w) <= 5 * math.sqrt(12 * w), (out["stale_hits"], 16 * w)
    assert out["stale_wins"] == 0 and out["retargets"] == 1
    assert out["nonces_done"] >= out["stale_hits"] and out["nonces_done"] % 64 == 0
    _protocol_checks(out)


@pytest.mark.parametrize("how", HOW)
def test_win_lane_after_the_split(gpu_engine, how):
    """T0 = 0, T1 = f000000000000000: every lane of a wave's first block hits, about 4 of them qualify, and the win
    lane must be one of those -- taken from the unfiltered mask it is lane 0, whose value is below T1 in 15 waves of
    16; the host refuses such a win and counts it (stale_wins).  Which qualifying lane wins is not asserted: lanes
    and waves race.

    The counts are tied as well.  A workgroup's 8 waves hash in step and leave together before the hash after a win,
    and a workgroup none of whose 512 first lanes qualifies is one in 2^48: so every wave that hashed B hashed one
    block of it, and added its lanes below T1 right before it left the entry.  stale_hits is therefore nonces_done
    less the qualifying lanes, Binomial(nonces_done, 1/16); bound 5 sigma.  An add that a leaving wave lost -- nearly
    every add here is a wave's last act on the entry -- falls out of it."""
    out = hb.raised_while_parked(gpu_engine, 123, how, 0, 0xf000000000000000, run_ms=None)
    _show(f"win lane, {how}", out)
    assert out["held"] is True, "B was decided while it was parked: a parked entry was hashed"
    assert out["status"] == _lib.NPOW_OK
    assert out["hashlib"] == out["value"] >= 0xf000000000000000
    assert out["stale_wins"] == 0 and out["retargets"] == 1
    assert 0 < out["stale_hits"] <= out["nonces_done"]
    n = out["nonces_done"]
    assert n % 64 == 0 and abs(out["stale_hits"] - n * 15 / 16) <= 5 * math.sqrt(n * 15 / 256), (out["stale_hits"], n)
    for b, r, a in zip(out["before"], out["release"], out["after"]):
        assert a["invalid_work"] == b["invalid_work"] and a["yields"] == r["yields"]
        assert a["stale_missing"] == 0 and a["early_mismatches"] == 0 and a["dead"] == 0


@pytest.mark.parametrize("how", HOW)
def test_slot_reuse(gpu_engine, how):
    """The first test's flow twice: the same exact count both times.  The slot's stale word on the device is
    cumulative and the host credits its gain over a baseline (Slot::stale_base): a baseline error doubles the
    second count."""
    outs = [hb.raised_while_parked(gpu_engine, 124 + i, how, 0, M64) for i in range(2)]
    for i, out in enumerate(outs):
        _show(f"slot reuse, {how}, run {i}", out)
        _every_lane_stale(out)
    assert outs[0]["stale_hits"] == outs[1]["stale_hits"]


def _armed(eng, seed, how, moves):
    """B armed (threshold 2^64 - 1, reserve RMIN), parked; `moves` applied to it while parked; released; it ends by
    itself.  Returns (what the moves returned, candidates before the release, reserve info, search info, root)."""
    jobs = hb.Jobs(eng, seed)
    with hb.one_long_launch(eng, jobs):
        inv0 = eng.stats(0).invalid_work
        b = hb.park(eng, jobs, how, M64, reserve=RMIN)
        answers = [getattr(b, name)(thr) for name, thr in moves]
        parked = b.reserve_info()
        hb.release(eng, jobs)
        assert b.wait_result(30) is not None
        ri = b.reserve_info()
        info = b.wait_info(30)
        st = eng.stats(0)
    print(f"armed, {how}, {[(name, f'{thr:016x}') for name, thr in moves]}: answers {answers}, candidates parked {parked.candidates} -> {ri.candidates}, result "
          f"{info.nonce:x} {info.value:016x}, reserve {ri.nonce:x} {ri.value:016x}, threshold {ri.threshold:016x}, "
          f"stale_hits {info.stale_hits}, stale_wins {info.stale_wins}, retargets {info.retargets}, nonces_done "
          f"{info.nonces_done}")
    assert parked.candidates == 0 and parked.value == 0, "a parked entry was hashed"
    assert info.status == _lib.NPOW_OK
    assert hb.value(jobs.roots[3], info.nonce) == info.value
    assert st.invalid_work == inv0 and st.stale_missing == 0 and st.early_mismatches == 0 and st.dead == 0
    return answers, ri, info, jobs.roots[3]


@pytest.mark.parametrize("how", HOW)
def test_armed_relaxed_while_parked(gpu_engine, how):
    """relax(L) on the parked entry: lowered in place (False).  The waves watch at RMIN, find the record and split
    their hit lanes at L: at or above it a win, below it a reserve candidate, and none stale -- an armed entry's own
    threshold is 2^64 - 1, which no candidate meets.  Some 15 candidates in [RMIN, L) are met before the first win
    (2^-20 against 2^-24 per nonce), so stale_hits == 0 here is what the `value >= ethr` term of the stale mask is
    for: in a search without a reserve every hit lane meets it already, and no test of those can see it go."""
    answers, ri, info, root = _armed(gpu_engine, 126, how, [("relax", L)])
    assert answers == [False]
    assert info.value >= L
    assert ri.threshold == L and ri.answered == 0 and ri.relaxes == 1
    if ri.value:  # (a reserve the host harvested before the win)
        assert RMIN <= ri.value < L and hb.value(root, ri.nonce) == ri.value
    assert info.stale_hits == 0 and info.stale_wins == 0 and info.retargets == 0


@pytest.mark.parametrize("how", HOW)
def test_armed_relaxed_then_retargeted_while_parked(gpu_engine, how):
    """relax(RMIN) then retarget(L), both on the parked entry: with no hash between them the outcome is fixed --
    lowered in place, the raise holds, the result is at or above L.  (tests/test_gpu_reserve.py's test_both_ways
    makes the same two calls on a running search and has to accept either order.)"""
    answers, ri, info, _ = _armed(gpu_engine, 127, how, [("relax", RMIN), ("retarget", L)])
    assert answers == [False, True]
    assert info.value >= L
    assert ri.threshold == L and ri.answered == 0 and ri.relaxes == 1
    assert info.retargets == 1 and info.stale_hits == 0 and info.stale_wins == 0


@pytest.mark.parametrize("how", HOW)
def test_armed_raised_while_parked(gpu_engine, how):
    """B armed with threshold L and reserve RMIN, retarget(2^64 - 1) on the parked entry, released, cancelled 60 ms
    later.  No launch ended under B, so one entry built with ethr = L did all the hashing: every lane in [L, 2^64 - 1)
    met the entry's threshold and not the current one -- a stale hit, counted and passed over, and NO reserve
    candidate: for the rest of the launch in which an armed search is raised, the reserve takes values in
    [reserve, the threshold the launch's entry was built with) only (include/nanopow.h npow_retarget; DESIGN.md §1
    "Reserve hits").  So with n = nonces_done >= 2^30 the reserve holds a value in [RMIN, L) -- some 2^10 candidates
    -- and none at or above L, although about n / 2^24 >= 64 such nonces were passed: stale_hits, which is
    Binomial(n, 2^-24) exactly (L = ffffff0000000000), bound 5 sigma.

    Making those lanes candidates as well (`cand = hits & ~keep` for an armed entry) would let a later npow_relax to a
    level among them be answered at once; it changes the text of the unbounded search kernels, which
    tests/test_best_kernel_census.py pins instruction for instruction, and was not taken.  Then this test turns
    round: a reserve at or above L, P(none) = exp(-n / 2^24) <= e^-64."""
    eng = gpu_engine
    jobs = hb.Jobs(eng, 128)
    with hb.one_long_launch(eng, jobs):
        before = hb.settled(eng, [0])
        b = hb.park(eng, jobs, how, L, reserve=RMIN)
        held = b.retarget(M64)
        parked = b.reserve_info()
        rel = hb.release(eng, jobs)
        time.sleep(0.06)  # (~2^31 nonces of a whole GPU; the precondition below is what counts)
        end = [eng.stats(0)]  # (before B ends: its launch retires right after it)
        ri = b.reserve_info()
        jobs.toks[3].set()
        info = b.wait_info(30)
        assert info is not None
        after = [eng.stats(0)]
    n = info.nonces_done
    print(f"armed, raised while parked, {how}: held {held}, nonces_done {n} (2^{math.log2(max(n, 1)):.2f}), stale_hits "
          f"{info.stale_hits} (n / 2^24 = {n / 2 ** 24:.1f}), reserve {ri.nonce:x} {ri.value:016x}, candidates "
          f"{ri.candidates}, threshold {ri.threshold:016x}, retargets {info.retargets}, stale_wins {info.stale_wins}")
    assert held is True and parked.candidates == 0 and parked.value == 0, "a parked entry was hashed"
    assert info.status == _lib.NPOW_CANCELLED and info.retargets == 1 and info.stale_wins == 0
    _protocol_checks({"before": [hb.device_counts(s) for s in before], "release": [hb.device_counts(s) for s in rel],
                      "end": [hb.device_counts(s) for s in end], "after": [hb.device_counts(s) for s in after]})
    assert n >= 1 << 30 and n % 64 == 0, "precondition: the search hashed too little for the bound below"
    assert ri.armed == 1 and ri.reserve_threshold == RMIN and ri.threshold == M64 and ri.answered == 0
    assert abs(info.stale_hits - n / 2 ** 24) <= 5 * math.sqrt(n / 2 ** 24), (info.stale_hits, n / 2 ** 24)
    assert RMIN <= ri.value < L and hb.value(jobs.roots[3], ri.nonce) == ri.value, \
        f"the reserve after {n} nonces under an entry built with L: {ri.value:016x}"
    assert ri.candidates >= 1


def test_two_cu_partitions():
    """The first test's flow on searches split over two CU partitions (device_mask 3), in a child process: each
    device has its own floor record and stale words, and the job's count is their sum."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "hit_branch_worker.py")],
                       env=dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2"), capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    _show("two partitions", out)
    assert out["n_devices"] == 2 and len(out["after"]) == 2
    assert out["waves"] == 8 * (out["after"][0]["grid"] + out["after"][1]["grid"])
    _every_lane_stale(out)
