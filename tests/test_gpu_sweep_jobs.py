"""Sweep jobs on the GPU (npow_submit_sweep / npow_wait_sweep): a range's hits enumerated by the pool
kernel's dense mapping, inside the launches that answer searches.

Hit-set equality is the direct statement about that mapping (b = it * K + j over the entry's own
workgroups, the ragged last block, ranges stitched over launches): every nonce hashed exactly once, every
compare right.  The references are the hashlib-pinned fixtures of tests/golden and the C oracle; the shapes
are the smallest at which the mapping can go wrong (a grid iteration covers 2^19 nonces, a workgroup row
512, a wave block 64).  Everything runs on device 0 except the CU-partition test (tests/sweep_job_worker.py).
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest

import oracle
from conftest import ROOT, load_golden
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE, AUDIT = 0xfffffe0000000000, 0xffff000000000000
CAP = _lib.NPOW_SWEEP_JOB_HITS
ROOT_A = bytes(range(3, 35))
RAGGED = [1, 63, 64, 65, 511, 512, 513, 4097, 65537]
ODD_START = 0x0123456789abcdef


@functools.lru_cache(maxsize=None)
def ref(root, threshold, start, count):
    """oracle.sweep, computed once per range and shared (a tuple: nobody changes it)."""
    return tuple(oracle.sweep(root, threshold, start, count, threads=min(16, os.cpu_count() or 1)))


def small_cases():
    """The two 2^24 cases and the wrap-around case (ffffffffffc00000 + 2^23, 111 hits) of sweeps_small.json."""
    cases = load_golden("sweeps_small.json")["cases"][-3:]
    assert [c["count"] for c in cases] == [1 << 24, 1 << 24, 1 << 23] and cases[2]["start"] == "ffffffffffc00000"
    assert len(cases[2]["hits"]) == 111
    return cases


def submit_case(eng, c, **kw):
    return eng.submit_sweep(bytes.fromhex(c["root"]), int(c["threshold"], 16), int(c["start"], 16), c["count"],
                            device_mask=1, **kw)


def check_case(res, c):
    assert res is not None and res.status == _lib.NPOW_OK
    assert [f"{h:016x}" for h in res.hits] == c["hits"], c["method"]
    assert res.total == len(c["hits"]) and res.nonces_done == c["count"]


def search_ok(eng, root, thr):
    r = eng.submit(root, thr, device_mask=1).wait(60)
    assert r is not None and r.status == _lib.NPOW_OK
    assert oracle.work_value_hashlib(root, r.nonce) == r.value >= thr


# -- 1. fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2])
def test_small_fixtures_and_device_counter(gpu_engine, i):
    c = small_cases()[i]
    gpu_engine.reset_stats(0)
    check_case(submit_case(gpu_engine, c).wait(60), c)
    assert gpu_engine.stats(0).nonces == c["count"]  # a lone job: the device hashed the range and nothing else


def test_2p30_hashlib_fixture(gpu_engine):
    g = load_golden("sweep_2p30_hashlib.json")
    check_case(submit_case(gpu_engine, g, cap=1 << 12).wait(60), g)


# -- 2. every lane, ragged ends -------------------------------------------------------------------------
def test_every_lane_is_a_hit_ragged_counts(gpu_engine):
    """Threshold 0: every wave mask is full, the hits are the range itself (the jobs share their launches)."""
    ts = [gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, n, device_mask=1, cap=n) for n in RAGGED]
    for n, t in zip(RAGGED, ts):
        r = t.wait(60)
        assert r is not None and r.status == _lib.NPOW_OK, n
        assert r.hits == list(range(ODD_START, ODD_START + n)), n
        assert r.total == n and r.nonces_done == n


def test_a_quarter_of_the_lanes_ragged_counts(gpu_engine):
    thr = 0xc000000000000000
    ts = [gpu_engine.submit_sweep(ROOT_A, thr, ODD_START, n, device_mask=1, cap=n) for n in RAGGED]
    for n, t in zip(RAGGED, ts):
        r = t.wait(60)
        want = list(ref(ROOT_A, thr, ODD_START, n))
        assert r is not None and r.status == _lib.NPOW_OK, n
        assert r.hits == want and r.total == len(want) and r.nonces_done == n, n


# -- 3. capacity ----------------------------------------------------------------------------------------
def test_more_hits_than_a_device_keeps(gpu_engine):
    count = CAP + 64
    r = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, count, device_mask=1, cap=count).wait(120)
    assert r is not None and r.status == _lib.NPOW_ERR_CAPACITY
    assert r.total == count and r.nonces_done == count  # the count stays exact
    assert r.hits[:CAP] == list(range(ODD_START, ODD_START + CAP))  # the first CAP nonces of the range
    search_ok(gpu_engine, ROOT_A, RECEIVE)  # the device still serves


def test_more_hits_than_the_caller_takes(gpu_engine):
    r = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, 4097, device_mask=1, cap=1000).wait(60)
    assert r is not None and r.status == _lib.NPOW_ERR_CAPACITY
    assert r.total == 4097 and r.hits == list(range(ODD_START, ODD_START + 1000))


# -- 4. many launches -----------------------------------------------------------------------------------
def test_nothing_lost_or_doubled_at_launch_boundaries(gpu_engine):
    """16 iterations per launch: the 2^24 range takes several launches, two of them in flight."""
    gpu_engine.set_tuning(16, 0, 0)
    try:
        gpu_engine.reset_stats(0)
        r = gpu_engine.submit_sweep(ROOT_A, AUDIT, 0, 1 << 24, device_mask=1).wait(60)
        launches = gpu_engine.stats(0).launches
    finally:
        gpu_engine.set_tuning(8192, 0, 0)
    want = list(ref(ROOT_A, AUDIT, 0, 1 << 24))
    assert r is not None and r.status == _lib.NPOW_OK
    assert r.hits == want and r.total == len(want) and r.nonces_done == 1 << 24
    assert launches >= 3, launches


# -- 5. beside searches ---------------------------------------------------------------------------------
def test_exact_beside_searches(gpu_engine):
    tok = _lib.CancelToken()
    endless = [gpu_engine.submit(bytes([i]) * 32, M64, start=i << 50, device_mask=1, cancel=tok) for i in range(4)]
    roots = [bytes([0x40 + i]) * 32 for i in range(2)]
    searches = [gpu_engine.submit(r, RECEIVE, device_mask=1) for r in roots]
    cases = small_cases()
    sweeps = [submit_case(gpu_engine, cases[0]), submit_case(gpu_engine, cases[2]),
              gpu_engine.submit_sweep(ROOT_A, AUDIT, 0, 1 << 22, device_mask=1)]
    check_case(sweeps[0].wait(60), cases[0])
    check_case(sweeps[1].wait(60), cases[2])
    r = sweeps[2].wait(60)
    want = list(ref(ROOT_A, AUDIT, 0, 1 << 22))
    assert r.status == _lib.NPOW_OK and r.hits == want and r.nonces_done == 1 << 22
    for root, t in zip(roots, searches):
        s = t.wait(60)
        assert s is not None and s.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(root, s.nonce) == s.value >= RECEIVE
    tok.set()
    for t in endless:
        assert t.wait(30).status == _lib.NPOW_CANCELLED


# -- 6. one root, overlapping ranges ----------------------------------------------------------------------
def test_two_jobs_of_one_root_over_overlapping_ranges(gpu_engine):
    """Hits are attributed by slot and generation, not by root or nonce."""
    a = gpu_engine.submit_sweep(ROOT_A, AUDIT, 0, 1 << 22, device_mask=1)
    b = gpu_engine.submit_sweep(ROOT_A, AUDIT, 1 << 21, 1 << 22, device_mask=1)
    ra, rb = a.wait(60), b.wait(60)
    assert ra.status == rb.status == _lib.NPOW_OK
    assert ra.hits == list(ref(ROOT_A, AUDIT, 0, 1 << 22))
    assert rb.hits == list(ref(ROOT_A, AUDIT, 1 << 21, 1 << 22))
    assert set(ra.hits) & set(rb.hits)  # the overlap holds hits: both jobs report them


# -- 7. cancel --------------------------------------------------------------------------------------------
def test_cancel_returns_what_was_found(gpu_engine):
    start, count, thr = 5 << 44, 1 << 40, 0xfffff00000000000
    t = gpu_engine.submit_sweep(ROOT_A, thr, start, count, device_mask=1)
    assert t.wait(0.05) is None  # NPOW_PENDING: the ticket stays valid
    t.cancel()
    r = t.wait(30)
    assert r is not None and r.status == _lib.NPOW_CANCELLED
    assert 0 < r.nonces_done < count
    assert r.total == len(r.hits)
    offs = [(h - start) & M64 for h in r.hits]
    assert all(o < count for o in offs) and all(x < y for x, y in zip(offs, offs[1:]))
    assert all(oracle.work_value(ROOT_A, h) >= thr for h in r.hits)
    search_ok(gpu_engine, ROOT_A, RECEIVE)


# -- 8. wrong calls -----------------------------------------------------------------------------------------
def test_other_calls_refuse_a_sweep_ticket(gpu_engine):
    lib = gpu_engine.lib
    c = small_cases()[2]
    t = submit_case(gpu_engine, c)
    bad = _lib.NPOW_ERR_BAD_ARGUMENT
    u32, u64 = ctypes.c_uint32(0), ctypes.c_uint64(0)
    info = _lib.SearchInfo()
    info.size = ctypes.sizeof(info)
    rinfo = _lib.ReserveInfo()
    rinfo.size = ctypes.sizeof(rinfo)
    assert lib.npow_promote(t.ticket, 2) == bad
    assert lib.npow_retarget(t.ticket, M64) == bad
    assert lib.npow_relax(t.ticket, 0xfffff00000000000, ctypes.byref(u32)) == bad
    assert lib.npow_ticket_reserve(t.ticket, ctypes.byref(rinfo)) == bad
    assert lib.npow_ticket_background(t.ticket, ctypes.byref(u32)) == bad
    assert lib.npow_wait(t.ticket, 0, ctypes.byref(u64), ctypes.byref(u64), ctypes.byref(u64)) == bad
    assert lib.npow_wait_info(t.ticket, 0, ctypes.byref(info)) == bad
    assert lib.npow_wait_result(t.ticket, 0, ctypes.byref(u64), ctypes.byref(u64)) == bad
    assert lib.npow_last_error()
    check_case(t.wait(60), c)  # still collectable, and exact
    # npow_wait_sweep on a search's ticket
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
    n = ctypes.c_uint64(0)
    assert lib.npow_wait_sweep(s.ticket, 0, None, 0, ctypes.byref(n), None) == bad
    res = s.wait(60)
    assert res.status == _lib.NPOW_OK and oracle.work_value_hashlib(ROOT_A, res.nonce) == res.value >= RECEIVE


def test_empty_range_completes_at_once(gpu_engine):
    gpu_engine.reset_stats(0)
    r = gpu_engine.submit_sweep(ROOT_A, 0, 12345, 0, device_mask=1).wait(0)
    assert r is not None and r.status == _lib.NPOW_OK and r.hits == [] and r.total == 0 and r.nonces_done == 0
    assert gpu_engine.stats(0).nonces == 0 and gpu_engine.stats(0).launches == 0


# -- 9. CU partitions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 4])
def test_split_over_cu_partitions(g):
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES=str(g), NANOPOW_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweep_job_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["ok"] and out["devices"] == g and out["nonces_done"] == (1 << 22) + 3
    checks, failures = out["affinity"]  # the test hooks' device-affinity check of every HIP call site
    assert checks > 0 and failures == 0, out["affinity"]
    assert sum(out["nonces_per_device"]) == (1 << 22) + 3 and all(n > 0 for n in out["nonces_per_device"])
