"""Best jobs on the GPU (npow_submit_best / npow_wait_best): the strongest nonce of a range, found inside the pool's
launches by waves that chase the best value so far.

The reference is the C oracle's work values of the range (argmax, first occurrence on ties) and hashlib for the
returned value.  The shapes are the smallest at which the kernel's branch and the host's fold can go wrong: ragged
ends (a wave block is 64 nonces, a workgroup row 512, a grid iteration 2^19 on a whole MI355X), the maximum in the
first and in the last lane of a range, ranges stitched over several launches with the maximum in the first and in the
last of them, the wrap at 2^64.  Everything runs on device 0 except the CU-partition test (tests/best_job_worker.py).

The records each launch appended are written to bench_out/best_records.jsonl; the only assertion on them is that no
launch's entry appended more than its region holds.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_golden
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE = 0xfffffe0000000000
ROOT_A = bytes(range(3, 35))
START = 0x0123456789abcdef
N = 1 << 22
RAGGED = [1, 63, 64, 65, 511, 512, 513, 4097, 65537, 1 << 19, (1 << 19) + 1]
OUT = os.path.join(ROOT, "bench_out")


@functools.lru_cache(maxsize=None)
def values(root=ROOT_A, start=START, count=N):
    """The oracle's work values of the range, computed once and shared (read-only)."""
    v = oracle.work_values_range(root, start, count)
    v.setflags(write=False)
    return v


def want(off, count, root=ROOT_A, start=START, n=N):
    """(nonce, value) of the strongest nonce of [start + off, start + off + count): argmax, first occurrence."""
    v = values(root, start, n)[off:off + count]
    k = int(np.argmax(v))
    return (start + off + k) & M64, int(v[k])


def log_records(test, info, **kw):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "best_records.jsonl"), "a") as f:
        f.write(json.dumps({"test": test, "count": info.count, "launches": info.launches, "records": info.records,
                            "records_max": info.records_max, "room": info.room, **kw}) + "\n")


def finish(t, timeout=60.0):
    """The job's last look (npow_ticket_best, once it has finished) and its result."""
    deadline = time.time() + timeout
    info = t.info()
    while not info.finished and time.time() < deadline:
        time.sleep(0.0005)
        info = t.info()
    assert info.finished, info
    assert info.records_max <= info.room or info.launches == 0, info  # never above the region's room
    return t.wait(5), info


def check(res, off, count, **kw):
    nonce, value = want(off, count, **kw)
    assert res is not None and res.status == _lib.NPOW_OK, res
    assert (res.nonce, res.value, res.nonces_done) == (nonce, value, count), (off, count)
    assert oracle.work_value_hashlib(kw.get("root", ROOT_A), res.nonce) == res.value


# -- 1. ragged counts -----------------------------------------------------------------------------------
def test_ragged_counts_share_launches(gpu_engine):
    ts = [gpu_engine.submit_best(ROOT_A, START, n, device_mask=1) for n in RAGGED]
    for n, t in zip(RAGGED, ts):
        res, info = finish(t)
        log_records("ragged", info)
        check(res, 0, n)
        assert info.room >= 1 << 14


# -- 2. the maximum at the edges ------------------------------------------------------------------------
def test_maximum_at_the_edges_and_just_outside(gpu_engine):
    m = int(np.argmax(values()))
    cases = [(0, m + 1),      # the maximum in the last lane of a ragged tail
             (m, N - m)]      # ... in the first lane
    if m > 0:
        cases.append((0, m))  # the true maximum excluded: the runner-up
    if m + 1 < N:
        cases.append((m + 1, N - m - 1))
    ts = [gpu_engine.submit_best(ROOT_A, START + off, n, device_mask=1) for off, n in cases]
    for (off, n), t in zip(cases, ts):
        res, info = finish(t)
        log_records("edges", info, offset=off)
        check(res, off, n)
    assert want(0, m + 1)[0] == want(m, N - m)[0] == START + m
    if len(cases) == 4:
        assert START + m not in (want(*cases[2])[0], want(*cases[3])[0])


# -- 3. stitching ---------------------------------------------------------------------------------------
def _window(span, last):
    """A window (offset, count) of the oracle array that a lone job hashes in 3 or 4 launches of `span` nonces, with
    its maximum in the first launch's part -- or, `last`, in the last launch's part.  The longest such window, at
    the lowest offset on a grid of span / 8."""
    v = values()
    for n in (4 * span, 7 * span // 2, 3 * span, 5 * span // 2):
        launches = -(-n // span)
        for a in range(0, N - n + 1, span // 8):
            k = int(np.argmax(v[a:a + n]))
            if (k >= (launches - 1) * span) if last else (k < span):
                return a, n
    raise AssertionError("no window of the oracle array has its maximum there")


def test_best_is_kept_and_displaced_across_launches(gpu_engine):
    """One wave iteration per launch (npow_set_tuning(2): with 32, as the position tests use, a whole MI355X covers
    2^23 nonces per launch and the 2^22 range would take one): a lone job of 2.5 to 4 launch spans, cut from the
    oracle array, takes 3 or 4 launches.  With the maximum in the first launch's part the early best must survive the
    later launches; with it in the last launch's part it must displace what the earlier ones found."""
    span = gpu_engine.stats(0).grid * 8 * 64  # the nonces one wave iteration of the device covers
    assert 4 * span <= N, span
    gpu_engine.set_tuning(2, 0, 0)
    try:
        for last in (False, True):
            off, n = _window(span, last)
            res, info = finish(gpu_engine.submit_best(ROOT_A, START + off, n, device_mask=1))
            log_records("stitching_last" if last else "stitching_first", info, offset=off)
            check(res, off, n)
            k = (res.nonce - START - off) & M64
            assert (k >= (-(-n // span) - 1) * span) if last else (k < span), (k, span, n)
            assert info.launches >= 3, info
    finally:
        gpu_engine.set_tuning(8192, 0, 0)


def test_position_test_tuning_beside_another_job(gpu_engine):
    """npow_set_tuning(32, 0, 0) as the position tests use it, the whole 2^22 array and a second job beside it."""
    gpu_engine.set_tuning(32, 0, 0)
    try:
        a = gpu_engine.submit_best(ROOT_A, START, N, device_mask=1)
        b = gpu_engine.submit_best(ROOT_A, START + 12345, N // 2 + 77, device_mask=1)
        for t, off, n in ((a, 0, N), (b, 12345, N // 2 + 77)):
            res, info = finish(t)
            log_records("tuning32", info, offset=off)
            check(res, off, n)
    finally:
        gpu_engine.set_tuning(8192, 0, 0)


# -- 4. floor -------------------------------------------------------------------------------------------
def test_floor_at_and_above_the_maximum(gpu_engine):
    n = 65537
    nonce, value = want(0, n)
    r = gpu_engine.submit_best(ROOT_A, START, n, floor=value, device_mask=1).wait(60)
    assert tuple(r) == (_lib.NPOW_OK, nonce, value, n)
    r = gpu_engine.submit_best(ROOT_A, START, n, floor=value + 1, device_mask=1).wait(60)
    assert tuple(r) == (_lib.NPOW_EXHAUSTED, None, None, n)


# -- 5. wrap --------------------------------------------------------------------------------------------
def test_range_across_the_wrap(gpu_engine):
    c = load_golden("sweeps_small.json")["cases"][-1]
    assert c["start"] == "ffffffffffc00000" and c["count"] == 1 << 23
    root, start, n = bytes.fromhex(c["root"]), int(c["start"], 16), c["count"]
    res, info = finish(gpu_engine.submit_best(root, start, n, device_mask=1))
    log_records("wrap", info)
    check(res, 0, n, root=root, start=start, n=n)


# -- 6. sharing -----------------------------------------------------------------------------------------
def test_beside_a_sweep_job_and_a_search(gpu_engine):
    best = gpu_engine.submit_best(ROOT_A, START, N, device_mask=1)
    sweep = gpu_engine.submit_sweep(ROOT_A, RECEIVE, START, N, device_mask=1)
    search = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
    res, info = finish(best)
    log_records("sharing", info)
    check(res, 0, N)
    sw = sweep.wait(60)
    assert sw is not None and sw.status == _lib.NPOW_OK
    assert sw.hits == oracle.sweep(ROOT_A, RECEIVE, START, N) and sw.nonces_done == N
    s = search.wait(60)
    assert s is not None and s.status == _lib.NPOW_OK
    assert oracle.work_value_hashlib(ROOT_A, s.nonce) == s.value >= RECEIVE


# -- 7. cancel ------------------------------------------------------------------------------------------
def test_cancel_returns_the_best_so_far(gpu_engine):
    count = 1 << 36
    t = gpu_engine.submit_best(ROOT_A, START, count, device_mask=1)
    assert t.wait(0) is None  # NPOW_PENDING: the ticket stays valid
    deadline = time.time() + 1.0
    while t.info().nonces_done == 0 and time.time() < deadline:
        time.sleep(0.001)
    t.cancel()
    r = t.wait(30)
    assert r is not None and r.status == _lib.NPOW_CANCELLED
    assert r.nonces_done < count
    if r.nonce is not None:
        assert oracle.work_value_hashlib(ROOT_A, r.nonce) == r.value
        assert (r.nonce - START) & M64 < count
    # the device still serves
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1).wait(60)
    assert s.status == _lib.NPOW_OK and oracle.work_value_hashlib(ROOT_A, s.nonce) == s.value >= RECEIVE


# -- 8. device counter ----------------------------------------------------------------------------------
def test_lone_job_counts_its_range(gpu_engine):
    gpu_engine.reset_stats(0)
    r = gpu_engine.submit_best(ROOT_A, START, 1 << 24, device_mask=1).wait(60)
    assert r.status == _lib.NPOW_OK and r.nonces_done == 1 << 24
    assert oracle.work_value_hashlib(ROOT_A, r.nonce) == r.value
    assert gpu_engine.stats(0).nonces == 1 << 24


def test_empty_range_is_exhausted_at_once(gpu_engine):
    gpu_engine.reset_stats(0)
    r = gpu_engine.submit_best(ROOT_A, 12345, 0, device_mask=1).wait(0)
    assert r is not None and tuple(r) == (_lib.NPOW_EXHAUSTED, None, None, 0)
    assert gpu_engine.stats(0).nonces == 0 and gpu_engine.stats(0).launches == 0


# -- wrong calls ------------------------------------------------------------------------------------------
def test_ticket_kinds_refuse_each_other(gpu_engine):
    lib = gpu_engine.lib
    bad = _lib.NPOW_ERR_BAD_ARGUMENT
    n = 65537
    t = gpu_engine.submit_best(ROOT_A, START, n, device_mask=1)
    u32, u64 = ctypes.c_uint32(0), ctypes.c_uint64(0)
    info = _lib.SearchInfo()
    info.size = ctypes.sizeof(info)
    rinfo = _lib.ReserveInfo()
    rinfo.size = ctypes.sizeof(rinfo)
    sinfo = _lib._SweepInfoStruct()
    sinfo.size = ctypes.sizeof(sinfo)
    binfo = _lib._BestInfoStruct()
    binfo.size = ctypes.sizeof(binfo)
    assert lib.npow_wait(t.ticket, 0, ctypes.byref(u64), ctypes.byref(u64), ctypes.byref(u64)) == bad
    assert lib.npow_wait_info(t.ticket, 0, ctypes.byref(info)) == bad
    assert lib.npow_wait_result(t.ticket, 0, ctypes.byref(u64), ctypes.byref(u64)) == bad
    assert lib.npow_wait_sweep(t.ticket, 0, None, 0, ctypes.byref(u64), None) == bad
    assert lib.npow_ticket_sweep(t.ticket, ctypes.byref(sinfo)) == bad
    assert lib.npow_promote(t.ticket, 2) == bad
    assert lib.npow_retarget(t.ticket, M64) == bad
    assert lib.npow_relax(t.ticket, 0xfffff00000000000, ctypes.byref(u32)) == bad
    assert lib.npow_ticket_reserve(t.ticket, ctypes.byref(rinfo)) == bad
    assert lib.npow_ticket_background(t.ticket, ctypes.byref(u32)) == bad
    assert lib.npow_last_error()
    collected = t.ticket
    check(t.wait(60), 0, n)  # still collectable, and exact
    # npow_wait_best and npow_ticket_best on a search's and on a sweep job's ticket
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
    w = gpu_engine.submit_sweep(ROOT_A, RECEIVE, START, n, device_mask=1)
    for other in (s, w):
        assert lib.npow_wait_best(other.ticket, 0, ctypes.byref(u64), ctypes.byref(u64), None) == bad
        assert lib.npow_ticket_best(other.ticket, ctypes.byref(binfo)) == bad
    assert lib.npow_wait_best(collected, 0, ctypes.byref(u64), ctypes.byref(u64), None) == bad  # released
    res = s.wait(60)
    assert res.status == _lib.NPOW_OK and oracle.work_value_hashlib(ROOT_A, res.nonce) == res.value >= RECEIVE
    assert w.wait(60).status == _lib.NPOW_OK


# -- 9. CU partitions -------------------------------------------------------------------------------------
def test_split_over_two_cu_partitions():
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2", NANOPOW_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "best_job_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["ok"] and out["devices"] == 2
    checks, failures = out["affinity"]  # the test hooks' device-affinity check of every HIP call site
    assert checks > 0 and failures == 0, out["affinity"]
    assert out["nonces_per_device"] == [1 << 22, 1 << 22]
    assert out["second_half"]["winner_in_second_part"]
