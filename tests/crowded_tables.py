"""Crowded pool tables: the scenarios of tests/test_gpu_crowded_tables.py, shared with its CU-partition child
(tests/crowded_tables_worker.py).  Each takes an engine, runs on device 0 and raises AssertionError on a mismatch.

How a table is crowded.  A blocking npow_sweep from a thread takes the device from the pool (TaskLock): while it runs
the pool's worker launches nothing, so every job submitted meanwhile is admitted and waits, and when the sweep ends the
worker's next table holds all of them.  The holder is seen to hold the device when the device's launch counter has
moved (its first launch has retired; the pool is idle, so nothing else can move it) -- no sleep guesses at it.  The
holder runs to its end, so the launches it adds to the counter are a fixed number, measured once on the idle device
(holder_launches).

How a test proves that its table was crowded -- a test that passes because the jobs ran one after another would be
worthless:
* a best job among the collecting entries: BestInfo.room is the smallest region of the launch's hit records it was
  given, and room == NPOW_SWEEP_JOB_HITS >> s only in a launch with more than 2^(s-1) collecting entries;
* the pigeonhole, for tables of bounded searches: each range fits its entry's own share of a launch at n = 64, so each
  job takes part in exactly one launch; if P pool launches retired between the idle device before and the idle device
  after, one of them held at least n / P jobs, and n > 16 P makes that more than 16 (the table then lies in device
  memory, not in the kernel arguments).  P counts every launch of the device in that time less the holder's own: more
  than held the jobs, never fewer.
"""
import contextlib
import json
import os
import random
import threading
import time

import numpy as np

import oracle
from nanopow import _lib

M64 = (1 << 64) - 1
CAP = _lib.NPOW_SWEEP_JOB_HITS
QUARTER = 0xc000000000000000  # a quarter of the lanes
RECEIVE = 0xfffffe0000000000
COUNTS = [1, 63, 64, 65, 511, 513, 4097, 65537]
HOLD_ROOT = bytes(range(101, 133))
HOLD_FIRST = 1 << 31  # what one launch of npow_sweep covers: the holder's first launch, whose end shows that it holds
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def until(cond, timeout=30.0, nap=0.0005):
    deadline = time.time() + timeout
    while not cond():
        assert time.time() < deadline, "timed out"
        time.sleep(nap)


def idle_launches(eng):
    """The device's launch counter with the pool idle (npow_device_stats waits for the worker to retire its launches)."""
    until(lambda: eng.pool_status() == (0, 0))
    return eng.stats(0).launches


def _hold(eng):
    # ... and its second launch is the time to submit in: some 30 ms on a whole MI355X, 130 ms on 32 CUs
    count = HOLD_FIRST + (1 << 30 if eng.stats(0).grid >= 512 else 1 << 29)
    hits = eng.sweep(HOLD_ROOT, M64, 0, count, device_mask=1, cap=1)
    assert hits == [] or oracle.work_value_hashlib(HOLD_ROOT, hits[0]) == M64


_holder_launches = {}


def holder_launches(eng):
    """The launches one holder adds to the device's counter, measured on the idle device (once per engine)."""
    if id(eng) not in _holder_launches:
        before = idle_launches(eng)
        _hold(eng)
        _holder_launches[id(eng)] = idle_launches(eng) - before
        assert _holder_launches[id(eng)] >= 2, _holder_launches
    return _holder_launches[id(eng)]


class Held:
    launches_before = 0  # the idle device's launch counter before the holder
    own = 0              # the launches the holder adds to it


@contextlib.contextmanager
def held_device(eng):
    """Submit in the block: the jobs enter the worker's next table together.  Collect after it."""
    own = holder_launches(eng)
    h = Held()
    h.own = own
    h.launches_before = idle_launches(eng)
    th = threading.Thread(target=_hold, args=(eng,))
    th.start()
    try:
        until(lambda: eng.stats(0).launches > h.launches_before)  # the holder has the device
        yield h
    finally:
        th.join()


def pool_launches(eng, h):
    """P of the pigeonhole: call once every job of the block has been collected."""
    return idle_launches(eng) - h.launches_before - h.own


def shift_of(n):
    s = 0
    while (1 << s) < n:
        s += 1
    return s


def roots(seed, n):
    rng = random.Random(seed)
    out = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(n)]
    assert len(set(out)) == n
    return out, rng


def ragged_ranges(rng, n, top=1 << 17):
    """n (start, count): odd starts, counts from COUNTS and ragged ones up to `top`; range 0 crosses 2^32, range 1
    crosses 2^64."""
    out = []
    for i in range(n):
        count = COUNTS[i % len(COUNTS)] if i % 3 else rng.randrange(1, top + 1)
        if i < 2:
            count = max(count, 4097)
        start = rng.getrandbits(64) | 1
        if i == 0:
            start = ((1 << 32) - count // 2) | 1
        elif i == 1:
            start = ((1 << 64) - count // 2) | 1
        out.append((start & M64, count))
    assert out[0][0] < 1 << 32 < out[0][0] + out[0][1] and out[1][0] + out[1][1] > 1 << 64
    return out


def sweep_ref(root, thr, start, count):
    return oracle.sweep(root, thr, start, count, threads=min(16, os.cpu_count() or 1), cap=count)


def best_ref(root, start, count):
    v = oracle.work_values_range(root, start, count)
    k = int(np.argmax(v))  # first occurrence
    return (start + k) & M64, int(v[k])


def finished(t, timeout=60.0):
    until(lambda: t.info().finished, timeout)
    return t.info()


def check_best(t, root, start, count, room=None):
    info = finished(t)
    res = t.wait(5)
    nonce, value = best_ref(root, start, count)
    assert res is not None and res.status == _lib.NPOW_OK, res
    assert (res.nonce, res.value, res.nonces_done) == (nonce, value, count), (res, hex(nonce), hex(value), count)
    assert oracle.work_value_hashlib(root, res.nonce) == res.value
    assert info.records_max <= info.room, info
    if room is not None:
        assert info.room == room, (info, room)  # the proof: a launch with that many collecting entries held it
    return info


def check_sweep(t, root, thr, start, count):
    r = t.wait(60)
    want = list(range(start, start + count)) if thr == 0 and start + count <= M64 else sweep_ref(root, thr, start, count)
    assert r is not None and r.status == _lib.NPOW_OK, (r and r.status, count)
    assert r.hits == want, (len(r.hits), len(want), hex(start), count)
    assert r.total == len(want) and r.nonces_done == count, (r.total, r.nonces_done, count)


# -- a. sweep jobs ------------------------------------------------------------------------------------------------
def sweep_table(eng, n, thr, seed):
    """n collecting entries: n - 1 sweep jobs of distinct roots and one best job, the witness.  Everything exact."""
    rs, rng = roots(seed, n)
    rg = ragged_ranges(rng, n)
    w = n // 2  # the witness's place in the table
    with held_device(eng):
        ts = [eng.submit_best(rs[i], rg[i][0], rg[i][1], device_mask=1) if i == w else
              eng.submit_sweep(rs[i], thr, rg[i][0], rg[i][1], device_mask=1, cap=rg[i][1]) for i in range(n)]
    info = check_best(ts[w], rs[w], *rg[w], room=CAP >> shift_of(n))
    for i in range(n):
        if i != w:
            check_sweep(ts[i], rs[i], thr, *rg[i])
    return {"n": n, "threshold": f"{thr:016x}", "room": info.room, "nonces": sum(c for _, c in rg)}


# -- b. best jobs ---------------------------------------------------------------------------------------------------
def edge_cut(root, rng, last, W=1 << 16):
    """A range of `root` whose maximum is its first nonce -- or, `last`, its last one, in a ragged tail; odd start."""
    for _ in range(64):
        s = rng.getrandbits(64) | 1
        v = oracle.work_values_range(root, s, W)
        m = int(np.argmax(v))
        if last and (m + 1) % 64 and m + 1 >= 65:
            return s, m + 1
        if not last and m % 2 == 0 and W - m >= 65:
            return (s + m) & M64, W - m
    raise AssertionError("no window with its maximum there")


def best_table(eng, seed, n=64):
    rs, rng = roots(seed, n)
    rg = ragged_ranges(rng, n)
    first, last = [8, 9, 10, 11], [12, 13, 14, 15]
    for i in first + last:
        rg[i] = edge_cut(rs[i], rng, i in last)
    with held_device(eng):
        ts = [eng.submit_best(rs[i], rg[i][0], rg[i][1], device_mask=1) for i in range(n)]
    infos = [check_best(ts[i], rs[i], *rg[i], room=CAP >> shift_of(n)) for i in range(n)]
    for i in first:
        assert ts[i].result.nonce == rg[i][0]
    for i in last:
        assert ts[i].result.nonce == (rg[i][0] + rg[i][1] - 1) & M64 and rg[i][1] % 64
    return {"n": n, "records_max": max(i.records_max for i in infos), "room": infos[0].room,
            "records": sum(i.records for i in infos)}


# -- c. bounded first-win searches ----------------------------------------------------------------------------------
PLACES = ["first nonce", "last nonce", "first lane of a block", "last lane of a block"]


def place_cut(root, rng, place, count, W=1 << 15):
    """(start, count, nonce, value): a range of `root`, odd start, whose one maximum lies at `place`."""
    for _ in range(200):
        s = rng.getrandbits(64)
        v = oracle.work_values_range(root, s, W)
        m = int(np.argmax(v))
        if int((v == v[m]).sum()) != 1:
            continue
        if place == "first nonce":
            off, cnt = 0, min(count, W - m)
        elif place == "last nonce":
            cnt = min(count, m + 1)
            off = cnt - 1
        else:
            blocks = min(count, W) // 64
            j = min(max(1, blocks // 2), m // 64)
            off = 64 * j + (63 if place.startswith("last") else 0)
            cnt = min(count, W - (m - off))
            if j < 1 or off > m or cnt < off + 65:  # a block in the middle: one before it, one after it
                continue
        start = (s + m - off) & M64
        if start & 1 and cnt >= 1:
            return start, cnt, (s + m) & M64, int(v[m])
    raise AssertionError("no window with its maximum there")


def search_table(eng, n, seed):
    """n bounded first-win searches: three quarters of them at the maximum of their range, which lies at a chosen
    place, a quarter one above it.  Crowded by the pigeonhole."""
    rs, rng = roots(seed, n)
    n_none = n // 4
    none = ragged_ranges(rng, n_none)
    jobs = []  # (root, threshold, start, count, nonce, value); nonce None: one above the maximum, no winner
    winners = 0
    for i in range(n):
        if i % 4 == 3:  # n // 4 of them
            start, count = none[i // 4]
            top = int(oracle.work_values_range(rs[i], start, count).max())
            assert top < M64
            jobs.append((rs[i], top + 1, start, count, None, None))
            continue
        place = PLACES[winners % 4]
        count = COUNTS[(winners // 4) % 8] if place.endswith("nonce") else [511, 513, 4097, 65537][(winners // 4) % 4]
        winners += 1
        start, count, nonce, value = place_cut(rs[i], rng, place, count)
        jobs.append((rs[i], value, start, count, nonce, value))
    grid = eng.stats(0).grid
    iters = 4096  # the launch's wave iterations at the default tuning (npow_set_tuning 8192)
    assert all(j[3] <= (grid // 64) * 8 * iters * 64 for j in jobs)  # each range fits own(e, 64, iters): one launch
    with held_device(eng) as h:
        ts = [eng.submit(r, thr, start=start, device_mask=1, max_nonces_per_device=count)
              for r, thr, start, count, _, _ in jobs]
    for t, (r, thr, start, count, nonce, value) in zip(ts, jobs):
        res = t.wait(60)
        assert res is not None, "pending"
        if nonce is None:
            assert res.status == _lib.NPOW_EXHAUSTED and res.nonces_done == count, (res, count)
        else:
            assert res.status == _lib.NPOW_OK, (res, hex(start), count)
            assert (res.nonce, res.value) == (nonce, value), (res, hex(nonce), hex(value), hex(start), count)
            assert oracle.work_value_hashlib(r, res.nonce) == res.value >= thr
    p = pool_launches(eng, h)
    assert p >= 1 and n > 16 * p, f"{n} jobs over {p} pool launches: no launch is shown to have held more than 16"
    return {"n": n, "pool_launches": p, "winners": sum(1 for j in jobs if j[4] is not None),
            "exhausted": sum(1 for j in jobs if j[4] is None), "grid": grid, "rem": grid % n}


# -- d. stitching ---------------------------------------------------------------------------------------------------
def stitch_table(eng, n, seed, count=65537):
    """One wave iteration per launch: n sweep jobs of `count` nonces and unequal thresholds, several launches each."""
    rs, rng = roots(seed, n)
    rg = [(s, count) for s, _ in ragged_ranges(rng, n)]
    thrs = [(0xc0 + (i * 7) % 0x3f) << 56 for i in range(n)]  # c0.. to fe..: a quarter of the lanes down to 1 in 128
    w = n // 2
    eng.set_tuning(2, 0, 0)
    try:
        with held_device(eng):
            ts = [eng.submit_best(rs[i], *rg[i], device_mask=1) if i == w else
                  eng.submit_sweep(rs[i], thrs[i], *rg[i], device_mask=1, cap=count) for i in range(n)]
        launches = max(finished(t).launches for t in ts)
        info = check_best(ts[w], rs[w], *rg[w], room=CAP >> shift_of(n))
        for i in range(n):
            if i != w:
                check_sweep(ts[i], rs[i], thrs[i], *rg[i])
    finally:
        eng.set_tuning(8192, 0, 0)
    assert launches >= 3, launches
    return {"n": n, "launches": launches, "room": info.room}


def log_records(name, **kw):
    out = os.path.join(ROOT_DIR, "bench_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "best_records.jsonl"), "a") as f:
        f.write(json.dumps({"test": name, **kw}) + "\n")
