"""Reserve hits (npow_submit_reserve, npow_ticket_reserve, npow_relax): a search submitted with a reserve threshold
R <= threshold remembers the best nonce it passes whose value is in [R, threshold), the host can look at it
(Ticket.reserve) and lower the search's threshold to any level down to R (Ticket.relax) -- decided at once from the
reserve when that qualifies, lowered inside the running launch otherwise.  Nothing ends or restarts in either case.
Every test but the child process runs on device 0 only.  Run on an MI355X: ``pytest -m gpu``.

The solo tests search the root of tests/golden/sweep_2p36_hashlib.json, every nonce of which in [0, 2^36) with a value
at or above OLD = fffffff800000000 is known (126 hits, found with hashlib): from S = 0x846e097c0 the next eight hits are
all below NEW = fffffffe00000000, the first of them 2^31.19 nonces (~55-70 ms of a whole GPU) from S, and the first
hit at or above NEW is 0xa312db930, 2^32.94 nonces from S.  No test waits a guessed time for the GPU to have passed a
nonce: each polls Ticket.reserve() against a 10 s deadline.
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
import time

import pytest

from conftest import load_golden
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE = 0xfffffe0000000000
OLD, NEW = 0xfffffff800000000, 0xfffffffe00000000
RMIN = 0xfffff00000000000
S = 0x846e097c0
HERE = os.path.dirname(os.path.abspath(__file__))


def _roots(seed, n):
    rng = random.Random(seed)
    return [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(n)]


def _value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


@pytest.fixture(scope="module")
def fixture_hits():
    """(root, {nonce: hashlib value}) of the 2^36 sweep fixture."""
    g = load_golden("sweep_2p36_hashlib.json")
    root = bytes.fromhex(g["root"])
    assert int(g["threshold"], 16) == OLD and int(g["start"], 16) == 0 and g["count"] == 1 << 36
    hits = {int(h, 16): _value(root, int(h, 16)) for h in g["hits"]}
    assert len(hits) == 126 and all(v >= OLD for v in hits.values())
    after = sorted(n for n in hits if n >= S)
    assert all(hits[n] < NEW for n in after[:8]) and after[8] == 0xa312db930 and hits[after[8]] == 0xfffffffe03ad1051
    return root, hits


def _idle_stats(eng, device=0):
    """The device's counters once the launches of earlier searches have retired (two equal reads 1 ms apart)."""
    prev = eng.stats(device)
    for _ in range(2000):
        time.sleep(0.001)
        st = eng.stats(device)
        if (st.launches, st.yields) == (prev.launches, prev.yields):
            return st
        prev = st
    raise AssertionError("the device's launches never settled")


def _poll_reserve(t, cond=lambda r: True, seen=None):
    """Ticket.reserve() until it holds a nonce that meets cond (10 s deadline); seen collects every value read."""
    deadline = time.monotonic() + 10
    while time.monotonic() < deadline:
        r = t.reserve()
        if r is not None:
            if seen is not None:
                seen.append(r.value)
            if cond(r):
                return r
        time.sleep(0.0005)
    raise AssertionError("no reserve within 10 s")


class _Solo:
    """The solo set-up: one launch covers [S, S + 2^34) densely and outlasts the search."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.set_pool_tuning(budget_us=600000)
        self.eng.set_tuning(65536)
        return self

    def __exit__(self, *exc):
        self.eng.set_pool_tuning(budget_us=20000)
        self.eng.set_tuning(8192)


def _end(t, timeout=30):
    """Cancel and collect a ticket a failed assertion may have left running."""
    if t is not None and t.result is None:
        t.cancel()
        t.wait(timeout)


def test_answered_from_the_reserve(gpu_engine, fixture_hits):
    eng = gpu_engine
    root, hits = fixture_hits
    t = None
    with _Solo(eng):
        try:
            t = eng.submit(root, M64, start=S, device_mask=1, reserve=OLD)
            r = _poll_reserve(t)
            assert r.nonce in hits and S <= r.nonce < S + (1 << 36), f"{r.nonce:x} is no fixture hit"
            assert r.value == hits[r.nonce]
            before = t.reserve_info()
            assert before.armed == 1 and before.reserve_threshold == OLD and before.threshold == M64
            assert before.answered == 0 and before.relaxes == 0 and before.device == 0 and before.candidates >= 1
            assert t.relax(OLD) is True
            res = t.wait_result(0)  # zero timeout: the result is there before relax returned
            assert res is not None and res.status == _lib.NPOW_OK
            assert res.nonce in hits and res.value == hits[res.nonce] >= OLD
            ri = t.reserve_info()
            info = t.wait_info(30)
        finally:
            _end(t)
    print(f"answered: reserve {r.nonce:x} {r.value:016x}, result {res.nonce:x} {res.value:016x}, candidates "
          f"{ri.candidates}, nonces_done {info.nonces_done}")
    assert info.status == _lib.NPOW_OK and (info.nonce, info.value) == (res.nonce, res.value)
    assert ri.answered == 1 and ri.relaxes == 1 and ri.threshold == OLD and ri.value == res.value
    assert info.nonces_done > 0
    assert eng.stats(0).stale_missing == 0


def test_the_reserve_gets_better(gpu_engine, fixture_hits):
    eng = gpu_engine
    root, hits = fixture_hits
    t, seen = None, []
    with _Solo(eng):
        try:
            t = eng.submit(root, M64, start=S, device_mask=1, reserve=OLD)
            r = _poll_reserve(t, lambda r: r.value >= NEW, seen)
            assert t.relax(NEW) is True
            res = t.wait_result(0)
            info = t.wait_info(30)
        finally:
            _end(t)
    print(f"better: {len(set(seen))} distinct reserves, last {r.nonce:x} {r.value:016x}")
    assert seen == sorted(seen), "the reserve's value decreased between polls"
    assert all(v >= OLD for v in seen)
    assert res is not None and res.status == _lib.NPOW_OK and res.value >= NEW
    assert res.nonce in hits and res.value == hits[res.nonce]
    assert info.status == _lib.NPOW_OK


def test_lowered_in_place(gpu_engine, fixture_hits):
    """Relaxed 5 ms after the submit: the first fixture hit is ~55-70 ms of hashing away, so there is no reserve yet,
    the threshold drops inside the running launch, and that launch returns a fixture hit."""
    eng = gpu_engine
    root, hits = fixture_hits
    t = None
    with _Solo(eng):
        try:
            s0 = _idle_stats(eng)
            t = eng.submit(root, M64, start=S, device_mask=1, reserve=OLD)
            time.sleep(0.005)
            answered = t.relax(OLD)
            res = t.wait_result(30)
            ri = t.reserve_info()
            info = t.wait_info(30)
            s1 = _idle_stats(eng)
        finally:
            _end(t)
    print(f"in place: nonce {info.nonce:x} value {info.value:016x}, launches {s0.launches} -> {s1.launches}, yields "
          f"{s0.yields} -> {s1.yields}, candidates {ri.candidates}")
    assert answered is False
    assert res is not None and info.status == _lib.NPOW_OK
    assert info.nonce in hits and S <= info.nonce < S + (1 << 34), f"{info.nonce:x}"
    assert info.value == hits[info.nonce] >= OLD
    assert ri.answered == 0 and ri.relaxes == 1 and ri.threshold == OLD
    assert s1.launches == s0.launches + 1, "the search took another launch"
    assert s1.yields == s0.yields
    assert s1.stale_missing == 0


def test_lowered_to_a_level_between(gpu_engine, fixture_hits):
    eng = gpu_engine
    root, hits = fixture_hits
    t = None
    with _Solo(eng):
        try:
            t = eng.submit(root, M64, start=S, device_mask=1, reserve=OLD)
            time.sleep(0.005)
            answered = t.relax(NEW)
            res = t.wait_result(30)
            ri = t.reserve_info()
            info = t.wait_info(30)
        finally:
            _end(t)
    print(f"between: nonce {info.nonce:x} value {info.value:016x}, reserve {ri.nonce:x} {ri.value:016x}")
    assert answered is False and res is not None
    assert info.status == _lib.NPOW_OK and info.value >= NEW
    assert info.nonce in hits and info.value == hits[info.nonce]
    assert ri.value == 0 or (OLD <= ri.value < NEW and ri.value == hits[ri.nonce])  # below NEW, or none: both right
    assert ri.answered == 0 and ri.threshold == NEW


def test_both_ways(gpu_engine, fixture_hits):
    eng = gpu_engine
    root, hits = fixture_hits
    t = None
    with _Solo(eng):
        try:
            t = eng.submit(root, NEW, start=S, device_mask=1, reserve=OLD)
            answered = t.relax(OLD)
            held = t.retarget(NEW)
            res = t.wait_result(30)
            ri = t.reserve_info()
            info = t.wait_info(30)
        finally:
            _end(t)
    print(f"both ways: answered {answered} held {held} value {info.value:016x} retargets {info.retargets} stale_wins "
          f"{info.stale_wins}")
    assert res is not None and info.status == _lib.NPOW_OK
    assert info.value == _value(root, info.nonce)
    if answered:  # decided from a reserve at once: the raise came too late
        assert held is False and info.value >= OLD and ri.answered == 1
    else:
        assert held is True and info.value >= NEW and ri.answered == 0 and ri.threshold == NEW
        assert info.retargets == 1


def test_beside_other_searches(gpu_engine):
    """Two endless searches share one counted launch (admitted together behind a blocker, as in
    tests/test_gpu_retarget.py); a search with the lowest reserve threshold joins that launch as a dynamic entry, has
    a reserve within microseconds and is relaxed to it."""
    eng = gpu_engine
    rx, ra, rb, rc = _roots(191, 4)
    toks = [_lib.CancelToken() for _ in range(3)]
    tc = None
    eng.pool_config(1)
    try:
        tx = eng.submit(rx, M64, device_mask=1, cancel=toks[2])
        ta = eng.submit(ra, M64, start=1 << 52, device_mask=1, cancel=toks[0])
        tb = eng.submit(rb, M64, start=2 << 52, device_mask=1, cancel=toks[1])
        assert eng.pool_status() == (2, 1)
        eng.pool_config(64)  # admitted, and adopted, together
        toks[2].set()
        assert tx.wait(30).status == _lib.NPOW_CANCELLED
        time.sleep(0.005)  # (their launch is running)
        s0 = eng.stats(0)
        tc = eng.submit(rc, M64, start=3 << 52, device_mask=1, reserve=RMIN)
        r = _poll_reserve(tc)
        answered = tc.relax(RMIN)
        res = tc.wait_result(0)
        info = tc.wait_info(30)
        s1 = eng.stats(0)
        pending = (ta.wait(0), tb.wait(0))
    finally:
        eng.pool_config(64)
        for c in toks:
            c.set()
        _end(tc)
    ra_res, rb_res = ta.wait(30), tb.wait(30)
    print(f"beside two: reserve {r.nonce:x} {r.value:016x}, result {info.nonce:x} {info.value:016x}, dyn_entries "
          f"{s0.dyn_entries} -> {s1.dyn_entries}, yields {s0.yields} -> {s1.yields}")
    assert answered is True and res is not None and res.status == _lib.NPOW_OK
    assert info.status == _lib.NPOW_OK and _value(rc, info.nonce) == info.value >= RMIN
    assert _value(rc, r.nonce) == r.value >= RMIN
    assert s1.dyn_entries == s0.dyn_entries + 1, "the third search did not join the running launch"
    assert s1.yields == s0.yields, "a launch was ended"
    assert pending == (None, None), "a neighbour ended"
    assert ra_res.status == _lib.NPOW_CANCELLED and rb_res.status == _lib.NPOW_CANCELLED
    assert s1.stale_missing == 0


def test_results_stay_right(gpu_engine):
    """16 searches at fffffffe00000000 with the receive difficulty as their reserve, each relaxed after 2 ms to one of
    three levels: every result validates under hashlib at or above its relaxed threshold, and every reserve the
    host holds has hashlib's value.  (The 16 share one GPU: a whole GPU hashes 2^31 nonces, one expected win at
    fffffffe00000000, in ~60 ms.)"""
    eng = gpu_engine
    eng.reset_stats(0)
    inv0 = eng.stats(0).invalid_work
    rng = random.Random(192)
    roots = _roots(193, 16)
    levels = [rng.choice((RECEIVE, 0xffffff0000000000, OLD)) for _ in roots]
    tickets = []
    try:
        for i, r in enumerate(roots):
            tickets.append(eng.submit(r, NEW, start=i << 48, device_mask=1, reserve=RECEIVE))
        time.sleep(0.002)
        how = [t.relax(lv) for t, lv in zip(tickets, levels)]
        # (None: the search was decided at fffffffe00000000 within those 2 ms -- about one run in thirty has one --
        # and its result stands, above every level)
        n_res = 0
        for r, t, lv, h in zip(roots, tickets, levels, how):
            assert t.wait_result(60) is not None
            ri = t.reserve_info()
            info = t.wait_info(60)
            assert info is not None and info.status == _lib.NPOW_OK
            # (too late: never relaxed, so its result stands at the threshold of its submit)
            assert _value(r, info.nonce) == info.value >= (NEW if h is None else lv), (hex(info.value), hex(lv), h)
            if ri.value:
                n_res += 1
                assert _value(r, ri.nonce) == ri.value >= RECEIVE
            assert ri.threshold == (NEW if h is None else lv) and ri.reserve_threshold == RECEIVE and ri.armed == 1
    finally:
        for t in tickets:
            _end(t)
    st = eng.stats(0)
    print(f"16 searches: answered {how.count(True)}, lowered {how.count(False)}, too late {how.count(None)}, "
          f"{n_res} held a reserve")
    assert how.count(None) <= 2, how
    assert st.early_mismatches == 0 and st.stale_missing == 0, (st.early_mismatches, st.stale_missing)
    assert st.invalid_work == inv0 and st.dead == 0


def test_unarmed_searches_are_untouched(gpu_engine):
    eng = gpu_engine
    r0, r1 = _roots(194, 2)
    t = eng.submit(r0, RECEIVE, device_mask=1)
    t2 = eng.submit(r1, RECEIVE, device_mask=1, reserve=RECEIVE)  # reserve == threshold: the existing submit
    try:
        for tk in (t, t2):
            ri = tk.reserve_info()
            assert ri.armed == 0 and ri.value == 0 and ri.device == -1 and ri.reserve_threshold == RECEIVE
            assert tk.reserve() is None
            assert eng.lib.npow_relax(tk.ticket, RECEIVE, None) == _lib.NPOW_ERR_BAD_ARGUMENT
            with pytest.raises(_lib.NanoPowError) as e:
                tk.relax(RECEIVE)
            assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
        info, info2 = t.wait_info(30), t2.wait_info(30)
    finally:
        _end(t)
        _end(t2)
    assert info.status == _lib.NPOW_OK and _value(r0, info.nonce) == info.value >= RECEIVE
    assert info2.status == _lib.NPOW_OK and _value(r1, info2.nonce) == info2.value >= RECEIVE


def test_arguments(gpu_engine):
    eng = gpu_engine
    lib = eng.lib
    root, = _roots(195, 1)
    tk = ctypes.c_uint64(0)

    def submit_rc(threshold, reserve, weight=1, background=0):
        return lib.npow_submit_reserve(root, threshold, reserve, 0, 1, None, weight, background, ctypes.byref(tk))

    assert submit_rc(OLD, OLD + 1) == _lib.NPOW_ERR_BAD_ARGUMENT       # reserve > threshold
    assert submit_rc(OLD, RMIN - 1) == _lib.NPOW_ERR_BAD_ARGUMENT      # reserve < NPOW_RESERVE_MIN
    assert b"NPOW_RESERVE_MIN" in lib.npow_last_error()
    for w in (0, 3, 16):
        assert submit_rc(M64, OLD, weight=w) == _lib.NPOW_ERR_BAD_ARGUMENT  # a bad weight
    assert lib.npow_submit_reserve(root, M64, OLD, 0, 1, None, 1, 0, None) == _lib.NPOW_ERR_BAD_ARGUMENT

    info = _lib.ReserveInfo()
    info.size = ctypes.sizeof(info)
    ans = ctypes.c_uint32(9)
    assert lib.npow_ticket_reserve(0x7fffffff12345, ctypes.byref(info)) == _lib.NPOW_ERR_BAD_ARGUMENT
    assert lib.npow_relax(0x7fffffff12345, OLD, ctypes.byref(ans)) == _lib.NPOW_ERR_BAD_ARGUMENT  # no such ticket
    assert b"ticket" in lib.npow_last_error()

    tok = _lib.CancelToken()
    t = eng.submit(root, M64, device_mask=1, cancel=tok, reserve=OLD, weight=2)
    bg = eng.submit(_roots(196, 1)[0], M64, device_mask=1, reserve=OLD, background=True)
    try:
        assert lib.npow_ticket_reserve(t.ticket, None) == _lib.NPOW_ERR_BAD_ARGUMENT
        assert lib.npow_relax(t.ticket, OLD - 1, ctypes.byref(ans)) == _lib.NPOW_ERR_BAD_ARGUMENT  # below R
        assert t.relax(M64) is False                   # not below the current threshold: NPOW_OK, no effect
        assert t.reserve_info().relaxes == 0
        small = _lib.ReserveInfo()
        small.size = 8                                 # the library writes at most that many bytes
        small.reserve_threshold = 0x55
        assert lib.npow_ticket_reserve(t.ticket, ctypes.byref(small)) == _lib.NPOW_OK
        assert (small.size, small.armed, small.reserve_threshold) == (8, 1, 0x55)
        b = ctypes.c_uint32(0)
        assert lib.npow_ticket_background(bg.ticket, ctypes.byref(b)) == _lib.NPOW_OK and b.value == 1
        assert bg.reserve_info().armed == 1
        tok.set()
        bg.cancel()
        assert t.wait_result(30).status == _lib.NPOW_CANCELLED
        assert lib.npow_relax(t.ticket, OLD, ctypes.byref(ans)) == _lib.NPOW_TOO_LATE  # cancelled, uncollected
        assert t.relax(OLD) is None
        assert lib.npow_ticket_reserve(t.ticket, ctypes.byref(info)) == _lib.NPOW_OK and info.armed == 1
    finally:
        tok.set()
        _end(bg)
        t.wait(30)
    assert lib.npow_relax(t.ticket, OLD, None) == _lib.NPOW_ERR_BAD_ARGUMENT  # collected
    assert lib.npow_ticket_reserve(t.ticket, ctypes.byref(info)) == _lib.NPOW_ERR_BAD_ARGUMENT
    with pytest.raises(_lib.NanoPowError):
        t.relax(OLD)
    with pytest.raises(_lib.NanoPowError):
        eng.submit(root, OLD, device_mask=1, reserve=OLD + 1)


def test_decided_but_uncollected_ticket_is_too_late(gpu_engine):
    eng = gpu_engine
    r, = _roots(197, 1)
    t = eng.submit(r, 0xffffff0000000000, device_mask=1, reserve=RECEIVE)
    try:
        res = t.wait_result(30)
        assert res is not None and res.status == _lib.NPOW_OK
        assert t.relax(RECEIVE) is None
        info = t.wait_info(30)
    finally:
        _end(t)
    assert (info.status, info.nonce, info.value) == (_lib.NPOW_OK, res.nonce, res.value)
    assert _value(r, info.nonce) == info.value >= 0xffffff0000000000


def test_two_cu_partitions():
    """The first test's flow on a search split over two CU partitions: the reserve comes from either device, and after
    the answer both devices' final counts arrive."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "reserve_worker.py")],
                       env=dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2"), capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"partitions: {out}")
    assert out["reserve_hashlib"] == out["reserve_value"] >= OLD and out["reserve_device"] in (0, 1)
    assert out["answered"] is True and out["result_at_once"] is True
    assert out["status"] == _lib.NPOW_OK and out["n_devices"] == 2
    assert out["hashlib"] == out["value"] >= OLD
    assert out["info_answered"] == 1 and out["relaxes"] == 1
    assert out["nonces_done"] > 0
    for d in out["after"]:
        assert d["early_mismatches"] == 0 and d["stale_missing"] == 0 and d["dead"] == 0, out["after"]
