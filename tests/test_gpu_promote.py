"""Promotion of a live search (npow_promote): the weight of a job that is waiting, admitted or inside a running
launch is raised, and a running counted launch rebalances its workgroups to the new weight without ending -- no
yield, no new launch.  Every test but the last runs on device 0 only.  Run on an MI355X: ``pytest -m gpu``.

The share tests are tests/test_gpu_weights.py's dynamic-join test with the weight raised after the start instead
of given at the submit: 20 ms at equal shares, then 100 ms in which the promoted job C holds 8/10 of the device
beside A and B, nominally C / (A + B) = (20/3 + 80) / (2 (20/3 + 10)) = 2.6; with equal shares throughout C could
not even pass one of them, so the bound is C > A + B.
"""
import hashlib
import json
import math
import os
import random
import subprocess
import sys
import time

import pytest

from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE = 0xfffffe0000000000


def _roots(seed, n):
    rng = random.Random(seed)
    return [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(n)]


def _value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


def _promoted_in_a_running_launch(eng, seed, dynamic):
    """A and B (and C, unless `dynamic`) are admitted together behind a blocker under max_active 1, so they share
    one counted launch that outlasts the test; with `dynamic`, C joins that launch as a dynamic entry of weight 1.
    C is promoted to 8 20 ms after the blocker is gone, and all three are cancelled 100 ms later."""
    eng.set_pool_tuning(budget_us=400000)  # one launch lasts past the test: ...
    eng.set_tuning(65536)                  # ... 32,768 wave iterations, ~0.4 s
    eng.pool_config(1)
    try:
        rx, ra, rb, rc = _roots(seed, 4)
        toks = [_lib.CancelToken() for _ in range(4)]
        tx = eng.submit(rx, M64, device_mask=1, cancel=toks[3])
        ta = eng.submit(ra, M64, start=1 << 52, device_mask=1, cancel=toks[0], weight=1)
        tb = eng.submit(rb, M64, start=2 << 52, device_mask=1, cancel=toks[1], weight=1)
        tc = None
        if not dynamic:
            tc = eng.submit(rc, M64, start=3 << 52, device_mask=1, cancel=toks[2], weight=1)
        assert eng.pool_status() == ((2 if dynamic else 3), 1)
        eng.pool_config(64)  # admitted, and adopted, together
        toks[3].set()
        assert tx.wait(30).status == _lib.NPOW_CANCELLED
        t0 = time.monotonic()
        dyn0 = eng.stats(0).dyn_entries
        if dynamic:
            time.sleep(0.005)  # (A and B's launch is running)
            tc = eng.submit(rc, M64, start=3 << 52, device_mask=1, cancel=toks[2], weight=1)
        time.sleep(max(0.0, t0 + 0.02 - time.monotonic()))
        s0 = eng.stats(0)
        tc.promote(8)
        time.sleep(max(0.0, t0 + 0.12 - time.monotonic()))
        s1 = eng.stats(0)
        for c in toks:
            c.set()
        da, db, dc = (t.wait(30).nonces_done for t in (ta, tb, tc))
    finally:
        eng.pool_config(64)
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)
    ratio = dc / max(da + db, 1)
    print(f"{'dynamic' if dynamic else 'table'} entry promoted: A {da} B {db} C {dc}, C / (A + B) = {ratio:.3f}; "
          f"promotions {s0.promotions} -> {s1.promotions}, yields {s0.yields} -> {s1.yields}, launches "
          f"{s0.launches} -> {s1.launches}, dyn_entries {dyn0} -> {s0.dyn_entries}")
    if dynamic:
        assert s0.dyn_entries > dyn0, "C did not join the running launch"
    assert s1.promotions >= s0.promotions + 1, "the promotion was not published into the running launch"
    assert (s1.yields, s1.launches) == (s0.yields, s0.launches), "the launch was ended for the promotion"
    assert dc > da + db, f"C / (A + B) = {ratio:.3f} (A {da}, B {db}, C {dc})"


def test_table_entry_promoted_in_a_running_launch(gpu_engine):
    _promoted_in_a_running_launch(gpu_engine, 81, dynamic=False)


def test_dynamic_entry_promoted_in_a_running_launch(gpu_engine):
    _promoted_in_a_running_launch(gpu_engine, 82, dynamic=True)


def test_waiting_job_promoted_is_admitted_first(gpu_engine):
    """max_active 1: behind a running job wait L1 and then L2, both weight 1; L2 is promoted to 8 and so adopted
    first when the running one ends."""
    eng = gpu_engine
    eng.pool_config(1)
    try:
        r0, r1, r2 = _roots(83, 3)
        tok = _lib.CancelToken()
        first = eng.submit(r0, M64, device_mask=1, cancel=tok)
        s1 = time.monotonic()
        l1 = eng.submit(r1, RECEIVE, device_mask=1, weight=1)
        s2 = time.monotonic()
        l2 = eng.submit(r2, RECEIVE, device_mask=1, weight=1)
        assert eng.pool_status() == (2, 1)
        l2.promote(8)
        assert eng.pool_status() == (2, 1)
        tok.set()
        assert first.wait(30).status == _lib.NPOW_CANCELLED
        i2, i1 = l2.wait_info(30), l1.wait_info(30)
    finally:
        eng.pool_config(64)
    assert i2.status == _lib.NPOW_OK and i1.status == _lib.NPOW_OK
    a2, a1 = s2 + i2.adopt_us * 1e-6, s1 + i1.adopt_us * 1e-6
    assert a2 < a1, f"the promoted job was adopted {(a2 - a1) * 1e3:.3f} ms after the lighter one"


def test_results_stay_right(gpu_engine):
    """24 searches at receive difficulty, every third promoted (to 2, 4 or 8) right after its submit and again 1 ms
    later, every fourth cancelled: each result validates under hashlib against its own root, and the pool's
    protocol checks stay at 0."""
    eng = gpu_engine
    eng.reset_stats(0)
    roots = _roots(84, 24)
    tickets, toks = [], []
    for i, r in enumerate(roots):
        c = _lib.CancelToken()
        t = eng.submit(r, RECEIVE, start=i << 48, device_mask=1, cancel=c, weight=1)
        if i % 3 == 0:
            t.promote((2, 4, 8)[(i // 3) % 3])
        tickets.append(t)
        toks.append(c)
    time.sleep(0.001)
    for i, t in enumerate(tickets):
        if i % 3 == 0:
            t.promote((2, 4, 8)[(i // 3) % 3])  # (idempotent; a search decided meanwhile takes it too)
            t.promote(8)
        if i % 4 == 0:
            toks[i].set()
    n_ok = 0
    for i, (r, t) in enumerate(zip(roots, tickets)):
        res = t.wait(60)
        assert res is not None
        assert res.status in ((_lib.NPOW_OK, _lib.NPOW_CANCELLED) if i % 4 == 0 else (_lib.NPOW_OK,))
        if res.status == _lib.NPOW_OK:
            n_ok += 1
            assert _value(r, res.nonce) == res.value >= RECEIVE
    assert n_ok >= 18
    st = eng.stats(0)
    assert st.early_mismatches == 0 and st.stale_missing == 0, (st.early_mismatches, st.stale_missing)


def test_arguments(gpu_engine):
    eng = gpu_engine
    tok = _lib.CancelToken()
    t = eng.submit(_roots(85, 1)[0], M64, device_mask=1, cancel=tok)
    try:
        for w in (0, 3, 16):
            with pytest.raises(_lib.NanoPowError) as e:
                t.promote(w)
            assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
            assert eng.lib.npow_promote(t.ticket, w) == _lib.NPOW_ERR_BAD_ARGUMENT
        assert eng.lib.npow_promote(0x7fffffff12345, 8) == _lib.NPOW_ERR_BAD_ARGUMENT  # no such ticket
        assert b"ticket" in eng.lib.npow_last_error()
        t.promote(1)  # at the current weight: fine
    finally:
        tok.set()
        assert t.wait(30).status == _lib.NPOW_CANCELLED
    assert eng.lib.npow_promote(t.ticket, 8) == _lib.NPOW_ERR_BAD_ARGUMENT  # collected
    with pytest.raises(_lib.NanoPowError) as e:
        t.promote(8)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


def test_bounded_job_takes_no_weight(gpu_engine):
    eng = gpu_engine
    tok = _lib.CancelToken()
    t = eng.submit(_roots(86, 1)[0], M64, device_mask=1, max_nonces_per_device=1 << 36, cancel=tok)
    try:
        for w in (2, 8):
            with pytest.raises(_lib.NanoPowError) as e:
                t.promote(w)
            assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
        t.promote(1)
    finally:
        tok.set()
        assert t.wait(30).status in (_lib.NPOW_CANCELLED, _lib.NPOW_EXHAUSTED)


def test_lower_weight_changes_nothing(gpu_engine):
    """Two endless jobs at weights (4, 4), one of them "promoted" to 2 after 20 ms: NPOW_OK, and after 200 ms their
    nonce counts are still within sqrt(2) of each other (weight 2 beside 4 would halve its share)."""
    eng = gpu_engine
    ra, rb = _roots(87, 2)
    toks = [_lib.CancelToken(), _lib.CancelToken()]
    ta = eng.submit(ra, M64, start=1 << 52, device_mask=1, cancel=toks[0], weight=4)
    tb = eng.submit(rb, M64, start=2 << 52, device_mask=1, cancel=toks[1], weight=4)
    time.sleep(0.02)
    p0 = eng.stats(0).promotions
    tb.promote(2)
    tb.promote(4)
    time.sleep(0.18)
    p1 = eng.stats(0).promotions
    for c in toks:
        c.set()
    da, db = (t.wait(30).nonces_done for t in (ta, tb))
    r = db / max(da, 1)
    print(f"weights (4, 4), one promoted to 2: nonces {da} / {db}, ratio {r:.3f}")
    assert p1 == p0
    assert 1 / math.sqrt(2) < r < math.sqrt(2), f"ratio {r:.3f} ({da} / {db} nonces)"


def test_decided_but_uncollected_ticket(gpu_engine):
    eng = gpu_engine
    r, = _roots(88, 1)
    t = eng.submit(r, RECEIVE, device_mask=1)
    res = t.wait_result(30)
    assert res is not None and res.status == _lib.NPOW_OK
    t.promote(8)  # NPOW_OK: nothing to raise any more
    assert eng.lib.npow_promote(t.ticket, 8) == _lib.NPOW_OK
    full = t.wait(30)
    assert full.status == _lib.NPOW_OK and _value(r, full.nonce) == full.value >= RECEIVE


def test_two_cu_partitions():
    """The table-entry test on a job split over two CU partitions (a child process: the engine reads
    NANOPOW_VIRTUAL_DEVICES once): each device publishes the promotion into its own running launch."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2")
    p = subprocess.run([sys.executable, os.path.join(here, "promote_partition_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    da, db, dc = out["nonces"]
    print(f"two partitions: A {da} B {db} C {dc}, C / (A + B) = {dc / max(da + db, 1):.3f}, stats {out['devices']}")
    for d in out["devices"]:
        assert d["promotions_after"] >= d["promotions_before"] + 1, out["devices"]
        assert (d["yields_after"], d["launches_after"]) == (d["yields_before"], d["launches_before"]), out["devices"]
        assert d["early_mismatches"] == 0 and d["stale_missing"] == 0, out["devices"]
    assert dc > da + db, out["nonces"]
