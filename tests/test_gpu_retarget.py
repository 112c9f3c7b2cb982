"""Retargeting a live search (npow_retarget): the threshold of a job that is waiting, admitted or inside a running
launch is raised in place.  The launch goes on -- no yield, no new launch -- the waves that meet a hit under the old
threshold read the slot's floor record, pass the hit over and count it (npow_search_info.stale_hits), and a win that
a wave published before it could see the record is refused by the host (stale_wins, the fallback, forced in the last
test).  Every test but the two child processes runs on device 0 only.  Run on an MI355X: ``pytest -m gpu``.

The first test searches the root of tests/golden/sweep_2p36_hashlib.json, every nonce of which in [0, 2^36) with a
value at or above fffffff800000000 is known (126 hits, found with hashlib): from S = 0x846e097c0 the next eight hits
are all below fffffffe00000000, the first of them 2^31.19 nonces (~70 ms of a whole GPU) from S, and the first hit
at or above fffffffe00000000 is 0xa312db930, 2^32.94 nonces from S.
"""
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
    return root, hits


def test_fixture_is_what_the_first_test_relies_on(fixture_hits):
    root, hits = fixture_hits
    after = sorted(n for n in hits if n >= S)
    assert after[:8] == [0x8d93d76ac, 0x9130d17a7, 0x96abd5eeb, 0x98526d64f, 0x9bb515b4a, 0xa245f2f6b, 0xa2bb24bcd,
                         0xa2e42222f]
    assert all(hits[n] < NEW for n in after[:8])
    assert after[8] == 0xa312db930 and hits[after[8]] == 0xfffffffe03ad1051
    assert next(n for n in after[9:] if hits[n] >= NEW) == 0xa8a343838


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


def test_solo_search_passes_stale_hits_in_place(gpu_engine, fixture_hits):
    """One launch covers 2^34 nonces densely from S.  The search is retargeted 5 ms after its submit -- its launch
    is running with the old threshold in its table by then, and the first hit under it is ~70 ms away; retargeted
    any sooner, the table itself could carry the new threshold and no hit would be stale -- and returns the first
    fixture hit at the new threshold out of that same launch."""
    eng = gpu_engine
    root, hits = fixture_hits
    eng.set_pool_tuning(budget_us=600000)
    eng.set_tuning(65536)
    try:
        s0 = _idle_stats(eng)
        t = eng.submit(root, OLD, start=S, device_mask=1)
        time.sleep(0.005)
        assert t.retarget(NEW) is True
        info = t.wait_info(60)
        s1 = _idle_stats(eng)
    finally:
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)
    assert info is not None and info.status == _lib.NPOW_OK
    between = [n for n in hits if S <= n < info.nonce and hits[n] < NEW]
    print(f"solo: nonce {info.nonce:x} value {info.value:016x}, stale_hits {info.stale_hits} (fixture hits passed "
          f"{len(between)}), stale_wins {info.stale_wins}, retargets {info.retargets}, launches {s0.launches} -> "
          f"{s1.launches}, yields {s0.yields} -> {s1.yields}")
    assert info.nonce in hits, f"{info.nonce:x} is no fixture hit"
    assert info.value == hits[info.nonce] and info.value >= NEW
    assert 1 <= info.stale_hits <= len(between), (info.stale_hits, len(between))
    assert info.stale_wins == 0 and info.retargets == 1
    assert s1.launches == s0.launches + 1, "the search took another launch"
    assert s1.yields == s0.yields


def test_beside_other_searches(gpu_engine):
    """Two endless searches share one counted launch (admitted together behind a blocker, as in
    tests/test_gpu_promote.py: submitted one after the other, the second would end the first one's launch); a third
    joins that launch as a dynamic entry 5 ms later and is retargeted at once."""
    eng = gpu_engine
    rx, ra, rb, rc = _roots(91, 4)
    toks = [_lib.CancelToken() for _ in range(3)]
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
        dyn0 = eng.stats(0).dyn_entries
        tc = eng.submit(rc, OLD, start=3 << 52, device_mask=1)
        assert tc.retarget(NEW) is True
        y0 = eng.stats(0).yields
        info = tc.wait_info(60)
        s1 = eng.stats(0)
    finally:
        eng.pool_config(64)
        for c in toks:
            c.set()
    ra_res, rb_res = ta.wait(30), tb.wait(30)
    print(f"beside two: nonce {info.nonce:x} value {info.value:016x}, stale_hits {info.stale_hits}, stale_wins "
          f"{info.stale_wins}, dyn_entries {dyn0} -> {s1.dyn_entries}, yields {y0} -> {s1.yields}")
    assert ra_res.status == _lib.NPOW_CANCELLED and rb_res.status == _lib.NPOW_CANCELLED
    assert info.status == _lib.NPOW_OK
    assert _value(rc, info.nonce) == info.value >= NEW
    assert info.stale_wins == 0 and info.retargets == 1
    assert s1.dyn_entries > dyn0, "the third search did not join the running launch"
    assert s1.yields == y0, "a launch was ended between the retarget and the result"


def test_waiting_job(gpu_engine):
    eng = gpu_engine
    eng.pool_config(1)
    try:
        r0, r1 = _roots(92, 2)
        tok = _lib.CancelToken()
        blocker = eng.submit(r0, M64, device_mask=1, cancel=tok)
        t = eng.submit(r1, RECEIVE, device_mask=1)
        assert eng.pool_status() == (1, 1)
        assert t.retarget(0xffffff0000000000) is True
        assert eng.pool_status() == (1, 1)
        tok.set()
        assert blocker.wait(30).status == _lib.NPOW_CANCELLED
        info = t.wait_info(30)
    finally:
        eng.pool_config(64)
    assert info.status == _lib.NPOW_OK
    assert _value(r1, info.nonce) == info.value >= 0xffffff0000000000
    assert info.stale_hits == 0 and info.retargets == 1 and info.stale_wins == 0


def test_results_stay_right(gpu_engine):
    """24 searches at receive difficulty, every third retargeted to fffffff000000000 right after its submit and
    again 1 ms later, every fourth cancelled: each result validates under hashlib against its own root at the
    threshold that held for it, and the pool's protocol checks stay at 0."""
    eng = gpu_engine
    raised = 0xfffffff000000000
    eng.reset_stats(0)
    inv0 = eng.stats(0).invalid_work
    roots = _roots(93, 24)
    tickets, toks, held = [], [], {}
    for i, r in enumerate(roots):
        c = _lib.CancelToken()
        t = eng.submit(r, RECEIVE, start=i << 48, device_mask=1, cancel=c)
        if i % 3 == 0:
            held[i] = t.retarget(raised)
        tickets.append(t)
        toks.append(c)
    time.sleep(0.001)
    for i, t in enumerate(tickets):
        if i % 3 == 0:
            t.retarget(raised)  # (idempotent; False for a search decided meanwhile)
        if i % 4 == 0:
            toks[i].set()
    n_ok = stale_hits = stale_wins = 0
    for i, (r, t) in enumerate(zip(roots, tickets)):
        info = t.wait_info(60)
        assert info is not None
        assert info.status in ((_lib.NPOW_OK, _lib.NPOW_CANCELLED) if i % 4 == 0 else (_lib.NPOW_OK,))
        stale_hits += info.stale_hits
        stale_wins += info.stale_wins
        if info.status == _lib.NPOW_OK:
            n_ok += 1
            assert _value(r, info.nonce) == info.value >= (raised if held.get(i) else RECEIVE), (i, held.get(i))
    st = eng.stats(0)
    print(f"24 searches: {n_ok} ok, first retargets held {sum(held.values())} of {len(held)}, stale_hits "
          f"{stale_hits}, stale_wins {stale_wins}")
    assert n_ok >= 18
    assert st.early_mismatches == 0 and st.stale_missing == 0, (st.early_mismatches, st.stale_missing)
    assert st.invalid_work == inv0 and st.dead == 0


def test_arguments(gpu_engine):
    eng = gpu_engine
    tok = _lib.CancelToken()
    t = eng.submit(_roots(94, 1)[0], OLD, device_mask=1, cancel=tok)
    try:
        assert t.retarget(OLD) is True and t.retarget(OLD - 1) is True and t.retarget(0) is True  # never lowered
        assert eng.lib.npow_retarget(t.ticket, RECEIVE) == _lib.NPOW_OK
        assert eng.lib.npow_retarget(0x7fffffff12345, M64) == _lib.NPOW_ERR_BAD_ARGUMENT  # no such ticket
        assert b"ticket" in eng.lib.npow_last_error()
    finally:
        tok.set()
        info = t.wait_info(30)
    assert info.status in (_lib.NPOW_CANCELLED, _lib.NPOW_OK) and info.retargets == 0
    assert eng.lib.npow_retarget(t.ticket, M64) == _lib.NPOW_ERR_BAD_ARGUMENT  # collected
    with pytest.raises(_lib.NanoPowError) as e:
        t.retarget(M64)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


def test_decided_but_uncollected_ticket_is_too_late(gpu_engine):
    eng = gpu_engine
    r, = _roots(96, 1)
    t = eng.submit(r, RECEIVE, device_mask=1)
    res = t.wait_result(30)
    assert res is not None and res.status == _lib.NPOW_OK
    assert eng.lib.npow_retarget(t.ticket, M64) == _lib.NPOW_TOO_LATE
    assert t.retarget(M64) is False
    assert t.retarget(RECEIVE) is True  # (not above its threshold: nothing asked for)
    info = t.wait_info(30)
    assert (info.status, info.nonce, info.value) == (_lib.NPOW_OK, res.nonce, res.value)
    assert _value(r, info.nonce) == info.value >= RECEIVE and info.retargets == 0


def test_bounded_search_is_accepted(gpu_engine):
    eng = gpu_engine
    tok = _lib.CancelToken()
    t = eng.submit(_roots(97, 1)[0], OLD, device_mask=1, max_nonces_per_device=1 << 40, cancel=tok)
    try:
        assert t.retarget(M64) is True
    finally:
        tok.set()
        info = t.wait_info(30)
    assert info.status in (_lib.NPOW_CANCELLED, _lib.NPOW_EXHAUSTED) and info.retargets == 1


def _worker(mode, **env):
    p = subprocess.run([sys.executable, os.path.join(HERE, "retarget_worker.py"), mode], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"{mode}: {out}")
    return out, p.stderr


def test_two_cu_partitions():
    """A search split over two CU partitions, retargeted while both hash it: each device gets its own floor record."""
    out, _ = _worker("partitions", NANOPOW_VIRTUAL_DEVICES="2")
    assert out["held"] is True and out["status"] == _lib.NPOW_OK and out["n_devices"] == 2
    assert out["hashlib"] == out["value"] >= NEW
    assert out["stale_wins"] == 0 and out["retargets"] == 1
    for d in out["after"]:
        assert d["early_mismatches"] == 0 and d["stale_missing"] == 0 and d["dead"] == 0, out["after"]


def test_fallback_refuses_a_stale_win_and_rearms():
    """No floor record is written (the test hook): the launch publishes its first hit under the old threshold, the
    host refuses it -- correct work at the wrong difficulty, not invalid work -- and the search goes on."""
    out, err = _worker("blind", NANOPOW_FAULT_RETARGET_BLIND="1", NANOPOW_TEST_HOOKS="1")
    assert "TEST HOOKS ACTIVE" in err
    assert out["held"] is True and out["status"] == _lib.NPOW_OK
    assert out["hashlib"] == out["value"] >= NEW
    assert out["stale_wins"] >= 1 and out["retargets"] == 1
    assert out["after"][0]["invalid_work"] == out["before"][0]["invalid_work"]
    assert out["after"][0]["dead"] == 0
