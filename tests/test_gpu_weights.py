"""Weighted job shares of the GPU work pool (npow_submit_weighted, ABI 7): a job of weight w in {1, 2, 4, 8}
gets w / (sum of weights) of its device's workgroups among the live unbounded jobs, in a launch's start map
and through the scaled balancing rule for jobs that join a running launch; waiting jobs are admitted heaviest
first.  Every test runs on device 0 only.  Run on an MI355X: ``pytest -m gpu``.

The share bounds are the geometric midpoints between the ratio a weight stands for and the ratios of its
neighbours in the weight set -- they follow from {1, 2, 4, 8}, not from measurements.
"""
import hashlib
import math
import random
import time

import pytest

from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE = 0xfffffe0000000000
RUN_S = 0.2


def _roots(seed, n):
    rng = random.Random(seed)
    return [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(n)]


def _value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


def _endless(eng, roots, weights, plain=()):
    """Unwinnable jobs (threshold 2^64 - 1) submitted back to back; those whose index is in `plain` go through
    npow_submit (Engine.submit without the weight keyword takes the weighted call, so the C call is made here)."""
    import ctypes
    toks = [_lib.CancelToken() for _ in roots]
    tickets = []
    for i, (r, w, c) in enumerate(zip(roots, weights, toks)):
        if i in plain:
            assert w == 1
            t = ctypes.c_uint64(0)
            rc = eng.lib.npow_submit(r, M64, (i + 1) << 52, 1, 0, c.address, ctypes.byref(t))
            assert rc == _lib.NPOW_OK
            tickets.append(_lib.Ticket(eng, t.value, c))
        else:
            tickets.append(eng.submit(r, M64, start=(i + 1) << 52, device_mask=1, cancel=c, weight=w))
    return toks, tickets


def _run_and_count(eng, roots, weights, plain=(), run_s=RUN_S):
    toks, tickets = _endless(eng, roots, weights, plain)
    time.sleep(run_s)
    for c in toks:
        c.set()
    done = []
    for t in tickets:
        res = t.wait(30)
        assert res is not None and res.status == _lib.NPOW_CANCELLED
        done.append(res.nonces_done)
    return done


def test_static_share_follows_the_weights(gpu_engine):
    """Two endless jobs of weights (1, 4) for ~200 ms: the nonce counts' ratio is nearer to 4 than to 2 or 8 on a
    log scale; weights (1, 1) -- one of them through npow_submit -- stay within sqrt(2) of each other, so those
    margins do not hide an imbalance of the pool itself."""
    a, b = _run_and_count(gpu_engine, _roots(71, 2), (1, 4))
    r = b / max(a, 1)
    print(f"weights (1, 4): nonces {a} / {b}, ratio {r:.3f}")
    assert math.sqrt(8) < r < math.sqrt(32), f"weights (1, 4): ratio {r:.3f} ({a} / {b} nonces)"
    a, b = _run_and_count(gpu_engine, _roots(72, 2), (1, 1), plain=(0,))
    r1 = b / max(a, 1)
    print(f"weights (1, 1): nonces {a} / {b}, ratio {r1:.3f}")
    assert 1 / math.sqrt(2) < r1 < math.sqrt(2), f"weights (1, 1): ratio {r1:.3f} ({a} / {b} nonces)"


def test_one_heavy_job_among_eight_light_ones(gpu_engine):
    """Eight jobs of weight 1 and one of weight 8: the heavy one gets half the nonces (weight 4 would get a third;
    the bounds are the geometric midpoint towards that neighbour and its mirror image)."""
    done = _run_and_count(gpu_engine, _roots(73, 9), [1] * 8 + [8])
    share = done[8] / max(sum(done), 1)
    print(f"8 x weight 1 + weight 8: heavy share {share:.4f} (light jobs {done[:8]}, heavy {done[8]})")
    assert 0.408 < share < 0.612, f"heavy share {share:.4f} of {sum(done)} nonces"


def test_heavy_job_joins_a_running_launch(gpu_engine):
    """A weight-8 job published into a running launch (a dynamic entry) collects its share through the scaled
    balancing rule: started 20 ms after two weight-1 jobs and cancelled with them 100 ms later, it has hashed more
    than both together (with equal shares it could not even pass one of them).

    A and B must share one counted launch that outlasts the test.  A job submitted alone starts a one-entry launch,
    which the next job ends, so they are admitted together instead: they wait behind a blocker under max_active 1
    and are let in by one pool_config call; the blocker is cancelled before the clock starts."""
    eng = gpu_engine
    eng.set_pool_tuning(budget_us=400000)  # one launch lasts past the test: ...
    eng.set_tuning(65536)                  # ... 32,768 wave iterations, ~0.4 s
    eng.pool_config(1)
    try:
        rx, ra, rb, rc = _roots(74, 4)
        toks = [_lib.CancelToken() for _ in range(4)]
        tx = eng.submit(rx, M64, device_mask=1, cancel=toks[3])
        ta = eng.submit(ra, M64, start=1 << 52, device_mask=1, cancel=toks[0], weight=1)
        tb = eng.submit(rb, M64, start=2 << 52, device_mask=1, cancel=toks[1], weight=1)
        assert eng.pool_status() == (2, 1)
        eng.pool_config(64)  # A and B are admitted, and adopted, together
        toks[3].set()
        assert tx.wait(30).status == _lib.NPOW_CANCELLED
        t0 = time.monotonic()
        time.sleep(0.02)
        dyn0 = eng.stats(0).dyn_entries
        tc = eng.submit(rc, M64, start=3 << 52, device_mask=1, cancel=toks[2], weight=8)
        time.sleep(max(0.0, t0 + 0.12 - time.monotonic()))
        dyn1 = eng.stats(0).dyn_entries
        for c in toks:
            c.set()
        da, db, dc = (t.wait(30).nonces_done for t in (ta, tb, tc))
    finally:
        eng.pool_config(64)
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)
    ratio = dc / max(da + db, 1)
    print(f"dynamic join: A {da} B {db} C {dc}, C / (A + B) = {ratio:.3f}, dyn_entries {dyn0} -> {dyn1}")
    assert dyn1 > dyn0, "the weight-8 job did not join the running launch"
    assert dc > da + db, f"C / (A + B) = {ratio:.3f} (A {da}, B {db}, C {dc})"


def test_results_stay_right(gpu_engine):
    """More weight than a launch has table entries (20 x 8), then every weight mixed with cancellations: each
    result validates under hashlib against its own root, and the pool's protocol checks stay at 0."""
    eng = gpu_engine
    eng.reset_stats(0)
    roots = _roots(75, 36)
    heavy = [eng.submit(r, RECEIVE, start=i << 48, device_mask=1, weight=8) for i, r in enumerate(roots[:20])]
    mixed, toks = [], []
    for i, r in enumerate(roots[20:]):
        c = _lib.CancelToken()
        mixed.append(eng.submit(r, RECEIVE, start=(i + 20) << 48, device_mask=1, cancel=c, weight=(1, 2, 4, 8)[i % 4]))
        toks.append(c)
        if i % 2:
            c.set()
    for r, t in zip(roots[:20], heavy):
        res = t.wait(60)
        assert res is not None and res.status == _lib.NPOW_OK
        assert _value(r, res.nonce) == res.value >= RECEIVE
    for i, (r, t) in enumerate(zip(roots[20:], mixed)):
        res = t.wait(60)
        assert res is not None and res.status in ((_lib.NPOW_OK, _lib.NPOW_CANCELLED) if i % 2 else (_lib.NPOW_OK,))
        if res.status == _lib.NPOW_OK:
            assert _value(r, res.nonce) == res.value >= RECEIVE
    st = eng.stats(0)
    assert st.early_mismatches == 0 and st.stale_missing == 0, (st.early_mismatches, st.stale_missing)


@pytest.mark.parametrize("weight,bounded", [(0, 0), (3, 0), (16, 0), (2, 1 << 20)])
def test_bad_weights_are_refused(gpu_engine, weight, bounded):
    with pytest.raises(_lib.NanoPowError) as e:
        gpu_engine.submit(bytes(32), M64, device_mask=1, max_nonces_per_device=bounded, weight=weight)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


def test_heavier_waiting_job_is_admitted_first(gpu_engine):
    """max_active 1: behind a running job wait a weight-1 job and then a weight-8 job; when the running one ends,
    the weight-8 job is adopted first."""
    eng = gpu_engine
    eng.pool_config(1)
    try:
        r0, r1, r8 = _roots(76, 3)
        tok = _lib.CancelToken()
        first = eng.submit(r0, M64, device_mask=1, cancel=tok)
        s1 = time.monotonic()
        light = eng.submit(r1, RECEIVE, device_mask=1, weight=1)
        s8 = time.monotonic()
        heavy = eng.submit(r8, RECEIVE, device_mask=1, weight=8)
        assert eng.pool_status() == (2, 1)
        tok.set()
        assert first.wait(30).status == _lib.NPOW_CANCELLED
        i8, i1 = heavy.wait_info(30), light.wait_info(30)
    finally:
        eng.pool_config(64)
    assert i8.status == _lib.NPOW_OK and i1.status == _lib.NPOW_OK
    a8, a1 = s8 + i8.adopt_us * 1e-6, s1 + i1.adopt_us * 1e-6
    assert a8 < a1, f"weight 8 adopted {(a8 - a1) * 1e3:.3f} ms after weight 1"


def test_crowded_table_on_a_cu_partition_starves_no_job():
    """A device of 128 workgroups (one of 8 CU partitions, a child process: the engine reads NANOPOW_VIRTUAL_DEVICES
    once) with twenty weight-8 jobs and one of weight 1: the weights' sum, 161, exceeds the grid, and a start map
    over it would leave the entries past workgroup 127 without a workgroup in every launch.  The table builder
    halves the weights to 4 and 1 (sum 81), so each heavy job starts with 4 or 8 workgroups -- the smallest heavy
    count is at least a quarter of the largest (2 : 1 from the map, and as much again for the launches' starts) --
    and the light job, with one workgroup, hashes too, less than any heavy one."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="8")
    p = subprocess.run([sys.executable, os.path.join(here, "weights_partition_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    heavy, light = out["nonces"][:20], out["nonces"][20]
    print(f"grid {out['grid']}: heavy min {min(heavy)} max {max(heavy)}, light {light}")
    assert out["grid"] == 128
    assert min(heavy) * 4 >= max(heavy), f"heavy jobs' nonces {heavy}"
    assert 0 < light < min(heavy), f"light {light}, heavy min {min(heavy)}"
    assert out["early_mismatches"] == 0 and out["stale_missing"] == 0
