"""The hit test `value >= threshold` at thresholds whose low 32 bits decide.  Run on an MI355X: ``pytest -m gpu``.

Every result of the engine hangs on that one 64-bit comparison (npow_kernel.hip: `bool hit = value >= thr;` in
pool_body_ls2, both instantiations -- sweep jobs, best jobs and both win branches hang off it --, `value >= cur` and
`value >= ethr` in the hit branch, the ballot of npow_sweep_kernel_ls2), and the fixtures' thresholds have 40 low
zero bits.  A kernel that compares the high words only, compares the low words as signed integers, requires both words
to be >= or uses > for >= would pass them.  Here the thresholds are the rungs of tests/threshold_ladder.py around a
value the oracle knows: the sole hit of a launch's window (tests/search_positions.py), or the top three values of a range.

All expectations are exact and come from the oracle and hashlib; nothing here compares with a tolerance.  A rung that
the value meets ("yes"): the search returns h with value(h).  A rung it does not ("no"): the search returns a later
nonce, not h, whose hashlib value is at or above T -- about 2^-24 of all values are, so it ends within a few windows.

Out of scope: the low word of the in-launch floor read (`value >= cur` once npow_retarget or npow_relax reaches a
RUNNING launch) and reserve candidates -- a parked or dynamic entry starts at each workgroup's current iteration and a
reserve search runs on past its first window, so neither has a window the oracle covers in seconds;
tests/test_gpu_hit_branch.py covers those paths with full and quarter masks.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import search_position_worker as spw
import search_positions as sp
import threshold_ladder as tl
import threshold_ladder_worker as tlw
from nanopow import _lib
from oracle import work_value_hashlib

pytestmark = pytest.mark.gpu
M64 = sp.M64
HERE = os.path.dirname(os.path.abspath(__file__))
ZERO = {"yields": 0, "dyn_entries": 0, "invalid_work": 0}


def collect(t, timeout=60.0):
    """The ticket's result; a search that has not ended by then is cancelled (nothing is left running) and gives
    None."""
    x = t.wait(timeout)
    if x is None:
        t.cancel()
        t.wait(30)
    return x


@pytest.fixture(scope="module")
def grid(gpu_engine):
    return spw.whole_window_device(gpu_engine, 0, False)


@pytest.fixture(scope="module")
def windows(grid):
    t0 = time.monotonic()
    ws = tl.window_ladders(grid)
    print(f"window ladders, grid {grid}: oracle {time.monotonic() - t0:.2f} s; " +
          ", ".join(f"{a} seed {w.sh.seed} m1 {w.m1:016x} m2 {w.m2:016x}" for a, w in ws.items()))
    return ws


@pytest.fixture(scope="module")
def ranges():
    t0 = time.monotonic()
    rls = tl.range_ladders()
    print(f"range ladders: oracle {time.monotonic() - t0:.2f} s; " +
          ", ".join(f"{r.name} {[f'{v:016x}' for _, v in r.top[:3]]}" for r in rls))
    return rls


def test_unbounded_one_entry(gpu_engine, windows):
    """npow_pool_kernel_ls2_arg<false>: all three anchors, every rung, h at the first and the last position of the
    window (iteration 0, workgroup 0, wave 0, lane 0; iteration 15, the last workgroup, wave 7, lane 63)."""
    eng = gpu_engine
    assert tl.mixed([w.m1 for w in windows.values()])
    failures, n = [], 0
    t0 = time.monotonic()
    with spw.tuned(eng):
        c0 = spw.counters(eng, [0])[0]
        for w in windows.values():
            ps = (0, w.sh.full - 1)
            failures += tlw.one_entry_ladder(eng, w, ps)
            n += len(w.rungs) * len(ps)
        c1 = spw.counters(eng, [0])[0]
    print(f"{n} searches {time.monotonic() - t0:.2f} s")
    assert n == 3 * 8 * 2
    assert failures == [], f"{len(failures)} of {n}: {failures[:8]}"
    assert c1 == c0, (c0, c1)


# (bit 31 of m1, n, rung, the hit's (it, g from the grid's end, wv, lane)); 17 entries are more than kArgEntries, so
# that table is read from device memory (npow_pool_kernel_ls2<false>).  flip31 runs in both directions: "yes" where bit
# 31 of m1 is set, "no" where it is clear.
COPIES = [(False, 2, "hi-1", (15, 1, 7, 63)), (False, 2, "above", (0, 2, 0, 0)),
          (True, 17, "flip31", (15, 1, 7, 63)), (True, 17, "lomax", (9, 17, 2, 1)),
          (False, 17, "flip31", (0, None, 5, 62)), (False, 17, "lomax", (15, 1, 7, 63))]


@pytest.mark.parametrize("bit,n,rung,where", COPIES,
                         ids=[f"{'set' if b else 'clear'}-{n}-{r}" for b, n, r, _ in COPIES])
def test_unbounded_copies_in_one_table(gpu_engine, grid, windows, bit, n, rung, where):
    """n identical searches in one counted launch (tests/test_gpu_search_positions.py test_copies_in_one_table): at a
    "yes" rung exactly one copy returns h, at a "no" rung none does, and every result validates at T."""
    eng = gpu_engine
    assert grid > 2 * 17
    w = next(x for x in windows.values() if tl.bit31(x.m1) == bit)  # (the first anchor with that bit 31)
    sh, r = w.sh, tl.rung(w.m1, rung)
    anchor = sh.anchor
    assert r.meets == {"hi-1": True, "above": False, "flip31": bit, "lomax": False}[rung]
    it, back, wv, lane = where
    g = 16 if back is None else grid - back
    pos = sp.pos_of(it, g, wv, lane, grid)
    with spw.tuned(eng):
        results, deltas = spw.copies_in_one_table(eng, sh, pos, n, sp.root_of(1100 + n), threshold=r.T)
    print(f"{anchor}, n {n}, {rung} T {r.T:016x} ({'yes' if r.meets else 'no'}): nonces "
          f"{[f'{x.nonce:016x}' if x and x.nonce is not None else x for x in results]}, deltas {deltas}")
    assert deltas == ZERO
    assert all(x is not None and x.status == _lib.NPOW_OK for x in results)
    assert sum(1 for x in results if x.nonce == sh.h) == (1 if r.meets else 0)
    for x in results:
        v = work_value_hashlib(sh.root, x.nonce)
        assert v == int(x.value) and v >= r.T, (f"{x.nonce:016x}", f"{x.value:016x}")
        assert x.nonce != sh.h or x.value == w.m1


def test_bounded_win_branch(gpu_engine, grid, windows):
    """pool_body_ls2<true>'s win branch: a bounded search of F nonces beside four endless unbounded searches, h at the
    first and the last nonce of the range, every rung of two anchors (bit 31 of m1 set and clear)."""
    eng = gpu_engine
    two = tl.two_anchors(grid)
    toks = [_lib.CancelToken() for _ in range(4)]
    endless, failures = [], []
    inv0 = eng.stats(0).invalid_work
    t0 = time.monotonic()
    with spw.tuned(eng):
        try:
            endless = [eng.submit(sp.root_of(2100 + i), M64, start=(i + 1) << 52, device_mask=1, cancel=toks[i])
                       for i in range(4)]
            for w in two:
                sh, F = w.sh, w.sh.full
                for r in w.rungs:
                    for pos in (0, F - 1):
                        x = collect(eng.submit(sh.root, r.T, start=sp.start_of(sh, pos), device_mask=1,
                                               max_nonces_per_device=F))
                        if r.meets:
                            ok = x is not None and (x.status, x.nonce, x.value) == (_lib.NPOW_OK, sh.h, w.m1)
                        else:
                            ok = x is not None and x.status == _lib.NPOW_EXHAUSTED and x.nonces_done == F
                        if not ok:
                            failures.append((sh.anchor, r.name, f"{r.T:016x}", r.meets, pos, x))
            assert all(t.wait(0) is None for t in endless), "an endless search ended"
        finally:
            for c in toks:
                c.set()
            ended = [t.wait(30) for t in endless]
    print(f"32 bounded searches {time.monotonic() - t0:.2f} s")
    assert failures == []
    assert all(x is not None and x.status == _lib.NPOW_CANCELLED for x in ended)
    assert eng.stats(0).invalid_work == inv0


@pytest.mark.parametrize("kind", tlw.SWEEP_KINDS)
def test_enumeration(gpu_engine, ranges, kind):
    """The blocking npow_sweep (npow_sweep_kernel_ls2) and a plain, a background and a shared sweep job
    (pool_body_ls2<true>, collecting entries): the three ranges at every rung of their top three values.  The hit
    list and n_out equal the oracle's, nonces_done == count."""
    eng = gpu_engine
    inv0 = eng.stats(0).invalid_work
    t0 = time.monotonic()
    failures = [f for rl in ranges for f in tlw.sweep_ladder(eng, rl, kind)]
    print(f"{kind}: {3 * 8 * tl.LADDERED} sweeps {time.monotonic() - t0:.2f} s")
    assert failures == [], f"{len(failures)}: {failures[:6]}"
    assert eng.stats(0).invalid_work == inv0


@pytest.mark.parametrize("kind", tlw.BEST_KINDS)
def test_best_jobs(gpu_engine, ranges, kind):
    """Best jobs, plain, background and shared: the floor at every rung of the range's maximum -- (NPOW_OK, argmax,
    max), or NPOW_EXHAUSTED with nonces_done == count -- and at every rung of the second value: the maximum."""
    eng = gpu_engine
    t0 = time.monotonic()
    failures = [f for rl in ranges for f in tlw.best_ladder(eng, rl, kind)]
    print(f"{kind}: {3 * 16} best jobs {time.monotonic() - t0:.2f} s")
    assert failures == [], f"{len(failures)}: {failures[:6]}"


def test_raised_while_waiting(gpu_engine, grid, windows):
    """A bounded search of F nonces at T0 = lo0(m1), queued behind a blocker (npow_pool_config(1)), is retargeted to
    each rung before it is admitted: npow_retarget returns NPOW_OK and the outcome is the one max(T0, T) implies."""
    eng = gpu_engine
    failures = []
    t0 = time.monotonic()
    with spw.tuned(eng):
        inv0 = eng.stats(0).invalid_work
        eng.pool_config(1)
        for w in tl.two_anchors(grid):
            sh, F = w.sh, w.sh.full
            T0 = tl.rung(w.m1, "lo0").T
            assert w.m2 < T0 < w.m1
            for r in w.rungs:
                pos = (0, F - 1)[tl.NAMES.index(r.name) % 2]
                tok = _lib.CancelToken()
                blocker = eng.submit(sp.root_of(2200), M64, device_mask=1, cancel=tok)
                try:
                    t = eng.submit(sh.root, T0, start=sp.start_of(sh, pos), device_mask=1, max_nonces_per_device=F)
                    assert eng.pool_status() == (1, 1)
                    raised = t.retarget(r.T)  # (True: NPOW_OK, also where T is not above T0 and nothing changes)
                    assert eng.pool_status() == (1, 1)
                finally:
                    tok.set()
                    b = blocker.wait(30)
                x = collect(t)
                assert b is not None and b.status == _lib.NPOW_CANCELLED
                if w.m1 >= max(T0, r.T):
                    ok = x is not None and (x.status, x.nonce, x.value) == (_lib.NPOW_OK, sh.h, w.m1)
                else:
                    ok = x is not None and x.status == _lib.NPOW_EXHAUSTED and x.nonces_done == F
                if not (ok and raised is True):
                    failures.append((sh.anchor, r.name, f"{r.T:016x}", raised, pos, x))
        inv1 = eng.stats(0).invalid_work
    print(f"16 waiting searches {time.monotonic() - t0:.2f} s")
    assert failures == []
    assert inv1 == inv0


def test_cu_partitions():
    """NANOPOW_VIRTUAL_DEVICES=2, in a child process (tests/threshold_ladder_worker.py): the one-entry ladder on
    partition 1 with that grid's own sole hits, and one range's sweep-job and best-job ladders split over both."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "threshold_ladder_worker.py")],
                       env=dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2"), capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"partitions: grids {out['grids']}, {out['alone']} searches on partition 1, {out['split']} split jobs; "
          f"oracle {out['oracle_seconds']} s, GPU {out['gpu_seconds']} s")
    assert out["n_devices"] == 2 and out["failures"] == []
    assert out["alone"] == 3 * 8 * 2 and out["split"] == 3 * (8 * tl.LADDERED + 16) and out["bit31"] == [False, True]
    assert out["deltas"] == [ZERO] * 2
