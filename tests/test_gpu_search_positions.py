"""The unbounded first-win kernel (npow_kernel.hip pool_body_ls2<false>, launched as npow_pool_kernel_ls2_arg<false>
and, past kArgEntries entries, npow_pool_kernel_ls2<false>) loses no hit, wherever in a launch's window the hit lies.
Run on an MI355X: ``pytest -m gpu``.

Every unbounded winner is re-validated on the host, so a wrong value is caught; a LOST hit only makes a search a
little slower, and the statistical tests of the search times would pass a kernel that skips 1/16 of its range.  Here
each search has exactly one nonce h at or above its threshold in the window of its first launch (the construction:
tests/search_positions.py), at a chosen iteration, workgroup, wave and lane: it must return h.  A kernel that does not
run its last iteration, drops a lane from the ballot, lets one wave's blocks alias another's or loses the carry of
`nonce += step` into the high word returns a later nonce instead -- the search ends by itself within a few launches
and the assertion shows the wrong nonce.

The tunings make a launch 16 wave iterations long (well under a millisecond) under a time budget of 0.4 s, so no
launch ends on its budget and each covers its whole window.

Out of scope, by design of the kernel: a dynamic entry (a search that joins a running counted launch) and a search
taken by a lingering launch start at each workgroup's current iteration, not at block 0, so their first launch covers
no fixed window.  The tests assert that neither occurs (dyn_entries, and a device that does not linger: the whole GPU,
or a CU partition of more than 32 CUs).
"""
import json
import os
import subprocess
import sys
import time

import pytest

import search_position_worker as spw
import search_positions as sp
from nanopow import _lib
from oracle import work_value_hashlib

pytestmark = pytest.mark.gpu
M64 = sp.M64
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def grid(gpu_engine):
    return spw.whole_window_device(gpu_engine, 0, False)


@pytest.mark.parametrize("anchor", sp.ANCHORS)
def test_every_edge_one_entry(gpu_engine, grid, anchor):
    """A one-entry table, the hit at: the 16 corners of (iteration, workgroup, wave, lane); 64 positions that cover
    every lane, wave, iteration and XCD shard; both sides of three iteration boundaries; and, for the carry anchors,
    the first iteration whose wave has crossed 2^32 (or 2^64) in `nonce += step` before it reaches h -- the corners
    of the last iteration cross it too."""
    eng = gpu_engine
    t0 = time.monotonic()
    sh = sp.sole_hit(grid, anchor)
    t1 = time.monotonic()
    ps = sp.positions(sh)
    assert len(ps) == (86 if sh.boundary is None else 87)
    if sh.boundary is not None:
        crossing = [p for p in ps if sp.carried(sh, p)]
        assert set(sp.corners(grid)[8:]) <= set(crossing) and sp.first_carry(sh) in crossing
        print(f"{anchor}: {len(crossing)} of {len(ps)} positions cross the boundary before h")
    failures = []
    with spw.tuned(eng):
        c0 = spw.counters(eng, [0])[0]
        for pos in ps:
            bad = spw.sole_search(eng, sh, pos)
            if bad:
                failures.append(bad)
        c1 = spw.counters(eng, [0])[0]
    print(f"{anchor}: grid {grid}, F {sh.full}, seed {sh.seed}, h {sh.h:016x}, T {sh.threshold:016x}; oracle "
          f"{t1 - t0:.2f} s, {len(ps)} searches {time.monotonic() - t1:.2f} s")
    assert failures == [], f"{len(failures)} of {len(ps)} positions: {failures[:8]}"
    assert c1 == c0, (c0, c1)


# (anchor, n, the hit's (it, g from the grid's end, wv, lane)): one g of each residue mod n for n = 2 and 3, the last
# workgroup among them; 17 entries are more than kArgEntries, so that table is read from device memory
COPIES = [("plain", 2, (15, 1, 7, 63)), ("plain", 2, (0, 2, 0, 0)),
          ("carry32", 3, (15, 1, 7, 63)), ("carry32", 3, (8, 2, 3, 31)), ("carry32", 3, (1, 3, 4, 32)),
          ("wrap64", 17, (15, 1, 7, 63)), ("wrap64", 17, (9, 17, 2, 1)), ("plain", 17, (0, None, 5, 62))]


@pytest.mark.parametrize("anchor,n,where", COPIES, ids=[f"{a}-{n}-{i}" for i, (a, n, _) in enumerate(COPIES)])
def test_copies_in_one_table(gpu_engine, grid, anchor, n, where):
    """n identical searches in one counted launch: equal weights deal workgroup g to entry g % n (PoolTable::wsum 0)
    and the kernel balances workgroups only toward dynamic entries, so exactly one copy covers h in its first launch
    and must win with it; the workgroups that leave the won copy go on at their current iteration, past h's block.
    The other copies find a later nonce."""
    eng = gpu_engine
    assert grid % 3 != 0 and grid > 2 * 17  # (every entry has workgroups; three entries' counts differ)
    sh = sp.sole_hit(grid, anchor)
    it, back, wv, lane = where
    g = 16 if back is None else grid - back  # (None: workgroup 16, entry 16 of 17 -- the entry past kArgEntries)
    pos = sp.pos_of(it, g, wv, lane, grid)
    with spw.tuned(eng):
        results, deltas = spw.copies_in_one_table(eng, sh, pos, n, sp.root_of(1000 + n))
    print(f"{anchor}, n {n}, (it, g, wv, lane) {(it, g, wv, lane)}, entry {g % n}: nonces "
          f"{[f'{r.nonce:016x}' if r and r.nonce is not None else r for r in results]}, deltas {deltas}")
    assert deltas == {"yields": 0, "dyn_entries": 0, "invalid_work": 0}
    assert all(r is not None and r.status == _lib.NPOW_OK for r in results)
    assert sum(1 for r in results if r.nonce == sh.h) == 1, "the copy whose workgroups cover h lost it (or two had it)"
    for r in results:
        assert r.nonce == sh.h or work_value_hashlib(sh.root, r.nonce) == r.value >= sh.threshold


def test_bounded_first_win_at_the_same_positions(gpu_engine, grid):
    """The BOUNDED kernel's win branch: a bounded search of F nonces beside four endless unbounded searches -- its
    entry's own span is about F / 5, so the range takes several launches and h falls at an arbitrary place of the
    entry's dense mapping (last_b, tail).  With the range ending right before h: exhausted, every nonce counted."""
    eng = gpu_engine
    sh = sp.sole_hit(grid, "plain")
    F = sh.full
    toks = [_lib.CancelToken() for _ in range(4)]
    endless = []
    failures = []
    inv0 = eng.stats(0).invalid_work
    with spw.tuned(eng):
        try:
            endless = [eng.submit(sp.root_of(2000 + i), M64, start=(i + 1) << 52, device_mask=1, cancel=toks[i])
                       for i in range(4)]
            for pos in (0, 1, 63, 64, F // 2, F - 65, F - 64, F - 1):
                r = eng.submit(sh.root, sh.threshold, start=sp.start_of(sh, pos), device_mask=1,
                               max_nonces_per_device=F).wait(60)
                if not (r is not None and r.status == _lib.NPOW_OK and r.nonce == sh.h and r.value == sh.threshold):
                    failures.append(("win", pos, r))
            for pos in (1, 63, 64, F // 2, F - 1):
                r = eng.submit(sh.root, sh.threshold, start=sp.start_of(sh, pos), device_mask=1,
                               max_nonces_per_device=pos).wait(60)
                if not (r is not None and r.status == _lib.NPOW_EXHAUSTED and r.nonces_done == pos):
                    failures.append(("exhausted", pos, r))
            assert all(t.wait(0) is None for t in endless), "an endless search ended"
        finally:
            for c in toks:
                c.set()
            ended = [t.wait(30) for t in endless]
    assert failures == []
    assert all(r is not None and r.status == _lib.NPOW_CANCELLED for r in ended)
    assert eng.stats(0).invalid_work == inv0


def test_cu_partitions():
    """On CU partition 1 of 2 (its own grid and window: device_mask 2), and split over both (device_mask 3, the hit in
    partition 1's stride), in a child process."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "search_position_worker.py")],
                       env=dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2"), capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"partitions: grids {out['grids']}, {out['alone']} searches on partition 1, split {out['split']}, "
          f"{out['seconds']} s")
    assert out["n_devices"] == 2 and out["failures"] == []
    assert out["alone"] == 3 * 32 + 2 and len(out["split"]) == 4
    assert out["deltas"] == [{"yields": 0, "dyn_entries": 0, "invalid_work": 0}] * 2
