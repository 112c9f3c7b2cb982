"""Which nonce the reserve holds (npow_submit_reserve, npow_ticket_reserve, npow_relax), exactly.  Run on an MI355X:
``pytest -m gpu``.

The reserve comes out of the pool kernel's rare branch (npow_kernel.hip pool_body_ls2, ``if (hits != 0)``): the hit
mask is sorted into wins, stale hits and candidates (``cand = hits & ~keep & ~stale``), a loop over ``cand`` keeps the
larger value, ``readlane64(nonce, cl)`` reads its nonce from the lane, and ls2_publish_reserve publishes it through a
truncated key (pool_reserve_key).  A kernel that loses a candidate in some lanes, reads the nonce from the wrong lane,
compares ``value >= cur`` on the high words, orders keys by the wrong bits or never raises the record after its first
store yields no invalid work -- the host recomputes every record and drops what comes out below the reserve threshold --
it only costs npow_relax its "answered at once".  tests/test_gpu_reserve.py polls until *some* reserve appears; here
each search has one right reserve.

The construction (tests/reserve_records.py): the root of tests/golden/sweep_2p36_hashlib.json has every nonce of
[0, 2^36) at or above fffffff800000000 pinned by hashlib.  A record h has no higher value in [h - F, h + Z], F the
window of one launch; a search started at S = h - pos has h in its first launch at the chosen (iteration, workgroup,
wave, lane) -- the positions of tests/search_positions.py -- and for Z = 2^33 nonces (about a quarter of a second of a
whole MI355X; a condition of the construction) nothing can displace h or decide a search at v(h) + 1.  The tunings are
search_position_worker.tuned(): 16 wave iterations per launch, no launch ends on its budget.  No test sleeps a guessed
time: each polls against a 10 s deadline, and gives up sooner only on the device's `launches` counter
(tests/reserve_exact_worker.py).

Out of reach, and said so: several candidates in one wave, which the ``do ... while (cand)`` loop handles, need two
values at or above NPOW_RESERVE_MIN within 64 nonces -- one pair per about 2^34 nonces; the fixture's closest pair is
2^22 apart.  Such a pair sits at the 2^-20 level, where the next candidate or win comes within a launch, before any
harvest: no deterministic test reaches it, and none approximates it statistically here.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import reserve_exact_worker as rw
import reserve_records as rr
import search_position_worker as spw
import search_positions as sp
from nanopow import _lib
from test_gpu_reserve import _Solo

pytestmark = pytest.mark.gpu
M64 = rr.M64
HERE = os.path.dirname(os.path.abspath(__file__))
ZERO = {"yields": 0, "dyn_entries": 0, "invalid_work": 0}


@pytest.fixture(scope="module")
def grid(gpu_engine):
    return spw.whole_window_device(gpu_engine, 0, False)


@pytest.fixture(scope="module")
def two_records(grid):
    """(first, second) for the device's grid (reserve_exact_worker.pick), with their fixture root and values."""
    first, second = rw.pick(sp.full(grid))
    _, hits = rr.fixture()
    assert rr.low_word_decides(hits[first]) and rr.low_word_decides(hits[second])
    return first, second


def _sh(h, grid):
    root, hits = rr.fixture()
    return sp.SoleHit(grid, "fixture", None, root, None, h, hits[h], sp.full(grid), None, None)


def test_sole_candidate_at_every_edge(gpu_engine, grid, two_records):
    """T = 2^64 - 1, R = v(h), the record at each of the 86 positions of a one-entry launch: the first reserve the
    host ever reads is (h, v(h)); relax(v(h) + 1) is lowered in place, relax(v(h)) answered at once with h;
    stale_hits == stale_wins == 0; reserve_info answered, h, device 0; no yield, no dynamic entry, no invalid work."""
    h = two_records[0]
    ps = sp.positions(_sh(h, grid))
    assert len(ps) == 86
    t0 = time.monotonic()
    n, failures, deltas = rw.exact_many(gpu_engine, h, ps, grid, rr.ladder(h)[:1])
    print(f"grid {grid}, record {h:x} {rr.fixture()[1][h]:016x}: {n} searches {time.monotonic() - t0:.2f} s")
    assert n == 86 and failures == [], f"{len(failures)} of {n}: {failures[:6]}"
    assert deltas == ZERO


@pytest.mark.parametrize("which", [0, 1])
def test_the_ladder(gpu_engine, grid, two_records, which):
    """The five other candidate rungs of (T, R) -- T in {2^64 - 1, v + 1}, R in {v, v - 1, fffffff800000000} -- at the
    16 corners and every fourth lane position, on two records whose low words decide v against v - 1 and v + 1.  With
    T = v + 1 the kernel's `value >= cur` must refuse h as a win and file it as a candidate: the search is not decided
    until relax(v), stale_wins == 0, the reserve is h.  With R = fffffff800000000 lower hits of the window may be
    filed first: every pair read is a fixture hit of [S, S + F), values never decrease, the sequence ends at h.  (No
    record of this fixture has a lower hit within F of it -- tests/test_reserve_records_cpu.py prints them -- so no
    position puts two in the first window; the rule is asserted all the same.)"""
    h = two_records[which]
    rungs = rr.ladder(h)[1:6]
    assert [r.name for r in rungs] == ["T=max,R=v-1", "T=max,R=old", "T=v+1,R=v", "T=v+1,R=v-1", "T=v+1,R=old"]
    ps = sp.corners(grid) + sp.lane_positions(grid)[::4]
    assert len(ps) == 32
    F = sp.full(grid)
    before = [n for n in rr.lower_in_window(h, F) if n < h]
    both = [h - max(before)] if before else []  # (the lower hit at position 0 and h in the same window)
    t0 = time.monotonic()
    n, failures, deltas = rw.exact_many(gpu_engine, h, ps + both, grid, rungs)
    print(f"grid {grid}, record {h:x} {rr.fixture()[1][h]:016x}: {n} searches {time.monotonic() - t0:.2f} s")
    assert n == 5 * len(ps + both) and failures == [], f"{len(failures)} of {n}: {failures[:6]}"
    assert deltas == ZERO


@pytest.mark.parametrize("where", [(0, 0, 0, 0), (15, -1, 7, 63), (7, 5, 3, 33)])
def test_not_a_candidate(gpu_engine, grid, two_records, where):
    """T = 2^64 - 1, R = v(h) + 1: once the device's `launches` counter has grown by four since before the submit --
    it steps as a launch retires, npow_pool.cpp Worker::retire_launches `account_launch(d_, f.ring);`, in order, at
    most two in flight -- the search's first launch, which hashed h, lies behind, and the host has read no record at
    all: candidates == 0, value == 0.  (The host would drop a wrong record, so `candidates` is the witness.)
    Cancelled with nonces_done above F and below Z, or the run proves nothing.

    The `nonces` counter cannot be the witness: it is credited when a slot retires (Worker::credit_counts,
    `d_.nonces += c.done;`), not per launch, and stood still for 10 s under a search that runs on (measured)."""
    h = two_records[0]
    it, g, wv, lane = where
    pos = sp.pos_of(it, g % grid, wv, lane, grid)
    out = rw.not_a_candidate(gpu_engine, h, pos, grid)
    print(f"not a candidate, {where}: {out}")
    assert out["status"] == _lib.NPOW_CANCELLED
    assert out["F"] < out["nonces_done"] < out["Z"], "inconclusive: the search did not pass h inside the stretch"
    assert out["candidates"] == 0 and out["value"] == 0 and out["nonce"] == 0
    assert out["stale_hits"] == 0 and out["deltas"] == ZERO


# (n, the record's (it, g from the grid's end, wv, lane)); 17 entries are more than kArgEntries: the entry's reserve and
# threshold are then re-read from device memory (None: workgroup 16, entry 16 of 17, the entry past kArgEntries)
COPIES = [(2, (15, 1, 7, 63)), (2, (0, 2, 0, 0)), (17, (9, 17, 2, 1)), (17, (0, None, 5, 62))]


@pytest.mark.parametrize("n,where", COPIES, ids=[f"{n}-{i}" for i, (n, _) in enumerate(COPIES)])
def test_copies_in_one_table(gpu_engine, grid, two_records, n, where):
    """n copies (T = 2^64 - 1, R = v(h)) in one counted launch: each copy hashes the blocks of its own workgroups, so
    exactly one passes h and holds (h, v(h)); every other copy reads value == 0 at that moment; relax(v(h)) answers
    the covering copy with h, and the others are cancelled."""
    h = two_records[0]
    v = rr.fixture()[1][h]
    it, back, wv, lane = where
    g = 16 if back is None else grid - back
    pos = sp.pos_of(it, g, wv, lane, grid)
    assert grid > 2 * 17
    with spw.tuned(gpu_engine):
        out = rw.copies(gpu_engine, h, pos, grid, n, sp.root_of(4000 + n))
    print(f"n {n}, (it, g, wv, lane) {(it, g, wv, lane)}, entry {g % n}: holders {out['holders']}, reserves "
          f"{[(f'{a:x}', f'{b:016x}') for a, b in out['reserves']]}, candidates {out['candidates']}, results "
          f"{out['results']}, deltas {out['deltas']}")
    assert out["deltas"] == ZERO
    assert len(out["holders"]) == 1, "the copy whose workgroups cover h lost it (or two had it)"
    k = out["holders"][0]
    assert [r for i, r in enumerate(out["reserves"]) if i != k] == [(0, 0)] * (n - 1)
    assert out["answered"] is True and out["at_once"] == (_lib.NPOW_OK, h, v)
    assert len(out["results"]) == n
    for i, r in enumerate(out["results"]):
        assert r is not None
        if i == k:
            assert r[:3] == (_lib.NPOW_OK, h, v)
        else:
            assert r[0] == _lib.NPOW_CANCELLED and r[3] < rw.stretch(h, sp.full(grid))


def test_best_so_far_of_one_long_launch(gpu_engine):
    """tests/test_gpu_reserve.py's solo launch -- one launch covers [S, S + 2^34) -- with T = 2^64 - 1 and
    R = fffffff800000000: every reserve read is one of the window's 26 fixture hits with its hashlib value, the sequence
    never decreases and reaches the window's maximum, a927c68ff with ffffffffee3ad8ec (nothing higher follows within
    2^34 nonces of it, so nothing displaces it); candidates stays at or below 26; relax to that value is answered at
    once with a927c68ff.  A record that is never raised after its first store, or a key ordered by the wrong bits,
    ends below the maximum.

    Not asserted: that every read is one of the window's 7 prefix maxima in nonce order
    (reserve_records.running_records).  That holds only if the launch passes its nonces in order, and it does not:
    on an MI355X the reads were 9bb515b4a (2^32.4 nonces from S) and then b67e9f1f7 (2^33.65 from S, and no prefix
    maximum) when the launch had hashed 2^32.9 nonces in all, with the three lower hits before 9bb515b4a never read
    (candidates 2) -- workgroups of one launch drift thousands of wave iterations apart (VALU issue favours the
    oldest wave of a SIMD), so "passed so far" is no prefix of the range.  Which reads were prefix maxima is printed."""
    eng = gpu_engine
    root, hits = rr.fixture()
    window = {n: hits[n] for n in rr.hits_in(rr.SOLO_S, rr.SOLO_S + rr.SOLO_N)}
    run = rr.running_records(rr.SOLO_S, rr.SOLO_N)
    last = max(window, key=window.get)
    assert len(window) == 26 and last == run[-1] and (last, hits[last]) == (0xa927c68ff, 0xffffffffee3ad8ec)
    assert last in rr.records(sp.full(1024), rr.Z34)
    seen, t, ri = [], None, None
    with _Solo(eng):
        try:
            t = eng.submit(root, M64, start=rr.SOLO_S, device_mask=1, reserve=rr.OLD)
            deadline = time.monotonic() + 10
            while time.monotonic() < deadline:
                ri = t.reserve_info()
                if ri.value and (not seen or seen[-1] != (ri.nonce, ri.value)):
                    seen.append((ri.nonce, ri.value))
                if ri.nonce == last or (ri.value and window.get(ri.nonce) != ri.value):
                    break
                time.sleep(0.0005)
            answered = t.relax(hits[last])
            res = t.wait_result(0)
            info = t.wait_info(30)
        finally:
            rw.end(t)
    print(f"one long launch: read {[(f'{n:x}', f'{x:016x}', 'prefix maximum' if n in run else 'no prefix maximum') for n, x in seen]}, "
          f"candidates {ri.candidates}, nonces_done {info.nonces_done}")
    assert seen and all(window.get(n) == x for n, x in seen), "a reserve that is no fixture hit of the window"
    assert [x for _, x in seen] == sorted(x for _, x in seen)
    assert seen[-1] == (last, hits[last])
    assert 1 <= ri.candidates <= 26
    assert answered is True and res is not None and (res.status, res.nonce, res.value) == (_lib.NPOW_OK, last, hits[last])
    assert info.status == _lib.NPOW_OK and info.stale_hits == 0 and info.stale_wins == 0


def test_cu_partitions():
    """The sole-candidate flow on CU partition 1 of 2 alone (device_mask 2: its own grid and F, the search starts at
    S), at the corners and every fourth lane position, in a child process.  A split search is out of scope: device
    1's stride then starts at S + 2^63, outside the fixture's range."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "reserve_exact_worker.py")],
                       env=dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2"), capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"partitions: grids {out['grids']}, record {out['h']}, {out['searches']} searches, {out['seconds']} s")
    assert out["n_devices"] == 2 and out["searches"] == 32 and out["failures"] == []
    assert out["deltas"] == ZERO
