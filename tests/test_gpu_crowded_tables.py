"""Crowded pool tables on the GPU: exact results with 17 to 64 jobs in one launch.

A table of more than 16 entries is uploaded to device memory instead of travelling in the kernel arguments, its
bounded entries have few workgroups each (g % n == e: 16 of a whole MI355X's 1,024 at n = 64, one or two of a 32-CU
partition's 128), the first G % n entries one more than the rest, and its collecting entries share the launch's hit
records in 32 or 64 regions.  These tests compare every result of such a table with the C oracle (oracle.sweep,
oracle.work_values_range; returned values re-checked with hashlib): jobs of one table have distinct roots, so an entry
read from a neighbour's slot or hashed with a neighbour's uniforms gives wrong results; starts are odd, one range of a
table crosses 2^32 and one 2^64, counts are ragged.  The grid is read from the device, never assumed.

Every test proves that its table was crowded (tests/crowded_tables.py tells how the jobs are made to share a launch
and the two proofs: a best job's smallest region, and a pigeonhole on the device's launch counter).  The geometry
itself is walked exhaustively on the CPU in tests/test_dense_cpu.py; the CU-partition cases run in
tests/crowded_tables_worker.py.
"""
import json
import os
import subprocess
import sys

import pytest

import crowded_tables as ct
import oracle
from conftest import ROOT
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64, CAP, QUARTER, RECEIVE = ct.M64, ct.CAP, ct.QUARTER, ct.RECEIVE


# -- a. sweep jobs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,thr", [(17, QUARTER), (33, QUARTER), (63, QUARTER), (64, QUARTER), (64, 0)],
                         ids=["17", "33", "63", "64", "64-every-lane"])
def test_sweep_jobs_exact_in_a_table_of(gpu_engine, n, thr):
    """n collecting entries, one of them a best job whose smallest region shows the launch that held them all.  At
    threshold 0 every hit set is its range, in order."""
    out = ct.sweep_table(gpu_engine, n, thr, seed=100 + n)
    print(json.dumps(dict(out, grid=gpu_engine.stats(0).grid, rem=gpu_engine.stats(0).grid % n)))


# -- b. best jobs -------------------------------------------------------------------------------------------------
def test_64_best_jobs_at_floor_0(gpu_engine):
    """Each result is the oracle's argmax of its own range, first occurrence; four ranges are cut so that the maximum
    is their first nonce, four so that it is their last, in a ragged tail.  Every job's smallest region is a 64th of
    the records, and the initial burst of records at floor 0 stays within it."""
    out = ct.best_table(gpu_engine, seed=200)
    ct.log_records("crowded_64_best", **out)
    print(json.dumps(out))
    assert out["room"] == CAP >> 6 and out["records_max"] <= out["room"]


# -- c. bounded first-win searches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 33, 63])
def test_bounded_searches_exact_in_a_table_of(gpu_engine, n):
    """Three quarters of the searches have the maximum of their range as threshold and must return that nonce -- the
    first nonce, the last one, the first and the last lane of a block in the middle; a quarter have one more and must
    end NPOW_EXHAUSTED with every nonce counted.  The pigeonhole shows a launch of more than 16 entries."""
    out = ct.search_table(gpu_engine, n, seed=300 + n)
    print(json.dumps(out))
    assert out["exhausted"] == n // 4 and out["winners"] == n - n // 4


# -- d. stitching ---------------------------------------------------------------------------------------------------
def test_stitching_in_a_table_of_33(gpu_engine):
    """One wave iteration per launch: 33 sweep jobs of 65,537 nonces take several launches each, in 64 regions."""
    out = ct.stitch_table(gpu_engine, 33, seed=400)
    print(json.dumps(out))


# -- e. every kind ----------------------------------------------------------------------------------------------------
def test_one_table_of_every_kind(gpu_engine):
    """28 dense sweep jobs, a plain best job (the witness), shared and background sweep and best jobs, 8 bounded
    unique-hit searches and 8 unbounded searches at fffffe0000000000: 53 entries, 33 of them collecting in the plain and
    shared classes alone, so the witness's smallest region is a 64th whether or not the background ones are held."""
    eng = gpu_engine
    rs, rng = ct.roots(500, 53)
    rg = ct.ragged_ranges(rng, 37)
    kinds = ["sweep"] * 28 + ["best", "sweep shared", "sweep shared", "best shared", "best shared",
                              "sweep background", "sweep background", "best background", "best background"]
    cuts = [ct.place_cut(rs[37 + k], rng, ct.PLACES[k % 4], [511, 513, 4097, 65537][k // 2 % 4]) for k in range(8)]
    eng.reset_stats(0)
    with ct.held_device(eng):
        ts = []
        for i, kind in enumerate(kinds):
            kw = {"shared": "shared" in kind, "background": "background" in kind}
            if kind.startswith("best"):
                ts.append(eng.submit_best(rs[i], *rg[i], device_mask=1, **kw))
            else:
                ts.append(eng.submit_sweep(rs[i], QUARTER, *rg[i], device_mask=1, cap=rg[i][1], **kw))
        bounded = [eng.submit(rs[37 + k], value, start=start, device_mask=1, max_nonces_per_device=count)
                   for k, (start, count, _, value) in enumerate(cuts)]
        unbounded = [eng.submit(rs[45 + k], RECEIVE, start=rng.getrandbits(64) | 1, device_mask=1) for k in range(8)]
    for i, kind in enumerate(kinds):
        if kind.startswith("best"):
            ct.check_best(ts[i], rs[i], *rg[i], room=CAP >> 6 if kind == "best" else None)
        else:
            ct.check_sweep(ts[i], rs[i], QUARTER, *rg[i])
    for k, (start, count, nonce, value) in enumerate(cuts):
        r = bounded[k].wait(60)
        assert r is not None and r.status == _lib.NPOW_OK and (r.nonce, r.value) == (nonce, value), (r, k)
        assert oracle.work_value_hashlib(rs[37 + k], r.nonce) == r.value
    for k, t in enumerate(unbounded):
        r = t.wait(60)
        assert r is not None and r.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(rs[45 + k], r.nonce) == r.value >= RECEIVE
    st = eng.stats(0)
    assert (st.invalid_work, st.early_mismatches, st.stale_missing) == (0, 0, 0)


# -- f. the claimed map ------------------------------------------------------------------------------------------------
def test_claimed_map_beside_40_weight_8_searches(gpu_engine):
    """Two shared range jobs, a sweep and a best job, in a table dealt by the claimed start map beside 40 searches of
    weight 8 that cannot end: both finish exact while every search is live.  The searches were admitted before the
    device was handed back and leave no table until they are cancelled, so every launch of the range jobs held all
    42 entries; each search has hashed by the end.  (The launch-level witness covers the two range jobs only -- the
    best job's region is half of the records -- since a search leaves no per-launch record to read back.)  The split of
    the workgroups is the subject of tests/test_gpu_range_shared.py and tests/test_weights_cpu.py."""
    eng = gpu_engine
    rs, rng = ct.roots(600, 42)
    (s0, c0), (s1, c1) = ct.ragged_ranges(rng, 2)
    tok = _lib.CancelToken()
    try:
        with ct.held_device(eng):
            searches = [eng.submit(rs[2 + k], M64, start=rng.getrandbits(64) | 1, device_mask=1, cancel=tok, weight=8)
                        for k in range(40)]
            sweep = eng.submit_sweep(rs[0], QUARTER, s0, c0, device_mask=1, cap=c0, shared=True)
            best = eng.submit_best(rs[1], s1, c1, device_mask=1, shared=True)
            assert eng.pool_status() == (0, 42)  # all admitted while the device is held
        ct.until(lambda: sweep.info().finished and best.info().finished, 60)
        shares = [sweep.share(), best.share()]
        assert all(t.wait(0) is None for t in searches)  # live, all 40
        assert eng.pool_status()[1] >= 40
        ct.check_sweep(sweep, rs[0], QUARTER, s0, c0)
        ct.check_best(best, rs[1], s1, c1, room=CAP >> 1)  # the two range jobs shared their launch
        for sh in shares:
            assert sh.klass == _lib.RANGE_SHARED and sh.held_us == 0 and sh.launches >= 1 and sh.moves >= 0, sh
    finally:
        tok.set()
    for t in searches:
        i = t.wait_info(30)
        assert i is not None and i.status == _lib.NPOW_CANCELLED and i.nonces_done > 0
    print(shares)


# -- g. one 32-CU partition ---------------------------------------------------------------------------------------------
def test_on_one_32_cu_partition():
    """G = 128: tables of 17, 48, 63 and 64 entries give an entry 8 / 7, 3 / 2, 3 / 2 and 2 workgroups, the smallest
    counts the mapping can take."""
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="8")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "crowded_tables_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["ok"] and out["grid"] == 128
    assert [r["n"] for r in out["sweeps"]] == [17, 48, 63, 64] == [r["n"] for r in out["searches"]]
    assert out["stitching"]["n"] == 64 and out["stitching"]["launches"] >= 3
