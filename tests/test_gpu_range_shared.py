"""Shared range jobs on the GPU (npow_submit_sweep_shared / npow_submit_best_shared / npow_ticket_share): a sweep or
best job that takes a weight-1 share of the device beside the searches, is never held out of a table, and whose
claimed entries take the workgroups that the searches of a launch no longer want.

Hit-set equality and exact maxima are the statements about the chunk mapping under the new dealing (the start map over
a table whose bounded entries are all claimed, workgroups that move to a claimed entry mid-launch, launches cut by a
yield and their remainders): every nonce hashed exactly once.  The references are the hashlib-pinned fixtures of
tests/golden, the C oracle and the oracle window tests/test_gpu_best.py shares.  The mechanisms (never held, cut,
moved, not starved) are asserted from the counters of info() and share(), not from timings; the share test applies
the bands of tests/test_gpu_weights.py, and the one latency assertion compares two arms of the same run.  Everything
runs on device 0 except the CU-partition test (tests/range_shared_worker.py).  "Unending search" is a search at
threshold ffffffffffffffff with a cancel token, cancelled in a `finally`.

What was measured (ratios, medians, moves) is appended to bench_out/range_shared_records.jsonl; no assertion reads it.
"""
import contextlib
import ctypes
import functools
import json
import math
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import oracle
import test_gpu_best as plain_best  # the shared oracle window: values(), want()
import test_gpu_ticket_kinds as kinds
from conftest import ROOT, load_golden
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE, AUDIT = 0xfffffe0000000000, 0xffff000000000000
ROOT_A = bytes(range(3, 35))
ODD_START = 0x0123456789abcdef
R = 16  # kClaimRows (npow_claims.h; tests/test_claims_cpu.py pins it)
CHUNK = R * 512
RAGGED = [1, 63, 64, 65, 511, 512, 513, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 65, 65537]
START, N = plain_best.START, plain_best.N
values, want = plain_best.values, plain_best.want
SHARED, BACKGROUND, PLAIN = _lib.RANGE_SHARED, _lib.RANGE_BACKGROUND, _lib.RANGE_PLAIN


@functools.lru_cache(maxsize=None)
def ref(root, threshold, start, count):
    """oracle.sweep, computed once per range and shared (a tuple: nobody changes it)."""
    return tuple(oracle.sweep(root, threshold, start, count, threads=min(16, os.cpu_count() or 1)))


@functools.lru_cache(maxsize=None)
def small_cases():
    cases = load_golden("sweeps_small.json")["cases"][-3:]
    assert [c["count"] for c in cases] == [1 << 24, 1 << 24, 1 << 23] and cases[2]["start"] == "ffffffffffc00000"
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def big_case():
    return load_golden("sweep_2p30_hashlib.json")


def submit_case(eng, c, **kw):
    return eng.submit_sweep(bytes.fromhex(c["root"]), int(c["threshold"], 16), int(c["start"], 16), c["count"],
                            device_mask=1, shared=True, **kw)


def check_case(res, c):
    assert res is not None and res.status == _lib.NPOW_OK
    assert [f"{h:016x}" for h in res.hits] == c["hits"], c["method"]
    assert res.total == len(c["hits"]) and res.nonces_done == c["count"]


def record(name, **kw):
    """Append a record of what was measured (no assertion depends on it): to NANOPOW_RECORDS_DIR, or bench_out/ in the
    tree, which git ignores."""
    d = os.environ.get("NANOPOW_RECORDS_DIR") or os.path.join(ROOT, "bench_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "range_shared_records.jsonl"), "a") as f:
        f.write(json.dumps({"test": name, **kw}) + "\n")


@contextlib.contextmanager
def unending_search(eng, weight=1, fill=0x77, **kw):
    tok = _lib.CancelToken()
    search = eng.submit(bytes([fill]) * 32, M64, device_mask=1, cancel=tok, weight=weight, **kw)
    try:
        yield search, tok
    finally:
        tok.set()
        if search.result is None:
            assert search.wait(30).status == _lib.NPOW_CANCELLED


def until(cond, timeout=30.0, nap=0.0005):
    deadline = time.time() + timeout
    while not cond():
        assert time.time() < deadline, "timed out"
        time.sleep(nap)


def last_looks(t, timeout=60.0):
    """The job's info() and share() once it has finished, before its ticket is collected."""
    until(lambda: t.info().finished, timeout)
    return t.info(), t.share()


# -- 1. fixtures, alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2])
def test_small_fixtures_alone(gpu_engine, i):
    c = small_cases()[i]
    gpu_engine.reset_stats(0)
    t = submit_case(gpu_engine, c)
    assert t.share().klass == SHARED and not t.info().background
    info, share = last_looks(t)
    check_case(t.wait(60), c)
    assert share.klass == SHARED and share.held_us == 0 and info.held_us == 0 and share.launches >= 1
    assert gpu_engine.stats(0).nonces == c["count"]  # a lone job: the device hashed the range and nothing else


# -- 2. ragged counts in a map-dealt table ----------------------------------------------------------------
@pytest.mark.parametrize("thr", [0, 0xc000000000000000])
def test_ragged_counts_beside_a_weight_8_search(gpu_engine, thr):
    """Every lane a hit, then a quarter of them: counts around a wave block, a row and a chunk, each job a claimed
    entry of weight 1 in a table whose search weighs 8 -- dealt by the start map."""
    with unending_search(gpu_engine, weight=8):
        ts = [gpu_engine.submit_sweep(ROOT_A, thr, ODD_START, n, device_mask=1, cap=n, shared=True) for n in RAGGED]
        for n, t in zip(RAGGED, ts):
            r = t.wait(60)
            want_hits = list(range(ODD_START, ODD_START + n)) if thr == 0 else list(ref(ROOT_A, thr, ODD_START, n))
            assert r is not None and r.status == _lib.NPOW_OK, n
            assert r.hits == want_hits and r.total == len(want_hits), n
            assert r.nonces_done == n, n


# -- 3. not starved ---------------------------------------------------------------------------------------
def test_not_starved_by_a_live_search(gpu_engine):
    n = 65537
    with unending_search(gpu_engine) as (search, _):
        # the premise: a background job in this situation makes no progress
        bg = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, n, device_mask=1, cap=n, background=True)
        assert bg.wait(0.3) is None
        assert bg.info().nonces_done == 0
        job = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, n, device_mask=1, cap=n, shared=True)
        info, share = last_looks(job, 30)
        r = job.wait(30)
        assert search.wait(0) is None  # the search is still live
        assert r is not None and r.status == _lib.NPOW_OK
        assert r.hits == list(range(ODD_START, ODD_START + n)) and r.nonces_done == n
        assert share.klass == SHARED and share.held_us == 0 and info.held_us == 0
        assert bg.info().nonces_done == 0 and bg.share().klass == BACKGROUND  # still held: the search is foreground
    rb = bg.wait(30)
    assert rb is not None and rb.status == _lib.NPOW_OK and rb.nonces_done == n


# -- 4. shares ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [8, 1])
def test_share_beside_a_search_follows_the_weights(gpu_engine, weight):
    """An unending search of weight W beside a shared job (weight 1) for 0.5 s: the ratio of their nonces lies in
    (W / sqrt 2, W * sqrt 2), the band tests/test_gpu_weights.py applies to two searches."""
    start, count = 7 << 44, 1 << 35
    with unending_search(gpu_engine, weight=weight) as (search, tok):
        job = gpu_engine.submit_sweep(ROOT_A, AUDIT, start, count, device_mask=1, cap=1 << 20, shared=True)
        try:
            time.sleep(0.5)
            job_n = job.info().nonces_done
            tok.set()
            s = search.wait_info(30)
            assert s is not None and s.status == _lib.NPOW_CANCELLED
            search_n = s.nonces_done
            share = job.share()
        finally:
            job.cancel()
            r = job.wait(60)
    assert r is not None and r.status == _lib.NPOW_CANCELLED
    ratio = search_n / max(job_n, 1)
    record("shares", weight=weight, search_nonces=search_n, job_nonces=job_n, ratio=ratio, moves=share.moves,
           launches=share.launches, launches_cut=share.launches_cut)
    print(f"weight {weight}: search {search_n} / job {job_n} nonces, ratio {ratio:.3f}, {share}")
    assert job_n > 0 and share.held_us == 0
    assert weight / math.sqrt(2) < ratio < weight * math.sqrt(2), f"weight {weight}: ratio {ratio:.3f}"


# -- 5. freed workgroups move ---------------------------------------------------------------------------------
def test_workgroups_of_a_cancelled_search_move_to_the_job(gpu_engine):
    start, count = 9 << 44, 1 << 35
    gpu_engine.set_pool_tuning(budget_us=200000)
    try:
        job = gpu_engine.submit_sweep(ROOT_A, AUDIT, start, count, device_mask=1, cap=1 << 20, shared=True)
        try:
            rounds = []
            for k in range(3):  # (a cancel that lands in a launch's last moments moves nothing: again, a new search)
                with unending_search(gpu_engine, weight=8, fill=0x71 + k):
                    done0 = job.info().nonces_done
                    until(lambda: job.info().nonces_done > done0)
                launches = job.share().launches  # (the search is cancelled and collected here)
                until(lambda: job.share().launches > launches + 1)
                rounds.append(job.share().moves)
                if rounds[-1] > 0:
                    break
            share = job.share()
        finally:
            job.cancel()
            r = job.wait(60)
    finally:
        gpu_engine.set_pool_tuning(budget_us=20000)
    record("moves", rounds=rounds, launches=share.launches, launches_cut=share.launches_cut)
    print("moves after each round:", rounds, share)
    assert share.moves > 0 and share.held_us == 0
    assert r is not None and r.status == _lib.NPOW_CANCELLED
    offs = [(h - start) & M64 for h in r.hits]
    assert all(o < count for o in offs) and all(x < y for x, y in zip(offs, offs[1:]))
    step = max(1, len(r.hits) // 64)
    for h in r.hits[::step][:64]:
        assert oracle.work_value_hashlib(ROOT_A, h) >= AUDIT


# -- 6. exact through cuts and moves ---------------------------------------------------------------------------
def test_exact_beside_serial_searches(gpu_engine):
    g = big_case()
    job = submit_case(gpu_engine, g, cap=1 << 12)
    found, stop = [], threading.Event()

    def client():
        k = 0
        while not stop.is_set():
            root = bytes([0x50 + (k & 0x3f)]) * 31 + bytes([k >> 6 & 0xff])
            r = gpu_engine.submit(root, RECEIVE, device_mask=1).wait(60)
            found.append((root, r))
            k += 1

    th = threading.Thread(target=client)
    th.start()
    try:
        i, share = last_looks(job, 30)
    finally:
        stop.set()
        th.join(120)
    print("beside serial searches:", i, share, "searches:", len(found))
    check_case(job.wait(120), g)
    assert share.launches_cut >= 1 and share.held_us == 0
    assert found
    for root, r in found:
        assert r is not None and r.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(root, r.nonce) == r.value >= RECEIVE
    record("serial_searches", searches=len(found), moves=share.moves, launches=share.launches,
           launches_cut=share.launches_cut)


# -- 7. what a client pays ------------------------------------------------------------------------------------
def _searches_beside(eng, job, n=12):
    """decide_us of n serial receive-difficulty searches, those after which the job is still pending."""
    out = []
    for k in range(n):
        root = bytes([0x21 + k]) * 32
        info = eng.submit(root, RECEIVE, device_mask=1).wait_info(60)
        assert info is not None and info.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(root, info.nonce) == info.value >= RECEIVE
        if not job.info().finished:
            out.append(info.decide_us)
    return out


def test_a_search_beside_a_shared_job_waits_a_chunk_not_a_launch(gpu_engine):
    """The median time-to-decision of serial searches beside a shared job is under a quarter of that beside a plain
    sweep job of the same range, measured in the same run: the form and the factor of
    tests/test_gpu_sweep_background.py's test for the background class.  The mechanism predicts a chunk, a launch
    start and a half share against half a ~66-ms launch."""
    start, count = 7 << 44, 1 << 35
    arms, infos = {}, {}
    for arm, shared in (("shared", True), ("plain", False)):
        job = gpu_engine.submit_sweep(ROOT_A, AUDIT, start, count, device_mask=1, cap=1 << 20, shared=shared)
        try:
            until(lambda: job.info().nonces_done > 0)
            arms[arm] = _searches_beside(gpu_engine, job)
            s, i = job.share(), job.info()
            infos[arm] = {"klass": s.klass, "launches": s.launches, "launches_cut": s.launches_cut,
                          "held_us": s.held_us, "moves": s.moves, "nonces_done": i.nonces_done}
        finally:
            job.cancel()
            r = job.wait(60)
        assert r is not None and r.status == _lib.NPOW_CANCELLED and r.nonces_done < count
    record("client_cost", decide_us=arms, info=infos)
    print("decide_us:", {k: [round(x) for x in v] for k, v in arms.items()}, infos)
    assert len(arms["shared"]) >= 5 and len(arms["plain"]) >= 5, {k: len(v) for k, v in arms.items()}
    ms, mp = statistics.median(arms["shared"]), statistics.median(arms["plain"])
    print(f"median decide_us: shared {ms:.0f}, plain {mp:.0f}, ratio {ms / mp:.3f}")
    assert ms < mp / 4, (ms, mp)
    assert infos["shared"]["klass"] == SHARED and infos["plain"]["klass"] == PLAIN
    assert infos["shared"]["launches_cut"] >= 1 and infos["shared"]["held_us"] == 0


# -- 8. best jobs -----------------------------------------------------------------------------------------------
def _best(eng, off, count, **kw):
    return eng.submit_best(ROOT_A, START + off, count, device_mask=1, shared=True, **kw)


def _check_best(res, off, count):
    nonce, value = want(off, count)  # argmax, first occurrence: the smallest nonce - start among equal values
    assert res is not None and res.status == _lib.NPOW_OK, res
    assert (res.nonce, res.value, res.nonces_done) == (nonce, value, count), (off, count)
    assert oracle.work_value_hashlib(ROOT_A, res.nonce) == res.value


def _best_cases():
    m = int(np.argmax(values()))
    assert 2 * CHUNK <= m < N - 2 * CHUNK, m
    tail = 2 * CHUNK + 70  # a ragged length: its last block holds 6 lanes
    cases = {f"ragged {n}": (0, n) for n in RAGGED}
    cases.update({
        "last lane of a chunk": (m - (2 * CHUNK - 1), 3 * CHUNK + 77),
        "first lane of the next chunk": (m - 2 * CHUNK, 3 * CHUNK + 77),
        "last lane of the ragged tail": (m + 1 - tail, tail),
        "lane 0 of the range": (m, 2 * CHUNK + 65),
        "just excluded at the end": (m - tail, tail),
        "just excluded at the start": (m + 1, 2 * CHUNK + 65),
    })
    return m, cases


@pytest.mark.parametrize("beside", [False, True])
def test_best_jobs_alone_and_beside_a_weight_8_search(gpu_engine, beside):
    m, cases = _best_cases()
    with (unending_search(gpu_engine, weight=8) if beside else contextlib.nullcontext()):
        ts = {k: _best(gpu_engine, off, n) for k, (off, n) in cases.items()}
        whole = _best(gpu_engine, 0, N)
        looks = [whole.info()]
        deadline = time.time() + 60
        while not looks[-1].finished and time.time() < deadline:  # npow_ticket_best mid-run
            time.sleep(0.0005)
            looks.append(whole.info())
        for k, (off, n) in cases.items():
            assert ts[k].share().klass == SHARED and ts[k].hold().background == 0
            info, share = last_looks(ts[k])
            assert info.records_max <= info.room and share.held_us == 0
            res = ts[k].wait(5)
            _check_best(res, off, n)
            if not k.startswith("ragged"):
                assert (res.nonce == START + m) == (not k.startswith("just excluded")), k
        for a, b in zip(looks, looks[1:]):
            assert b.nonces_done >= a.nonces_done and b.value >= a.value, (a, b)
        _check_best(whole.wait(30), 0, N)
        # the floor: at the maximum, and above it
        n = 65537
        nonce, value = want(0, n)
        assert tuple(_best(gpu_engine, 0, n, floor=value).wait(60)) == (_lib.NPOW_OK, nonce, value, n)
        assert tuple(_best(gpu_engine, 0, n, floor=value + 1).wait(60)) == (_lib.NPOW_EXHAUSTED, None, None, n)


# -- 9. mixed table --------------------------------------------------------------------------------------------
def test_both_classes_and_searches_in_one_table(gpu_engine):
    g = big_case()
    n_bg = 65537
    with unending_search(gpu_engine, fill=0x66, background=True):
        sweep = submit_case(gpu_engine, g, cap=1 << 12)
        best = _best(gpu_engine, 0, N)
        bg = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, n_bg, device_mask=1, cap=n_bg, background=True)
        fg = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
        s = fg.wait(60)
        assert s is not None and s.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(ROOT_A, s.nonce) == s.value >= RECEIVE
        # the background job is not starved by the shared ones: it is launched while they are pending
        until(lambda: bg.info().launches >= 1)
        assert not sweep.info().finished
        rb = bg.wait(60)
        assert rb is not None and rb.status == _lib.NPOW_OK
        assert rb.hits == list(range(ODD_START, ODD_START + n_bg)) and rb.nonces_done == n_bg
        _, share = last_looks(sweep)
        check_case(sweep.wait(60), g)
        assert share.klass == SHARED and share.held_us == 0
        _check_best(best.wait(60), 0, N)


# -- 10. ticket calls ------------------------------------------------------------------------------------------
def _share(lib, ticket, size=None):
    s = _lib._RangeShareStruct()
    s.size = ctypes.sizeof(s) if size is None else size
    return lib.npow_ticket_share(ticket, ctypes.byref(s)), s


@pytest.mark.parametrize("kind", ["sweep", "best"])
def test_ticket_calls(gpu_engine, kind):
    lib, bad = gpu_engine.lib, _lib.NPOW_ERR_BAD_ARGUMENT
    golden = load_golden("ticket_kind_errors.json")["kinds"][kind]
    if kind == "sweep":
        t = gpu_engine.submit_sweep(ROOT_A, RECEIVE, START, kinds.N, device_mask=1, cap=kinds.N, shared=True)
    else:
        t = gpu_engine.submit_best(ROOT_A, START, kinds.N, device_mask=1, shared=True)
    c = kinds.Caller(lib, t.ticket)
    # every call of another kind refuses the ticket as it refuses the plain job's, and leaves it collectable
    for name in kinds.CALLS:
        if name not in kinds.OWN[kind]:
            assert list(c.call(name)) == golden[name], name
            assert golden[name][0] == bad
    rc, s = _share(lib, t.ticket)
    assert rc == _lib.NPOW_OK and s.klass == SHARED and s.size == 40 and s.held_us == 0
    rc, s = _share(lib, t.ticket, size=8)  # written up to the caller's size
    assert rc == _lib.NPOW_OK and (s.size, s.klass, s.launches, s.moves) == (8, SHARED, 0, 0)
    assert _share(lib, t.ticket, size=0)[0] == bad and lib.npow_ticket_share(t.ticket, None) == bad
    if kind == "sweep":
        assert list(kinds._until_finished(c, "npow_ticket_sweep", c.sinfo)) == golden["npow_ticket_sweep"]
        assert c.sinfo.background == 0 and c.sinfo.held_us == 0
        assert list(c.call("npow_wait_sweep", timeout_us=30_000_000)) == golden["npow_wait_sweep"]
        got = list(c.hits[:c.n.value])
        assert got == list(ref(ROOT_A, RECEIVE, START, kinds.N)) and c.done.value == kinds.N
    else:
        h = _lib._BestHoldStruct()
        h.size = ctypes.sizeof(h)
        assert lib.npow_ticket_best_hold(t.ticket, ctypes.byref(h)) == _lib.NPOW_OK
        assert (h.background, h.held_us) == (0, 0)  # the class is reported by npow_ticket_share alone
        assert list(kinds._until_finished(c, "npow_ticket_best", c.binfo)) == golden["npow_ticket_best"]
        assert list(c.call("npow_wait_best", timeout_us=30_000_000)) == golden["npow_wait_best"]
        nonce, value = want(0, kinds.N)
        assert (c.nonce.value, c.value.value, c.done.value) == (nonce, value, kinds.N)
    collected, t.ticket, t.result = t.ticket, 0, object()
    assert _share(lib, collected)[0] == bad and _share(lib, 1 << 60)[0] == bad  # collected, unknown


def test_ticket_share_tells_the_other_classes(gpu_engine):
    lib, bad = gpu_engine.lib, _lib.NPOW_ERR_BAD_ARGUMENT
    n = kinds.N
    jobs = {
        ("sweep", PLAIN): gpu_engine.submit_sweep(ROOT_A, RECEIVE, START, n, device_mask=1, cap=n),
        ("sweep", BACKGROUND): gpu_engine.submit_sweep(ROOT_A, RECEIVE, START, n, device_mask=1, cap=n,
                                                       background=True),
        ("best", PLAIN): gpu_engine.submit_best(ROOT_A, START, n, device_mask=1),
        ("best", BACKGROUND): gpu_engine.submit_best(ROOT_A, START, n, device_mask=1, background=True),
    }
    for (kind, klass), t in jobs.items():
        assert t.share().klass == klass, (kind, klass)
        _, share = last_looks(t)
        assert (share.klass, share.moves) == (klass, 0) and share.launches >= 1, (kind, klass, share)
        r = t.wait(30)
        if kind == "sweep":
            assert r.status == _lib.NPOW_OK and r.hits == list(ref(ROOT_A, RECEIVE, START, n))
        else:
            _check_best(r, 0, n)
        with pytest.raises(_lib.NanoPowError):
            t.share()  # collected
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
    assert _share(lib, s.ticket)[0] == bad  # a search's ticket
    assert b"npow_ticket_share: the ticket is a search's" in lib.npow_last_error()
    assert s.wait(60).status == _lib.NPOW_OK
    # count == 0 completes at once and touches no device
    z = gpu_engine.submit_sweep(ROOT_A, 0, 12345, 0, device_mask=1, shared=True)
    assert z.share().klass == SHARED
    r = z.wait(0)
    assert r is not None and r.status == _lib.NPOW_OK and r.hits == [] and r.nonces_done == 0
    zb = gpu_engine.submit_best(ROOT_A, 12345, 0, device_mask=1, shared=True)
    assert tuple(zb.wait(0)) == (_lib.NPOW_EXHAUSTED, None, None, 0)
    with pytest.raises(ValueError):
        gpu_engine.submit_sweep(ROOT_A, 0, 0, 64, device_mask=1, shared=True, background=True)


# -- 11. CU partitions --------------------------------------------------------------------------------------------
def test_split_over_two_cu_partitions():
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2", NANOPOW_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "range_shared_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["ok"] and out["devices"] == 2 and out["nonces_done"] == 1 << 24
    checks, failures = out["affinity"]
    assert checks > 0 and failures == 0, out["affinity"]
    assert all(n > 0 for n in out["nonces_per_device"])
