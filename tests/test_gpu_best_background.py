"""Background best jobs on the GPU (npow_submit_best_background / npow_ticket_best_hold): the strongest nonce of a
range, found by claimed chunks of the bounded pool kernel whose waves chase the best value so far, only while no
foreground job wants the device.

An exact maximum is the statement about both halves at once: the chunk mapping (every nonce hashed exactly once: the
result's nonces_done, and the slot's done counts against the claims' prefixes inside the library) and the best branch
under it (the lane mask of a ragged block, a wave's watch carried from chunk to chunk, the records of launches that
were cut).  The references are the C oracle's work values of a 2^22 window (argmax, first occurrence: shared with
tests/test_gpu_best.py, computed once), the hashlib-pinned 2^30 fixture of tests/golden (its maximum is its strongest
hit) and hashlib for every returned value.  The shapes are the smallest at which the two can go wrong together: a
block is 64 nonces, a row 512, a chunk 8,192.  The mechanisms (held out, cut by the budget, cut by a yield) are
asserted from the counters of BestTicket.hold(), not from timings; the one timing assertion compares two arms of the
same run.  Everything runs on device 0 except the CU-partition test (tests/best_background_worker.py).

records_max of every job, and the launches, cuts and held time of the cut-heavy ones, are appended to
bench_out/best_background_records.jsonl; the only assertion on the records is that no launch's entry appended more
than its region holds.
"""
import ctypes
import functools
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import oracle
import test_gpu_best as plain_best  # the shared oracle window: values(), want(), _window()
import test_gpu_ticket_kinds as kinds
from conftest import ROOT, load_golden
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE = 0xfffffe0000000000
ROOT_A, START, N = plain_best.ROOT_A, plain_best.START, plain_best.N
CHUNK = 16 * 512  # kClaimRows rows of 512 nonces (npow_claims.h; tests/test_claims_cpu.py pins it)
RAGGED = [1, 63, 64, 65, 511, 512, 513, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 65, 65537]
values, want = plain_best.values, plain_best.want


@functools.lru_cache(maxsize=None)
def big_case():
    """The 2^30 fixture and its maximum: the hit with the highest hashlib value, the earliest among equal ones."""
    g = load_golden("sweep_2p30_hashlib.json")
    root, start = bytes.fromhex(g["root"]), int(g["start"], 16)
    assert g["count"] == 1 << 30 and len(g["hits"]) == 995 and g["threshold"] == "fffff00000000000"
    best = None
    for h in g["hits"]:
        n = int(h, 16)
        v = oracle.work_value_hashlib(root, n)
        if best is None or v > best[1] or (v == best[1] and (n - start) & M64 < (best[0] - start) & M64):
            best = (n, v)
    return root, int(g["threshold"], 16), start, g["count"], best


def record(name, **kw):
    """Append a record of what was measured (no assertion depends on it): to NANOPOW_RECORDS_DIR, or bench_out/ in the
    tree, which git ignores."""
    d = os.environ.get("NANOPOW_RECORDS_DIR") or os.path.join(ROOT, "bench_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "best_background_records.jsonl"), "a") as f:
        f.write(json.dumps({"test": name, **kw}) + "\n")


def submit(eng, off, count, root=ROOT_A, start=START, **kw):
    return eng.submit_best(root, start + off, count, device_mask=1, background=True, **kw)


def finish(t, name, timeout=60.0, **kw):
    """The job's last looks (npow_ticket_best and npow_ticket_best_hold, once it has finished) and its result."""
    deadline = time.time() + timeout
    info = t.info()
    while not info.finished and time.time() < deadline:
        time.sleep(0.0005)
        info = t.info()
    assert info.finished, info
    hold = t.hold()
    record(name, count=info.count, launches=info.launches, launches_cut=hold.launches_cut, held_us=hold.held_us,
           records=info.records, records_max=info.records_max, room=info.room, **kw)
    assert info.records_max <= info.room or info.launches == 0, info  # never above the region's room
    return t.wait(5), info, hold


def check(res, off, count):
    nonce, value = want(off, count)
    assert res is not None and res.status == _lib.NPOW_OK, res
    assert (res.nonce, res.value, res.nonces_done) == (nonce, value, count), (off, count)
    assert oracle.work_value_hashlib(ROOT_A, res.nonce) == res.value


def check_big(res):
    root, _, _, count, (nonce, value) = big_case()
    assert res is not None and res.status == _lib.NPOW_OK, res
    assert (res.nonce, res.value, res.nonces_done) == (nonce, value, count)
    assert oracle.work_value_hashlib(root, res.nonce) == res.value


# -- 1. ragged counts -----------------------------------------------------------------------------------
def test_ragged_counts_share_one_launch(gpu_engine):
    """Counts around a wave block, a row and a chunk at floor 0, submitted together: regions of one launch's records."""
    ts = [submit(gpu_engine, 0, n) for n in RAGGED]
    for n, t in zip(RAGGED, ts):
        assert t.hold().background == 1
        res, info, hold = finish(t, "ragged")
        check(res, 0, n)
        assert hold.background == 1 and info.records_max <= info.room


# -- 2. the maximum at chunk edges ----------------------------------------------------------------------
def test_maximum_at_chunk_edges_and_just_outside(gpu_engine):
    m = int(np.argmax(values()))
    assert 2 * CHUNK <= m < N - 2 * CHUNK, m  # (the window's argmax is 3,515,448: every case below fits)
    tail = 2 * CHUNK + 70  # a ragged length: its last block holds 6 lanes
    cases = {
        "last lane of a chunk": (m - (2 * CHUNK - 1), 3 * CHUNK + 77),
        "first lane of the next chunk": (m - 2 * CHUNK, 3 * CHUNK + 77),
        "last lane of the ragged tail": (m + 1 - tail, tail),
        "lane 0 of the range": (m, 2 * CHUNK + 65),
        "just excluded at the end": (m - tail, tail),          # [.., m): the runner-up
        "just excluded at the start": (m + 1, 2 * CHUNK + 65),  # (m, ..]
    }
    assert (m - cases["last lane of a chunk"][0]) % CHUNK == CHUNK - 1
    assert (m - cases["first lane of the next chunk"][0]) % CHUNK == 0 and tail % 64 == 6
    ts = {k: submit(gpu_engine, off, n) for k, (off, n) in cases.items()}
    for k, (off, n) in cases.items():
        res, _, _ = finish(ts[k], "edges", case=k)
        check(res, off, n)
        assert (res.nonce == START + m) == (not k.startswith("just excluded")), k


# -- 3. kept and displaced across launches ----------------------------------------------------------------
def test_best_is_kept_and_displaced_across_launches(gpu_engine):
    """One wave iteration per launch (npow_set_tuning(2), as tests/test_gpu_best.py): a lone job of 2.5 to 4 launch
    spans takes 3 or 4 launches.  With the maximum in the first launch's part the early best must survive the later
    launches; with it in the last launch's part it must displace what the earlier ones found."""
    span = gpu_engine.stats(0).grid * 8 * 64  # the nonces one wave iteration of the device covers
    assert 4 * span <= N and span % CHUNK == 0, span
    gpu_engine.set_tuning(2, 0, 0)
    try:
        for last in (False, True):
            off, n = plain_best._window(span, last)
            res, info, _ = finish(submit(gpu_engine, off, n), "stitching_last" if last else "stitching_first")
            check(res, off, n)
            k = (res.nonce - START - off) & M64
            assert (k >= (-(-n // span) - 1) * span) if last else (k < span), (k, span, n)
            assert info.launches >= 3, info
    finally:
        gpu_engine.set_tuning(8192, 0, 0)


# -- 4. cut by the budget -----------------------------------------------------------------------------------
@pytest.mark.parametrize("at_threshold", [False, True])
def test_cut_by_the_budget_and_exact(gpu_engine, at_threshold):
    """A 1-ms budget: 2^30 nonces take ~30 ms, so every launch but the last stops claiming with most of its span
    left, and the remainders come back.  What the cut launches found stays: the looks never go backwards."""
    root, thr, start, count, _ = big_case()
    gpu_engine.set_pool_tuning(budget_us=1000)
    try:
        t = gpu_engine.submit_best(root, start, count, floor=thr if at_threshold else 0, device_mask=1, background=True)
        looks = [t.info()]
        deadline = time.time() + 60
        while not looks[-1].finished and time.time() < deadline:
            time.sleep(0.0005)
            looks.append(t.info())
        res, info, hold = finish(t, "budget_1ms", floor=f"{thr if at_threshold else 0:016x}")
    finally:
        gpu_engine.set_pool_tuning(budget_us=20000)
    print("budget 1 ms:", info, hold)
    assert hold.launches_cut >= 1
    check_big(res)
    assert info.nonces_done == count
    for a, b in zip(looks, looks[1:]):
        assert b.nonces_done >= a.nonces_done and b.value >= a.value, (a, b)
        if at_threshold and b.value:
            assert b.value >= thr


# -- 5. held out ------------------------------------------------------------------------------------------
def test_held_out_while_a_search_is_live(gpu_engine):
    n = 65537
    tok = _lib.CancelToken()
    search = gpu_engine.submit(bytes([0x77]) * 32, M64, device_mask=1, cancel=tok)
    try:
        job = submit(gpu_engine, 0, n)
        assert job.wait(0.3) is None
        i = job.info()
        assert i.nonces_done == 0 and i.launches == 0 and not i.finished
        # a plain best job in the same situation is not held
        res, _, hold = finish(gpu_engine.submit_best(ROOT_A, START, n, device_mask=1), "held_plain", 30)
        check(res, 0, n)
        assert tuple(hold) == (0, 0, 0), hold
        assert job.info().launches == 0  # still held: the plain job was foreground too
    finally:
        tok.set()
    assert search.wait(30).status == _lib.NPOW_CANCELLED
    res, info, hold = finish(job, "held")
    print("held out:", info, hold)
    check(res, 0, n)
    assert hold.held_us > 0 and info.launches >= 1


# -- 6. preempted and still exact ---------------------------------------------------------------------------
def test_preempted_by_searches_and_exact(gpu_engine):
    root, _, start, count, _ = big_case()
    job = gpu_engine.submit_best(root, start, count, device_mask=1, background=True)
    found, stop = [], threading.Event()

    def client():
        k = 0
        while not stop.is_set():
            r_ = bytes([0x50 + (k & 0x3f)]) * 31 + bytes([k >> 6 & 0xff])
            found.append((r_, gpu_engine.submit(r_, RECEIVE, device_mask=1).wait(60)))
            k += 1

    th = threading.Thread(target=client)
    th.start()
    try:
        deadline = time.time() + 30
        while not job.info().finished and time.time() < deadline:
            time.sleep(0.005)
    finally:
        stop.set()
        th.join(120)
    res, info, hold = finish(job, "preempted", 120, searches=len(found))
    print("preempted:", info, hold, "searches:", len(found))
    check_big(res)
    assert found
    for r_, r in found:
        assert r is not None and r.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(r_, r.nonce) == r.value >= RECEIVE


# -- 7. cancel ------------------------------------------------------------------------------------------------
def _check_cancelled(job, start, count, floor, root=ROOT_A):
    job.cancel()
    r = job.wait(60)
    assert r is not None and r.status == _lib.NPOW_CANCELLED
    assert r.nonces_done < count
    if r.nonce is not None:
        assert (r.nonce - start) & M64 < count
        assert oracle.work_value_hashlib(root, r.nonce) == r.value >= floor
    return r


def test_cancel_while_held_and_while_running(gpu_engine):
    count = 1 << 36
    tok = _lib.CancelToken()
    search = gpu_engine.submit(bytes([0x78]) * 32, M64, device_mask=1, cancel=tok)
    try:
        held = submit(gpu_engine, 0, count, floor=RECEIVE)
        assert held.wait(0.05) is None and held.info().launches == 0
        r = _check_cancelled(held, START, count, RECEIVE)
        assert r.nonces_done == 0 and r.nonce is None
    finally:
        tok.set()
    assert search.wait(30).status == _lib.NPOW_CANCELLED
    running = submit(gpu_engine, 0, count, floor=RECEIVE)
    deadline = time.time() + 10
    while running.info().nonces_done == 0 and time.time() < deadline:
        time.sleep(0.001)
    assert running.info().nonces_done > 0
    r = _check_cancelled(running, START, count, RECEIVE)
    assert r.nonces_done > 0
    # the device still serves
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1).wait(60)
    assert s.status == _lib.NPOW_OK and oracle.work_value_hashlib(ROOT_A, s.nonce) == s.value >= RECEIVE


# -- 8. mixed table --------------------------------------------------------------------------------------------
def test_best_job_sweep_job_and_background_search_in_one_table(gpu_engine):
    tok = _lib.CancelToken()
    n_best, off_sweep, n_sweep = 3 * CHUNK + 65, CHUNK - 1, 65537  # overlapping ranges
    search = gpu_engine.submit(bytes([0x66]) * 32, M64, device_mask=1, cancel=tok, background=True)
    try:
        best = submit(gpu_engine, 0, n_best)
        sweep = gpu_engine.submit_sweep(ROOT_A, 0, START + off_sweep, n_sweep, device_mask=1, cap=n_sweep,
                                        background=True)
        res, _, _ = finish(best, "mixed")
        check(res, 0, n_best)
        r = sweep.wait(60)
        assert r is not None and r.status == _lib.NPOW_OK
        assert r.hits == list(range(START + off_sweep, START + off_sweep + n_sweep)) and r.nonces_done == n_sweep
    finally:
        tok.set()
    assert search.wait(30).status == _lib.NPOW_CANCELLED


# -- 9. wrong calls --------------------------------------------------------------------------------------------
def _hold(lib, ticket, size=None):
    h = _lib._BestHoldStruct()
    h.size = ctypes.sizeof(h) if size is None else size
    return lib.npow_ticket_best_hold(ticket, ctypes.byref(h)), h


def test_ticket_calls(gpu_engine):
    lib, bad = gpu_engine.lib, _lib.NPOW_ERR_BAD_ARGUMENT
    golden = load_golden("ticket_kind_errors.json")["kinds"]["best"]
    t = submit(gpu_engine, 0, kinds.N)
    assert lib.npow_promote(t.ticket, 2) == bad  # no lifting to the foreground
    # every call and expected status of the best column, in the order tests/test_gpu_ticket_kinds.py makes them
    c = kinds.Caller(lib, t.ticket)
    for name in kinds.CALLS:
        if name not in kinds.OWN["best"]:
            assert list(c.call(name)) == golden[name], name
            assert golden[name][0] == bad
    assert _hold(lib, t.ticket)[0] == _lib.NPOW_OK  # its own look, also before the job is over
    assert list(kinds._until_finished(c, "npow_ticket_best", c.binfo)) == golden["npow_ticket_best"]
    rc, h = _hold(lib, t.ticket)
    assert rc == _lib.NPOW_OK and h.background == 1 and h.size == 24
    rc, h = _hold(lib, t.ticket, size=8)  # written up to the caller's size
    assert rc == _lib.NPOW_OK and (h.size, h.background, h.launches_cut, h.held_us) == (8, 1, 0, 0)
    assert _hold(lib, t.ticket, size=0)[0] == bad and lib.npow_ticket_best_hold(t.ticket, None) == bad
    for name in ("npow_cancel", "npow_wait_best"):
        assert list(c.call(name, timeout_us=30_000_000)) == golden[name], name
    nonce, value = want(0, kinds.N)
    assert (c.nonce.value, c.value.value, c.done.value) == (nonce, value, kinds.N)
    collected, t.ticket, t.result = t.ticket, 0, object()
    assert _hold(lib, collected)[0] == bad and _hold(lib, 1 << 60)[0] == bad  # collected, unknown
    # a search's and a sweep job's ticket
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
    w = gpu_engine.submit_sweep(ROOT_A, RECEIVE, START, kinds.N, device_mask=1, background=True)
    for other in (s, w):
        assert _hold(lib, other.ticket)[0] == bad
        assert b"npow_ticket_best_hold: the ticket is a s" in lib.npow_last_error()
    assert s.wait(60).status == _lib.NPOW_OK and w.wait(60).status == _lib.NPOW_OK
    # a plain best job reads (0, 0, 0)
    p = gpu_engine.submit_best(ROOT_A, START, kinds.N, device_mask=1)
    assert tuple(p.hold()) == (0, 0, 0)
    res, _, hold = finish(p, "plain")
    assert tuple(hold) == (0, 0, 0)
    check(res, 0, kinds.N)
    with pytest.raises(_lib.NanoPowError):
        p.hold()  # collected
    # count == 0 completes at once
    z = gpu_engine.submit_best(ROOT_A, 12345, 0, device_mask=1, background=True)
    assert tuple(z.hold()) == (1, 0, 0)
    r = z.wait(0)
    assert r is not None and tuple(r) == (_lib.NPOW_EXHAUSTED, None, None, 0)


# -- 10. CU partitions -------------------------------------------------------------------------------------------
def test_split_over_two_cu_partitions():
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2", NANOPOW_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "best_background_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["ok"] and out["devices"] == 2 and out["nonces_done"] == N
    nonce, value = want(0, N)
    assert (int(out["nonce"], 16), int(out["value"], 16)) == (nonce, value)
    checks, failures = out["affinity"]  # the test hooks' device-affinity check of every HIP call site
    assert checks > 0 and failures == 0, out["affinity"]
    assert sum(out["nonces_per_device"]) == N and all(n > 0 for n in out["nonces_per_device"])


# -- 11. what a client pays ------------------------------------------------------------------------------------
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


def test_a_search_beside_a_background_best_job_waits_a_chunk_not_a_launch(gpu_engine):
    """The median time-to-decision of serial searches beside a background best job is under a quarter of that beside a
    plain best job of the same range, measured in the same run: the structure and the bound of
    tests/test_gpu_sweep_background.py's test of the same name for sweep jobs.  The mechanism predicts ~1/50 (a chunk
    and a launch start against half a ~66-ms launch and a half share); the factor 4 leaves room for launch
    overheads."""
    start, count = 7 << 44, 1 << 35
    arms, infos = {}, {}
    for arm, bg in (("background", True), ("plain", False)):
        job = gpu_engine.submit_best(ROOT_A, start, count, device_mask=1, background=bg)
        deadline = time.time() + 30
        while job.info().nonces_done == 0 and time.time() < deadline:
            time.sleep(0.002)
        assert job.info().nonces_done > 0
        arms[arm] = _searches_beside(gpu_engine, job)
        i, h = job.info(), job.hold()
        _check_cancelled(job, start, count, 0)
        infos[arm] = {"launches": i.launches, "launches_cut": h.launches_cut, "held_us": h.held_us,
                      "nonces_done": i.nonces_done, "records_max": i.records_max, "room": i.room}
        assert i.records_max <= i.room
    record("client_cost", decide_us=arms, info=infos)
    print("decide_us:", {k: [round(x) for x in v] for k, v in arms.items()}, infos)
    assert len(arms["background"]) >= 5 and len(arms["plain"]) >= 5, {k: len(v) for k, v in arms.items()}
    mb, mp = statistics.median(arms["background"]), statistics.median(arms["plain"])
    print(f"median decide_us: background {mb:.0f}, plain {mp:.0f}, ratio {mb / mp:.3f}")
    assert mb < mp / 4, (mb, mp)
    assert infos["background"]["launches_cut"] >= 1 and infos["background"]["held_us"] > 0
