"""Background sweep jobs on the GPU (npow_submit_sweep_background / npow_ticket_sweep): a range's hits enumerated
by claimed chunks of the bounded pool kernel, only while no foreground job wants the device.

Hit-set equality is the statement about the chunk mapping (chunk c = rows [cR, (c+1)R), block row * 8 + wave, the
ragged last block, the prefix a cut launch covered and the remainder it handed back): every nonce hashed exactly
once.  The references are the hashlib-pinned fixtures of tests/golden and the C oracle.  The shapes are the smallest
at which the mapping can go wrong: a wave block is 64 nonces, a row 512, a chunk R * 512 = 8,192, one chunk per
workgroup of the grid 2^23.  The mechanisms (held out, cut by the budget, cut by a yield) are asserted from the
counters of SweepTicket.info(), not from timings; the one timing assertion compares two arms of the same run.
Everything runs on device 0 except the CU-partition test (tests/sweep_background_worker.py).
"""
import functools
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import pytest

import oracle
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


def submit_case(eng, c, background=True, **kw):
    return eng.submit_sweep(bytes.fromhex(c["root"]), int(c["threshold"], 16), int(c["start"], 16), c["count"],
                            device_mask=1, background=background, **kw)


def check_case(res, c):
    assert res is not None and res.status == _lib.NPOW_OK
    assert [f"{h:016x}" for h in res.hits] == c["hits"], c["method"]
    assert res.total == len(c["hits"]) and res.nonces_done == c["count"]


def record(name, **kw):
    """Append a record of what was measured (no assertion depends on it): to NANOPOW_RECORDS_DIR, or bench_out/ in the
    tree, which git ignores."""
    d = os.environ.get("NANOPOW_RECORDS_DIR") or os.path.join(ROOT, "bench_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "sweep_background_records.jsonl"), "a") as f:
        f.write(json.dumps({"test": name, **kw}) + "\n")


# -- 1. fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2])
def test_small_fixtures_and_device_counter(gpu_engine, i):
    c = small_cases()[i]
    gpu_engine.reset_stats(0)
    t = submit_case(gpu_engine, c)
    assert t.info().background
    check_case(t.wait(60), c)
    assert gpu_engine.stats(0).nonces == c["count"]  # a lone job: the device hashed the range and nothing else


def test_2p30_hashlib_fixture(gpu_engine):
    g = big_case()
    t = submit_case(gpu_engine, g, cap=1 << 12)
    while not t.info().finished:
        time.sleep(0.002)
    i = t.info()
    print("2^30 lone background job:", i)
    assert i.nonces_done == g["count"] and i.hits == len(g["hits"]) and i.launches >= 1
    check_case(t.wait(60), g)
    with pytest.raises(_lib.NanoPowError):
        t.info()  # collected


# -- 2. ragged counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0, 0xc000000000000000])
def test_ragged_counts_share_launches(gpu_engine, thr):
    """Every lane a hit, then a quarter of them: counts around a wave block, a row and a chunk, in regions of one
    launch's hit records."""
    ts = [gpu_engine.submit_sweep(ROOT_A, thr, ODD_START, n, device_mask=1, cap=n, background=True) for n in RAGGED]
    for n, t in zip(RAGGED, ts):
        r = t.wait(60)
        want = list(range(ODD_START, ODD_START + n)) if thr == 0 else list(ref(ROOT_A, thr, ODD_START, n))
        assert r is not None and r.status == _lib.NPOW_OK, n
        assert r.hits == want and r.total == len(want), n
        assert r.nonces_done == n, n


# -- 3. launches cut by the time budget -------------------------------------------------------------------
def test_cut_by_the_budget_and_exact(gpu_engine):
    """A 1-ms budget: 2^30 nonces take ~30 ms, so every launch but the last stops claiming with most of its span
    left, and the remainders come back."""
    g = big_case()
    gpu_engine.set_pool_tuning(budget_us=1000)
    try:
        t = submit_case(gpu_engine, g, cap=1 << 12)
        deadline = time.time() + 60
        i = t.info()
        while i.launches_cut < 1 and not i.finished and time.time() < deadline:
            time.sleep(0.0005)
            i = t.info()
        r = t.wait(60)
    finally:
        gpu_engine.set_pool_tuning(budget_us=20000)
    print("budget 1 ms:", i)
    assert i.launches_cut >= 1
    check_case(r, g)


def test_iteration_cap_below_a_chunk(gpu_engine):
    """npow_set_tuning(16, ...) caps a launch at 8 iterations, half a chunk's rows: a launch's span then holds fewer
    chunks than the grid has workgroups, every claim is made at the launch's start (so the 1-ms budget, checked
    before a claim, cuts nothing: launches_cut is printed, not asserted), and the range takes several launches."""
    c = small_cases()[0]
    gpu_engine.set_tuning(16, 0, 0)
    gpu_engine.set_pool_tuning(budget_us=1000)
    try:
        t = submit_case(gpu_engine, c)
        while not t.info().finished:
            time.sleep(0.001)
        i = t.info()
        r = t.wait(60)
    finally:
        gpu_engine.set_tuning(8192, 0, 0)
        gpu_engine.set_pool_tuning(budget_us=20000)
    print("iteration cap 8:", i)
    check_case(r, c)
    assert i.launches >= 3 and i.nonces_done == c["count"]


# -- 4. held out ------------------------------------------------------------------------------------------
def test_held_out_while_a_search_is_live(gpu_engine):
    n = 65537
    tok = _lib.CancelToken()
    search = gpu_engine.submit(bytes([0x77]) * 32, M64, device_mask=1, cancel=tok)
    try:
        job = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, n, device_mask=1, cap=n, background=True)
        assert job.wait(0.3) is None
        i = job.info()
        assert i.nonces_done == 0 and i.launches == 0 and i.hits == 0 and not i.finished
        # a plain sweep job in the same situation is not held
        plain = gpu_engine.submit_sweep(ROOT_A, 0, ODD_START, n, device_mask=1, cap=n)
        rp = plain.wait(30)
        assert rp is not None and rp.status == _lib.NPOW_OK and rp.hits == list(range(ODD_START, ODD_START + n))
        assert job.info().launches == 0  # still held: the plain job was foreground too
    finally:
        tok.set()
    assert search.wait(30).status == _lib.NPOW_CANCELLED
    while not job.info().finished:
        time.sleep(0.001)
    i = job.info()
    print("held out:", i)
    r = job.wait(30)
    assert r is not None and r.status == _lib.NPOW_OK
    assert r.hits == list(range(ODD_START, ODD_START + n)) and r.nonces_done == n
    assert i.held_us > 0 and i.launches >= 1


# -- 5. preempted and still exact ---------------------------------------------------------------------------
def test_preempted_by_searches_and_exact(gpu_engine):
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
        deadline = time.time() + 30
        while not job.info().finished and time.time() < deadline:
            time.sleep(0.005)
        i = job.info()
    finally:
        stop.set()
        th.join(120)
    print("preempted:", i, "searches:", len(found))
    check_case(job.wait(120), g)
    assert found
    for root, r in found:
        assert r is not None and r.status == _lib.NPOW_OK
        assert oracle.work_value_hashlib(root, r.nonce) == r.value >= RECEIVE
    record("preempted", searches=len(found), launches=i.launches, launches_cut=i.launches_cut, held_us=i.held_us)


# -- 6. what a client pays ------------------------------------------------------------------------------------
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


def _check_cancelled(job, start, count, thr):
    i = job.info()
    job.cancel()
    r = job.wait(60)
    assert r is not None and r.status == _lib.NPOW_CANCELLED
    offs = [(h - start) & M64 for h in r.hits]
    assert all(o < count for o in offs) and all(x < y for x, y in zip(offs, offs[1:]))
    step = max(1, len(r.hits) // 64)
    for h in r.hits[::step][:64]:
        assert oracle.work_value_hashlib(ROOT_A, h) >= thr
    assert r.nonces_done < count
    return i


def test_a_search_beside_a_background_job_waits_a_chunk_not_a_launch(gpu_engine):
    """The median time-to-decision of serial searches beside a background job is under a quarter of that beside a
    plain sweep job of the same range, measured in the same run.  The mechanism predicts ~1/50 (a chunk and a launch
    start against half a ~66-ms launch and a half share); the factor 4 leaves room for launch overheads."""
    start, count = 7 << 44, 1 << 35
    arms = {}
    infos = {}
    for arm, bg in (("background", True), ("plain", False)):
        job = gpu_engine.submit_sweep(ROOT_A, AUDIT, start, count, device_mask=1, cap=1 << 20, background=bg)
        deadline = time.time() + 30
        while job.info().nonces_done == 0 and time.time() < deadline:
            time.sleep(0.002)
        assert job.info().nonces_done > 0
        arms[arm] = _searches_beside(gpu_engine, job)
        i = _check_cancelled(job, start, count, AUDIT)
        infos[arm] = {"launches": i.launches, "launches_cut": i.launches_cut, "held_us": i.held_us,
                      "nonces_done": i.nonces_done}
    record("client_cost", decide_us=arms, info=infos)
    print("decide_us:", {k: [round(x) for x in v] for k, v in arms.items()}, infos)
    assert len(arms["background"]) >= 5 and len(arms["plain"]) >= 5, {k: len(v) for k, v in arms.items()}
    mb, mp = statistics.median(arms["background"]), statistics.median(arms["plain"])
    print(f"median decide_us: background {mb:.0f}, plain {mp:.0f}, ratio {mb / mp:.3f}")
    assert mb < mp / 4, (mb, mp)
    assert infos["background"]["launches_cut"] >= 1 and infos["background"]["held_us"] > 0


# -- 7. mixed table --------------------------------------------------------------------------------------------
def test_two_jobs_and_a_background_search_in_one_table(gpu_engine):
    tok = _lib.CancelToken()
    counts = [3 * CHUNK + 65, 65537]
    search = gpu_engine.submit(bytes([0x66]) * 32, M64, device_mask=1, cancel=tok, background=True)
    jobs = [gpu_engine.submit_sweep(ROOT_A, 0, ODD_START + k, n, device_mask=1, cap=n, background=True)
            for k, n in enumerate(counts)]
    try:
        for k, (n, t) in enumerate(zip(counts, jobs)):
            r = t.wait(60)
            assert r is not None and r.status == _lib.NPOW_OK, n
            assert r.hits == list(range(ODD_START + k, ODD_START + k + n)) and r.nonces_done == n, n
    finally:
        tok.set()
    assert search.wait(30).status == _lib.NPOW_CANCELLED


# -- 8. wrong calls --------------------------------------------------------------------------------------------
def test_ticket_calls(gpu_engine):
    import ctypes
    lib = gpu_engine.lib
    bad = _lib.NPOW_ERR_BAD_ARGUMENT
    c = small_cases()[2]
    t = submit_case(gpu_engine, c)
    assert lib.npow_promote(t.ticket, 2) == bad  # no lifting to the foreground
    u32 = ctypes.c_uint32(0)
    assert lib.npow_ticket_background(t.ticket, ctypes.byref(u32)) == bad
    check_case(t.wait(60), c)
    p = submit_case(gpu_engine, c, background=False)
    assert not p.info().background  # a plain job's ticket is looked at too
    check_case(p.wait(60), c)
    s = gpu_engine.submit(ROOT_A, RECEIVE, device_mask=1)
    i = _lib._SweepInfoStruct()
    i.size = ctypes.sizeof(i)
    assert lib.npow_ticket_sweep(s.ticket, ctypes.byref(i)) == bad  # a search's ticket
    assert s.wait(60).status == _lib.NPOW_OK
    assert lib.npow_ticket_sweep(1 << 60, ctypes.byref(i)) == bad  # unknown
    z = gpu_engine.submit_sweep(ROOT_A, 0, 12345, 0, device_mask=1, background=True)
    r = z.wait(0)
    assert r is not None and r.status == _lib.NPOW_OK and r.hits == [] and r.nonces_done == 0


# -- 9. CU partitions --------------------------------------------------------------------------------------------
def test_split_over_two_cu_partitions():
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="2", NANOPOW_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweep_background_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["ok"] and out["devices"] == 2 and out["nonces_done"] == 1 << 24
    checks, failures = out["affinity"]
    assert checks > 0 and failures == 0, out["affinity"]
    assert sum(out["nonces_per_device"]) == 1 << 24 and all(n > 0 for n in out["nonces_per_device"])
