"""Background searches (npow_submit_background): a class of search that hashes only on the workgroups no foreground
search of its launch wants, and gets them back when the foreground searches end -- inside the running launch, with no
yield and no new launch.  Every test but the last runs on device 0 only.  Run on an MI355X: ``pytest -m gpu``.

The idioms are tests/test_gpu_promote.py's: a blocker under pool_config(1) so that the jobs queued behind it are
admitted together and share one counted launch; budget_us=400000 and set_tuning(65536) so that this launch outlasts
the test; threshold 2^64 - 1 so that a search ends only by its cancel; every setting restored in ``finally``.
"""
import contextlib
import ctypes
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


def _sleep_until(t):
    time.sleep(max(0.0, t - time.monotonic()))


class _Jobs:
    """Endless searches on device 0, each with a cancel token and a nonce region of its own."""

    def __init__(self, eng, seed):
        self.eng, self.roots, self.toks, self.tickets = eng, _roots(seed, 16), [], []

    def submit(self, background=False, threshold=M64, mask=1):
        i = len(self.tickets)
        self.toks.append(_lib.CancelToken())
        self.tickets.append(self.eng.submit(self.roots[i], threshold, start=(i + 1) << 52, device_mask=mask,
                                            cancel=self.toks[i], background=background))
        return self.tickets[-1]

    def cancel_all(self):
        for c in self.toks:
            c.set()

    def end(self):
        """Cancel and collect whatever a test that failed half-way left behind: no endless search outlives it."""
        self.cancel_all()
        for t in self.tickets:
            if t.result is None:
                t.wait(30)


@contextlib.contextmanager
def _one_long_launch(eng, jobs):
    """The tunings under which one launch outlasts a test, restored afterwards; the test's searches ended."""
    eng.set_pool_tuning(budget_us=400000)  # one launch lasts past the test: ...
    eng.set_tuning(65536)                  # ... 32,768 wave iterations, ~0.4 s
    try:
        yield
    finally:
        eng.pool_config(64)
        jobs.end()
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)


def _admit_together(eng, jobs, classes):
    """Queue one job per entry of `classes` (True: background) behind a blocker under max_active 1, admit them
    together, end the blocker.  Returns the time the blocker was gone."""
    eng.pool_config(1)
    blocker = jobs.submit()
    for bg in classes:
        jobs.submit(background=bg)
    assert eng.pool_status() == (len(classes), 1)
    eng.pool_config(64)  # admitted, and adopted, together
    jobs.toks[0].set()
    assert blocker.wait(30).status == _lib.NPOW_CANCELLED
    return time.monotonic()


def _same_launch(s0, s1):
    return (s1.yields, s1.launches) == (s0.yields, s0.launches)


def test_dynamic_background_entries_get_nothing(gpu_engine):
    """Foreground C and D run in a counted launch; background A and B join it 5 ms in as dynamic entries and are
    parked.  A + B <= 1 % of C + D in nonces: nominal 0; equal shares would give 1.0 and weights 8 : 1 0.125, so
    1 % tells the class from any weight."""
    eng, jobs = gpu_engine, _Jobs(gpu_engine, 91)
    with _one_long_launch(eng, jobs):
        t0 = _admit_together(eng, jobs, [False, False])
        _sleep_until(t0 + 0.005)
        s0 = eng.stats(0)
        jobs.submit(background=True)
        jobs.submit(background=True)
        _sleep_until(t0 + 0.1)
        s1 = eng.stats(0)
        jobs.cancel_all()
        dc, dd, da, db = (t.wait(30).nonces_done for t in jobs.tickets[1:])
    print(f"dynamic background: C {dc} D {dd} A {da} B {db}, (A + B) / (C + D) = {(da + db) / max(dc + dd, 1):.5f}; "
          f"dyn_entries {s0.dyn_entries} -> {s1.dyn_entries}, yields {s0.yields} -> {s1.yields}, launches "
          f"{s0.launches} -> {s1.launches}")
    assert s1.dyn_entries > s0.dyn_entries, "A and B did not join the running launch"
    assert _same_launch(s0, s1), "the launch was ended"
    assert dc > 0 and dd > 0
    assert da + db <= 0.01 * (dc + dd)


@pytest.mark.parametrize("n_bg,n_fg", [(1, 1), (3, 2)])
def test_table_start(gpu_engine, n_bg, n_fg):
    """Background and foreground jobs admitted together: the start map gives the background entries no workgroup
    (with two equal-weight foreground entries: the wsum rule).  Cancelled at 50 ms; A <= 1 % of C."""
    eng, jobs = gpu_engine, _Jobs(gpu_engine, 92 + n_bg)
    with _one_long_launch(eng, jobs):
        t0 = _admit_together(eng, jobs, [True] * n_bg + [False] * n_fg)
        _sleep_until(t0 + 0.05)
        jobs.cancel_all()
        done = [t.wait(30).nonces_done for t in jobs.tickets[1:]]
    a, c = sum(done[:n_bg]), sum(done[n_bg:])
    print(f"table start, {n_bg} background beside {n_fg} foreground: {done}, A / C = {a / max(c, 1):.5f}")
    assert all(d > 0 for d in done[n_bg:])
    assert a <= 0.01 * c


def test_yield_and_return_in_place(gpu_engine):
    """Background A and B share a counted launch; foreground C joins it at 20 ms and is cancelled at 60 ms; A and B
    are cancelled at 160 ms.  Nominal (A + B) / C = 120 / 40 = 3; 0.5 if the background never got the device back, 7
    if C held only half of it: the bounds are the geometric means, sqrt(0.5 * 3) and sqrt(3 * 7)."""
    eng, jobs = gpu_engine, _Jobs(gpu_engine, 95)
    with _one_long_launch(eng, jobs):
        t0 = _admit_together(eng, jobs, [True, True])
        _sleep_until(t0 + 0.01)  # (A and B's launch is running)
        s0 = eng.stats(0)
        _sleep_until(t0 + 0.02)
        tc = jobs.submit()
        _sleep_until(t0 + 0.06)
        jobs.toks[3].set()
        dc = tc.wait(30).nonces_done
        _sleep_until(t0 + 0.16)
        s1 = eng.stats(0)
        jobs.cancel_all()
        da, db = (t.wait(30).nonces_done for t in jobs.tickets[1:3])
    ratio = (da + db) / max(dc, 1)
    print(f"yield and return: A {da} B {db} C {dc}, (A + B) / C = {ratio:.3f}; dyn_entries {s0.dyn_entries} -> "
          f"{s1.dyn_entries}, yields {s0.yields} -> {s1.yields}, launches {s0.launches} -> {s1.launches}")
    assert s1.dyn_entries > s0.dyn_entries, "C did not join the running launch"
    assert _same_launch(s0, s1), "a launch ended or another search restarted"
    assert math.sqrt(0.5 * 3) < ratio < math.sqrt(3 * 7), f"(A + B) / C = {ratio:.3f}"


def test_promotion_lifts(gpu_engine):
    """Background A, B and C share one launch; C is promoted to weight 1 at 20 ms; all are cancelled at 120 ms.
    Nominal (A + B) / C = 0.125, unlifted 2.0: the bound is their geometric mean, 0.5."""
    eng, jobs = gpu_engine, _Jobs(gpu_engine, 96)
    with _one_long_launch(eng, jobs):
        t0 = _admit_together(eng, jobs, [True, True, True])
        _sleep_until(t0 + 0.02)
        s0 = eng.stats(0)
        jobs.tickets[3].promote(1)
        _sleep_until(t0 + 0.12)
        s1 = eng.stats(0)
        jobs.cancel_all()
        da, db, dc = (t.wait(30).nonces_done for t in jobs.tickets[1:])
    ratio = (da + db) / max(dc, 1)
    print(f"promotion lifts: A {da} B {db} C {dc}, (A + B) / C = {ratio:.3f}; promotions {s0.promotions} -> "
          f"{s1.promotions}, yields {s0.yields} -> {s1.yields}, launches {s0.launches} -> {s1.launches}")
    assert s1.promotions == s0.promotions + 1
    assert _same_launch(s0, s1), "the launch was ended for the promotion"
    assert ratio < 0.5, f"(A + B) / C = {ratio:.3f}"


def test_background_alone_is_the_pool_as_before(gpu_engine):
    """Two background jobs for 200 ms: equal shares, within the bound of the (1, 1) weights test."""
    eng, jobs = gpu_engine, _Jobs(gpu_engine, 97)
    try:
        jobs.submit(background=True)
        jobs.submit(background=True)
        time.sleep(0.2)
        jobs.cancel_all()
        da, db = (t.wait(30).nonces_done for t in jobs.tickets)
    finally:
        jobs.end()
    r = db / max(da, 1)
    print(f"two background jobs alone: nonces {da} / {db}, ratio {r:.3f}")
    assert 1 / math.sqrt(2) < r < math.sqrt(2), f"ratio {r:.3f} ({da} / {db} nonces)"


def test_foreground_is_admitted_first(gpu_engine):
    """max_active 1: behind a running job wait a background job and then a foreground one; the foreground one is
    adopted first when the running one ends."""
    eng = gpu_engine
    eng.pool_config(1)
    tok = _lib.CancelToken()
    try:
        r0, r1, r2 = _roots(98, 3)
        first = eng.submit(r0, M64, device_mask=1, cancel=tok)
        s1 = time.monotonic()
        bg = eng.submit(r1, RECEIVE, device_mask=1, background=True)
        s2 = time.monotonic()
        fg = eng.submit(r2, RECEIVE, device_mask=1)
        assert eng.pool_status() == (2, 1)
        tok.set()
        assert first.wait(30).status == _lib.NPOW_CANCELLED
        i2, i1 = fg.wait_info(30), bg.wait_info(30)
    finally:
        tok.set()
        eng.pool_config(64)
    assert i2.status == _lib.NPOW_OK and i1.status == _lib.NPOW_OK
    a2, a1 = s2 + i2.adopt_us * 1e-6, s1 + i1.adopt_us * 1e-6
    assert a2 < a1, f"the foreground job was adopted {(a2 - a1) * 1e3:.3f} ms after the background one"
    assert (i1.background, i2.background) == (1, 0)


def test_results_stay_right(gpu_engine):
    """24 searches at receive difficulty, alternating classes, every other background one promoted right after its
    submit: each result validates under hashlib against its own root, every status is NPOW_OK, the reported class is
    the one the job ended in, and the pool's protocol checks do not move."""
    eng = gpu_engine
    before = eng.stats(0)
    roots = _roots(99, 24)
    tickets, ended_bg = [], []
    for i, r in enumerate(roots):
        t = eng.submit(r, RECEIVE, start=i << 48, device_mask=1, background=i % 2 == 0)
        if i % 4 == 0:
            t.promote((1, 2, 8)[(i // 4) % 3])
        # its class from here on: a decided search keeps the one it had (the promotion came too late)
        cls = ctypes.c_uint32(7)
        assert eng.lib.npow_ticket_background(t.ticket, ctypes.byref(cls)) == _lib.NPOW_OK
        if i % 2 == 1:
            assert cls.value == 0
        elif i % 4 == 2:
            assert cls.value == 1
        tickets.append(t)
        ended_bg.append(cls.value)
    for i, (r, t) in enumerate(zip(roots, tickets)):
        info = t.wait_info(60)
        assert info is not None and info.status == _lib.NPOW_OK
        assert _value(r, info.nonce) == info.value >= RECEIVE
        assert info.background == ended_bg[i], (i, info.background, ended_bg[i])
    print(f"classes the searches ended in: {ended_bg}")
    assert sum(ended_bg) >= 6
    st = eng.stats(0)
    assert (st.early_mismatches, st.stale_missing) == (before.early_mismatches, before.stale_missing)


def test_arguments_and_a_parked_job(gpu_engine):
    """A background job parked beside two foreground ones: the argument errors of npow_promote, npow_retarget in
    place, and a cancel whose kill the other entries' pollers relay -- NPOW_CANCELLED within the bound of
    tests/test_gpu_pool.py's cancel test (10 s; the time is printed)."""
    eng, jobs = gpu_engine, _Jobs(gpu_engine, 100)
    with _one_long_launch(eng, jobs):
        t0 = _admit_together(eng, jobs, [False, False])
        _sleep_until(t0 + 0.005)
        s0 = eng.stats(0)
        ta = jobs.submit(background=True, threshold=M64 - 15)
        for w in (0, 3, 16):
            with pytest.raises(_lib.NanoPowError) as e:
                ta.promote(w)
            assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
            assert eng.lib.npow_promote(ta.ticket, w) == _lib.NPOW_ERR_BAD_ARGUMENT
        _sleep_until(t0 + 0.02)
        assert ta.retarget(M64) is True
        _sleep_until(t0 + 0.03)
        s1 = eng.stats(0)
        t_cancel = time.monotonic()
        ta.cancel()
        res = ta.wait(10)
        dt = time.monotonic() - t_cancel
        s2 = eng.stats(0)
        jobs.cancel_all()
        dc, dd = (t.wait(30).nonces_done for t in jobs.tickets[1:3])
    print(f"parked job: cancelled in {dt * 1e3:.3f} ms after {res.nonces_done} nonces beside C {dc} D {dd}; "
          f"dyn_entries {s0.dyn_entries} -> {s1.dyn_entries}, launches {s0.launches} -> {s2.launches}")
    assert res is not None and res.status == _lib.NPOW_CANCELLED
    assert s1.dyn_entries > s0.dyn_entries and _same_launch(s0, s2)
    assert res.nonces_done <= 0.01 * (dc + dd)
    with pytest.raises(_lib.NanoPowError):
        eng.submit(jobs.roots[9], M64, device_mask=1, max_nonces_per_device=1 << 30, background=True)


def test_two_cu_partitions():
    """The yield-and-return test on jobs split over two 32-CU partitions (NANOPOW_VIRTUAL_DEVICES=8: lingering
    launches are on), in a child process: the engine reads the variable once."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NANOPOW_VIRTUAL_DEVICES="8")
    p = subprocess.run([sys.executable, os.path.join(here, "background_partition_worker.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    da, db, dc = out["nonces"]
    ratio = (da + db) / max(dc, 1)
    print(f"two partitions: A {da} B {db} C {dc}, (A + B) / C = {ratio:.3f}, stats {out['devices']}")
    for d in out["devices"]:
        assert (d["yields_after"], d["launches_after"]) == (d["yields_before"], d["launches_before"]), out["devices"]
        assert d["stale_missing"] == 0 and d["early_mismatches"] == 0, out["devices"]
    assert math.sqrt(0.5 * 3) < ratio < math.sqrt(3 * 7), out["nonces"]
