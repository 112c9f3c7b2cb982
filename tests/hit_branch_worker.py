"""The flow of tests/test_gpu_hit_branch.py -- park, move the threshold, release -- and that file's child process
(the engine reads its environment once).  As a program: NANOPOW_VIRTUAL_DEVICES=2, the every-lane-stale flow with
every search split over both CU partitions (device_mask 3), one JSON line on stdout.

The flow.  Two endless foreground searches F1 and F2 (threshold 2^64 - 1) share one counted launch that outlasts the
test (tests/test_gpu_background.py's tunings).  A background search B in that launch holds no workgroup while either
of them is live: it weighs 0 in the start map, and a foreground poller skips background targets.  B's entry was built
with the threshold of its submit, and npow_retarget / npow_relax write its slot's floor record while it is parked.
When F1 and F2 are cancelled every workgroup picks B, the only live entry, and each wave's first hash of B runs under
the watch threshold of the submit and finds the floor record already there.  No step waits a guessed time for the GPU
to reach a nonce."""
import contextlib
import hashlib
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

M64 = (1 << 64) - 1
WAVES = 8  # per workgroup (npow_internal.h kLsWaves)


def value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


def devices_of(mask):
    return [d for d in range(64) if (mask >> d) & 1]


class Jobs:
    """Searches on the devices of `mask`, each with a cancel token and a nonce region of its own: the blocker, F1, F2
    and B, in that order."""

    def __init__(self, eng, seed, mask=1):
        rng = random.Random(seed)
        self.eng, self.mask = eng, mask
        self.roots = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(4)]
        self.toks, self.tickets = [], []

    def submit(self, threshold=M64, **kw):
        i = len(self.tickets)
        self.toks.append(_lib.CancelToken())
        self.tickets.append(self.eng.submit(self.roots[i], threshold, start=(i + 1) << 52, device_mask=self.mask,
                                            cancel=self.toks[i], **kw))
        return self.tickets[-1]

    def end(self):
        """Cancel and collect whatever a flow that failed half-way left behind: no endless search outlives it."""
        for c in self.toks:
            c.set()
        for t in self.tickets:
            if t.result is None:
                t.wait(30)


@contextlib.contextmanager
def one_long_launch(eng, jobs):
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


def settled(eng, devices):
    """Each device's counters once its retired launches and its yields stand still (two equal reads 1 ms apart)."""
    def key():
        sts = [eng.stats(d) for d in devices]
        return sts, [(st.launches, st.yields) for st in sts]
    _, prev = key()
    for _ in range(2000):
        time.sleep(0.001)
        sts, now = key()
        if now == prev:
            return sts
        prev = now
    raise AssertionError("the devices' launches never settled")


def park(eng, jobs, how, threshold, reserve=None):
    """F1 and F2 running in one counted launch per device, B (background, `threshold`, `reserve`) parked in it: a
    table entry (how == "table": queued behind the blocker with them, admitted and adopted together) or a dynamic
    entry (how == "dynamic": submitted once their launch runs; npow_device_stats.dyn_entries steps).  Returns B.

    The blocker's result is the order's proof in the table case: its slot retires only after the yield that ended
    its one-entry launch, and the worker builds the next table -- F1, F2 and B, adopted in the call that raised the
    yield -- in that same step, before it retires anything."""
    devices = devices_of(jobs.mask)
    kw = {"background": True} if reserve is None else {"background": True, "reserve": reserve}
    eng.pool_config(1)
    blocker = jobs.submit()
    jobs.submit()
    jobs.submit()
    b = jobs.submit(threshold, **kw) if how == "table" else None
    assert eng.pool_status() == (3 if how == "table" else 2, 1)
    eng.pool_config(64)  # admitted, and adopted, together
    jobs.toks[0].set()
    assert blocker.wait(30).status == _lib.NPOW_CANCELLED
    settled(eng, devices)
    if how == "dynamic":
        time.sleep(0.005)  # (a launch takes dynamic entries once the one before it has retired)
        dyn0 = [st.dyn_entries for st in settled(eng, devices)]
        b = jobs.submit(threshold, **kw)
        deadline = time.monotonic() + 10
        while [eng.stats(d).dyn_entries for d in devices] != [n + 1 for n in dyn0]:
            assert time.monotonic() < deadline, "B did not join the running launches as one dynamic entry each"
            time.sleep(0.0002)
    return b


def release(eng, jobs):
    """Cancel F1 and F2 and collect them: their final counts are in, so every workgroup has left them.  Returns the
    devices' counters then."""
    jobs.toks[1].set()
    jobs.toks[2].set()
    for t in jobs.tickets[1:3]:
        res = t.wait(30)
        assert res is not None and res.status == _lib.NPOW_CANCELLED
    return [eng.stats(d) for d in devices_of(jobs.mask)]


def device_counts(st):
    return {k: getattr(st, k) for k in ("launches", "yields", "grid", "invalid_work", "dead", "early_mismatches",
                                        "stale_missing", "dyn_entries")}


def raised_while_parked(eng, seed, how, t0, t1, mask=1, run_ms=20):
    """B parked at threshold t0, retargeted to t1, released; cancelled run_ms after the release (None: it ends by
    itself).  Returns what the tests assert on: plain numbers."""
    jobs = Jobs(eng, seed, mask)
    devices = devices_of(mask)
    with one_long_launch(eng, jobs):
        before = settled(eng, devices)
        b = park(eng, jobs, how, t0)
        held = b.retarget(t1)
        rel = release(eng, jobs)
        if run_ms is not None:
            time.sleep(run_ms * 1e-3)
        end = [eng.stats(d) for d in devices]  # (before B ends: its launch retires right after it)
        if run_ms is not None:
            jobs.toks[3].set()
        info = b.wait_info(30)
        assert info is not None
        after = [eng.stats(d) for d in devices]
    return {"held": held, "status": info.status, "nonce": info.nonce, "value": info.value,
            "hashlib": value(jobs.roots[3], info.nonce) if info.status == _lib.NPOW_OK else None,
            "stale_hits": info.stale_hits, "stale_wins": info.stale_wins, "retargets": info.retargets,
            "nonces_done": info.nonces_done, "n_devices": info.n_devices, "background": info.background,
            "waves": WAVES * sum(st.grid for st in after),
            "before": [device_counts(st) for st in before], "release": [device_counts(st) for st in rel],
            "end": [device_counts(st) for st in end], "after": [device_counts(st) for st in after]}


def main():
    eng = _lib.Engine()
    assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    print(json.dumps(raised_while_parked(eng, 131, "table", 0, M64, mask=3)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
