"""Child process of tests/test_gpu_background.py: background searches on jobs split over two CU partitions.  Run with
NANOPOW_VIRTUAL_DEVICES=8 (32-CU partitions: lingering launches are on).  Two endless background jobs, each split over
devices 0 and 1 (device_mask 3), are admitted together behind a blocker, so each device runs them in one counted
launch that outlasts the run; a foreground job joins at 20 ms and is cancelled at 60 ms, and the background jobs are
cancelled at 160 ms.  Prints one JSON line: the jobs' nonce counts (A, B, C) and each device's counters at 10 ms and
at 160 ms."""
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

M64 = (1 << 64) - 1


def main():
    eng = _lib.Engine()
    assert eng.n_devices == 8 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    eng.set_pool_tuning(budget_us=400000)
    eng.set_tuning(65536)
    eng.pool_config(1)
    rng = random.Random(101)
    roots = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(4)]
    toks = [_lib.CancelToken() for _ in range(4)]
    try:
        return run(eng, roots, toks)
    finally:
        for c in toks:  # (a run that failed half-way leaves no endless search behind)
            c.set()


def run(eng, roots, toks):
    tx = eng.submit(roots[3], M64, device_mask=3, cancel=toks[3])
    ta, tb = (eng.submit(roots[i], M64, start=(i + 1) << 52, device_mask=3, cancel=toks[i], background=True)
              for i in range(2))
    assert eng.pool_status() == (2, 1)
    eng.pool_config(64)
    toks[3].set()
    assert tx.wait(30).status == _lib.NPOW_CANCELLED
    t0 = time.monotonic()
    time.sleep(0.01)
    before = [eng.stats(d) for d in range(2)]
    time.sleep(max(0.0, t0 + 0.02 - time.monotonic()))
    tc = eng.submit(roots[2], M64, start=3 << 52, device_mask=3, cancel=toks[2])
    time.sleep(max(0.0, t0 + 0.06 - time.monotonic()))
    toks[2].set()
    rc = tc.wait(30)
    assert rc is not None and rc.status == _lib.NPOW_CANCELLED
    time.sleep(max(0.0, t0 + 0.16 - time.monotonic()))
    after = [eng.stats(d) for d in range(2)]
    for c in toks:
        c.set()
    done = []
    for t in (ta, tb):
        res = t.wait(30)
        assert res is not None and res.status == _lib.NPOW_CANCELLED
        done.append(res.nonces_done)
    done.append(rc.nonces_done)
    end = [eng.stats(d) for d in range(2)]
    devices = [{"yields_before": b.yields, "yields_after": a.yields, "launches_before": b.launches,
                "launches_after": a.launches, "dyn_before": b.dyn_entries, "dyn_after": a.dyn_entries,
                "early_mismatches": e.early_mismatches, "stale_missing": e.stale_missing}
               for b, a, e in zip(before, after, end)]
    print(json.dumps({"nonces": done, "devices": devices}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
