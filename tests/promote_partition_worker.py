"""Child process of tests/test_gpu_promote.py: a promotion on a job split over two CU partitions.  Run with
NANOPOW_VIRTUAL_DEVICES=2.  Three endless jobs of weight 1, each split over both devices (device_mask 3), are admitted
together behind a blocker, so each device runs them in one counted launch that outlasts the run; the third is
promoted to 8 after 20 ms and all are cancelled 100 ms later.  Prints one JSON line: the jobs' nonce counts and each
device's counters before and after the promotion's window."""
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
    assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    eng.set_pool_tuning(budget_us=400000)
    eng.set_tuning(65536)
    eng.pool_config(1)
    rng = random.Random(89)
    roots = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(4)]
    toks = [_lib.CancelToken() for _ in range(4)]
    tx = eng.submit(roots[3], M64, device_mask=3, cancel=toks[3])
    tickets = [eng.submit(roots[i], M64, start=(i + 1) << 52, device_mask=3, cancel=toks[i], weight=1)
               for i in range(3)]
    assert eng.pool_status() == (3, 1)
    eng.pool_config(64)
    toks[3].set()
    assert tx.wait(30).status == _lib.NPOW_CANCELLED
    t0 = time.monotonic()
    time.sleep(0.02)
    before = [eng.stats(d) for d in range(2)]
    tickets[2].promote(8)
    time.sleep(max(0.0, t0 + 0.12 - time.monotonic()))
    after = [eng.stats(d) for d in range(2)]
    for c in toks:
        c.set()
    done = []
    for t in tickets:
        res = t.wait(30)
        assert res is not None and res.status == _lib.NPOW_CANCELLED
        done.append(res.nonces_done)
    end = [eng.stats(d) for d in range(2)]
    devices = [{"promotions_before": b.promotions, "promotions_after": a.promotions, "yields_before": b.yields,
                "yields_after": a.yields, "launches_before": b.launches, "launches_after": a.launches,
                "early_mismatches": e.early_mismatches, "stale_missing": e.stale_missing}
               for b, a, e in zip(before, after, end)]
    print(json.dumps({"nonces": done, "devices": devices}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
