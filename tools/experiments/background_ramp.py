#!/usr/bin/env python3
"""How fast background workgroups leave for a foreground search that joins their launch (GPU 0).

The shape of tests/test_gpu_background.py: two endless background jobs A and B share one long counted launch; after
--before ms a foreground job C joins it as a dynamic entry, and d ms later all three are cancelled, for d in --ms
(every d a run of its own: twins, other roots).  Between two consecutive delays d1 < d2 the marginal share of C,
(C(d2) - C(d1)) / (total(d2) - total(d1)), is the share of the device C held in that window: 0 before the first
workgroup has moved, 1 once every background workgroup has polled and left.  The first window at 0.9 or more bounds the
ramp from C's publish.  From the poll cadence one expects about 2 ms (128 wave iterations of about 15 us until every
workgroup has polled); that is a derivation, this is the measurement.

    python tools/experiments/background_ramp.py [--ms 0,0.25,0.5,1,2,3,4,6,8,16] [--rounds 3]
"""
import argparse
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

M64 = (1 << 64) - 1


def one_run(eng, rng, before_ms, d_ms):
    root = lambda: bytes(rng.getrandbits(8) for _ in range(32))  # noqa: E731
    eng.pool_config(1)
    toks = [_lib.CancelToken() for _ in range(4)]
    tx = eng.submit(root(), M64, device_mask=1, cancel=toks[3])
    ta = eng.submit(root(), M64, start=1 << 52, device_mask=1, cancel=toks[0], background=True)
    tb = eng.submit(root(), M64, start=2 << 52, device_mask=1, cancel=toks[1], background=True)
    eng.pool_config(64)
    toks[3].set()
    tx.wait(30)
    t0 = time.perf_counter()
    time.sleep(max(0.0, t0 + before_ms * 1e-3 - time.perf_counter()))
    s0 = eng.stats(0)
    tp = time.perf_counter()
    tc = eng.submit(root(), M64, start=3 << 52, device_mask=1, cancel=toks[2])
    time.sleep(max(0.0, tp + d_ms * 1e-3 - time.perf_counter()))
    for c in toks:
        c.set()
    t_cancel = time.perf_counter()
    da, db, dc = (t.wait(30).nonces_done for t in (ta, tb, tc))
    s1 = eng.stats(0)
    return {"d_ms": d_ms, "after_submit_ms": round((t_cancel - tp) * 1e3, 3), "a": da, "b": db, "c": dc,
            "dyn_entries": s1.dyn_entries - s0.dyn_entries, "yields": s1.yields - s0.yields,
            "launches": s1.launches - s0.launches, "clock_mhz": round(s1.clock_mhz, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="0,0.25,0.5,1,2,3,4,6,8,16")
    ap.add_argument("--before", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    spans = [float(x) for x in a.ms.split(",")]
    eng = _lib.engine()
    rng = random.Random(8)
    eng.set_pool_tuning(budget_us=1000000)
    eng.set_tuning(65536)
    runs = []
    try:
        for rnd in range(a.rounds):
            for d in spans:
                rec = one_run(eng, rng, a.before, d)
                rec.update(round=rnd)
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        eng.pool_config(64)
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)
    mean = {}
    for d in spans:
        rs = [r for r in runs if r["d_ms"] == d]
        # (A and B hashed for --before ms first: only what came after C's submit counts, so the totals are differenced)
        mean[d] = (sum(r["c"] for r in rs) / len(rs), sum(r["a"] + r["b"] + r["c"] for r in rs) / len(rs),
                   sum(r["after_submit_ms"] for r in rs) / len(rs))
    for d1, d2 in zip(spans, spans[1:]):
        (c1, t1, m1), (c2, t2, m2) = mean[d1], mean[d2]
        print(json.dumps({"window_ms": [round(m1, 3), round(m2, 3)],
                          "marginal_share_c": round((c2 - c1) / max(t2 - t1, 1.0), 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
