#!/usr/bin/env python3
"""How fast a job promoted inside a running launch collects its new share (GPU 0).

The shape of tests/test_gpu_promote.py: three endless weight-1 jobs A, B and C share one long counted launch (C a
table entry, or with --dynamic a dynamic entry that joined it); after --before ms C is promoted to --weight, and
d ms later all three are cancelled, for d in --ms.  A promotion cannot be taken back, so every d is a run of its
own (twins: the same shape, other roots).  Between two consecutive delays d1 < d2 the marginal share of C,
(C(d2) - C(d1)) / (total(d2) - total(d1)), is the share of the device C held in that window: it starts at 1/3 and
ends at the nominal weight / (weight + 2).  The first window whose marginal share is within 10 % of the nominal
bounds the time from npow_promote to the share; the last windows show the share reached (and whether it
overshoots, as dynamic joins do).  Each run also reports promotions / yields / launches over its window.

    python tools/experiments/promote_convergence.py [--weight 8] [--ms 0,0.5,1,2,4,8,16,32,64] [--rounds 3] [--dynamic]
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


def one_run(eng, rng, weight, before_ms, d_ms, dynamic):
    root = lambda: bytes(rng.getrandbits(8) for _ in range(32))  # noqa: E731
    eng.pool_config(1)
    toks = [_lib.CancelToken() for _ in range(4)]
    tx = eng.submit(root(), M64, device_mask=1, cancel=toks[3])
    ta = eng.submit(root(), M64, start=1 << 52, device_mask=1, cancel=toks[0])
    tb = eng.submit(root(), M64, start=2 << 52, device_mask=1, cancel=toks[1])
    tc = None if dynamic else eng.submit(root(), M64, start=3 << 52, device_mask=1, cancel=toks[2])
    eng.pool_config(64)
    toks[3].set()
    tx.wait(30)
    t0 = time.perf_counter()
    if dynamic:
        time.sleep(0.003)
        tc = eng.submit(root(), M64, start=3 << 52, device_mask=1, cancel=toks[2])
    time.sleep(max(0.0, t0 + before_ms * 1e-3 - time.perf_counter()))
    s0 = eng.stats(0)
    tp = time.perf_counter()
    tc.promote(weight)
    time.sleep(max(0.0, tp + d_ms * 1e-3 - time.perf_counter()))
    for c in toks:
        c.set()
    t_cancel = time.perf_counter()
    da, db, dc = (t.wait(30).nonces_done for t in (ta, tb, tc))
    s1 = eng.stats(0)
    return {"d_ms": d_ms, "after_promote_ms": round((t_cancel - tp) * 1e3, 3), "a": da, "b": db, "c": dc,
            "promotions": s1.promotions - s0.promotions, "yields": s1.yields - s0.yields,
            "launches": s1.launches - s0.launches, "clock_mhz": round(s1.clock_mhz, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weight", type=int, default=8)
    ap.add_argument("--ms", default="0,0.5,1,2,4,8,16,32,64")
    ap.add_argument("--before", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dynamic", action="store_true")
    a = ap.parse_args()
    spans = [float(x) for x in a.ms.split(",")]
    eng = _lib.engine()
    rng = random.Random(6)
    eng.set_pool_tuning(budget_us=1000000)
    eng.set_tuning(65536)
    runs = []
    try:
        for rnd in range(a.rounds):
            for d in spans:
                rec = one_run(eng, rng, a.weight, a.before, d, a.dynamic)
                rec.update(round=rnd, weight=a.weight, dynamic=a.dynamic)
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        eng.pool_config(64)
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)
    # marginal shares between consecutive delays, the runs of each delay averaged over the rounds
    mean = {}
    for d in spans:
        rs = [r for r in runs if r["d_ms"] == d]
        mean[d] = (sum(r["c"] for r in rs) / len(rs), sum(r["a"] + r["b"] + r["c"] for r in rs) / len(rs),
                   sum(r["after_promote_ms"] for r in rs) / len(rs))
    nominal = a.weight / (a.weight + 2.0)
    for d1, d2 in zip(spans, spans[1:]):
        (c1, t1, m1), (c2, t2, m2) = mean[d1], mean[d2]
        print(json.dumps({"window_ms": [round(m1, 3), round(m2, 3)], "marginal_share_c": round((c2 - c1) / (t2 - t1), 4),
                          "nominal": round(nominal, 4), "weight": a.weight, "dynamic": a.dynamic}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
