#!/usr/bin/env python3
"""How fast a weight-8 job that joins a running launch collects its share (GPU 0).

The shape of tests/test_gpu_weights.py::test_heavy_job_joins_a_running_launch: two endless weight-1 jobs A and B
share one long counted launch; an endless job C of weight --weight joins it as a dynamic entry and is cancelled
d ms later, for d in --ms.  C's nonce count over d, against its full share (weight / (weight + 2)) of the device's
rate -- which each round reports from all three jobs' counts over its wall time --, gives the time C lost while
workgroups moved to it:
lag = d - nonces_C / (share x rate).  While C is still collecting, the lag grows with d; once it has its share the
lag stays put, and that plateau is the convergence cost in time.  The marginal share between two consecutive d's
is printed too: the first d at which it reaches 0.9 bounds the time from publish to 90 % of the share.
(C's span is taken from its own timeline, launch_us to finish_us of npow_wait_info, not from the sleeps.)

    python tools/experiments/weight_join_convergence.py [--weight 8] [--ms 0.5,1,2,4,8,16] [--rounds 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weight", type=int, default=8)
    ap.add_argument("--ms", default="0.5,1,2,4,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    spans = [float(x) for x in a.ms.split(",")]
    eng = _lib.engine()
    rng = random.Random(5)
    root = lambda: bytes(rng.getrandbits(8) for _ in range(32))  # noqa: E731
    eng.set_pool_tuning(budget_us=1000000)
    eng.set_tuning(65536)
    out = []
    try:
        for rnd in range(a.rounds):
            # A and B admitted together behind a blocker, so that one counted launch holds both
            eng.pool_config(1)
            tx_tok, ta_tok, tb_tok = _lib.CancelToken(), _lib.CancelToken(), _lib.CancelToken()
            tx = eng.submit(root(), M64, device_mask=1, cancel=tx_tok)
            ta = eng.submit(root(), M64, start=1 << 52, device_mask=1, cancel=ta_tok)
            tb = eng.submit(root(), M64, start=2 << 52, device_mask=1, cancel=tb_tok)
            t0 = time.perf_counter()
            eng.pool_config(64)
            tx_tok.set()
            tx.wait(30)
            time.sleep(0.025)
            c_total = 0
            for d in spans:
                tok = _lib.CancelToken()
                dyn0 = eng.stats(0).dyn_entries
                tc = eng.submit(root(), M64, start=rng.getrandbits(60), device_mask=1, cancel=tok, weight=a.weight)
                time.sleep(d * 1e-3)
                tok.set()
                info = tc.wait_info(30)
                joined = eng.stats(0).dyn_entries > dyn0
                out.append({"round": rnd, "d_ms": d, "weight": a.weight, "joined_running_launch": joined,
                            "nonces": info.nonces_done, "span_us": round(info.finish_us - info.launch_us, 1)})
                c_total += info.nonces_done
                time.sleep(0.003)  # A and B take the workgroups back (C's entry is dead: ls2_choose)
            wall = time.perf_counter() - t0
            ta_tok.set()
            tb_tok.set()
            da, db = ta.wait(30).nonces_done, tb.wait(30).nonces_done
            # the device's rate over the round (A and B ran for all of it; their cancel's latency is ~0.1 ms of it)
            out.append({"round": rnd, "a_nonces": da, "b_nonces": db, "wall_s": round(wall, 4),
                        "device_nonces_per_us": round((da + db + c_total) / (wall * 1e6), 1)})
    finally:
        eng.pool_config(64)
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)
    for rec in out:
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
