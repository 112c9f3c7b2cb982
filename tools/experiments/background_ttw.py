#!/usr/bin/env python3
"""On-demand time-to-work beside precache load, three ways (GPU 0).

--n serial searches at --difficulty (default fffffff800000000), each timed from the submit to its result
(npow_wait_result), in three arms:
  alone       nothing else on the device;
  weighted    at weight 8 beside 15 endless searches of weight 1 (the share 8/23, README "Weighted shares");
  background  a foreground search beside 15 endless background searches (npow_submit_background).
Prints one JSON line per arm (p50, p99, mean in ms; the device's yields, launches and dynamic entries over the arm)
and one with the ratios to the first arm.

    python tools/experiments/background_ttw.py [--n 200] [--difficulty fffffff800000000] [--load 15]
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


def arm(eng, rng, name, n, threshold, load, **load_kw):
    root = lambda: bytes(rng.getrandbits(8) for _ in range(32))  # noqa: E731
    toks = [_lib.CancelToken() for _ in range(load)]
    busy = [eng.submit(root(), M64, start=(i + 1) << 52, device_mask=1, cancel=toks[i], **load_kw)
            for i in range(load)]
    if load:
        time.sleep(0.05)  # the load's launch is running
    weight = {"weight": 8} if name == "weighted" else {}
    s0 = eng.stats(0)
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        t = eng.submit(root(), threshold, start=rng.getrandbits(64), device_mask=1, **weight)
        res = t.wait_result()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert res.status == _lib.NPOW_OK
        t.wait()
    s1 = eng.stats(0)
    for c in toks:
        c.set()
    load_nonces = sum(t.wait(30).nonces_done for t in busy)
    ms.sort()
    return {"arm": name, "n": n, "load": load, "p50_ms": round(ms[len(ms) // 2], 3),
            "p99_ms": round(ms[min(len(ms) - 1, int(len(ms) * 0.99))], 3), "mean_ms": round(sum(ms) / len(ms), 3),
            "load_nonces": load_nonces, "yields": s1.yields - s0.yields, "launches": s1.launches - s0.launches,
            "dyn_entries": s1.dyn_entries - s0.dyn_entries, "clock_mhz": round(s1.clock_mhz, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--difficulty", default="fffffff800000000")
    ap.add_argument("--load", type=int, default=15)
    a = ap.parse_args()
    threshold = int(a.difficulty, 16)
    eng = _lib.engine()
    rng = random.Random(7)
    out = [arm(eng, rng, "alone", a.n, threshold, 0),
           arm(eng, rng, "weighted", a.n, threshold, a.load, weight=1),
           arm(eng, rng, "background", a.n, threshold, a.load, background=True)]
    for rec in out:
        print(json.dumps(rec), flush=True)
    print(json.dumps({"p50_over_alone": {r["arm"]: round(r["p50_ms"] / out[0]["p50_ms"], 3) for r in out},
                      "p99_over_alone": {r["arm"]: round(r["p99_ms"] / out[0]["p99_ms"], 3) for r in out},
                      "difficulty": a.difficulty}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
