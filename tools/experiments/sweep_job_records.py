#!/usr/bin/env python3
"""Sweep jobs against npow_sweep, and what a search pays while a sweep job runs (one GPU, device 0).

    python tools/experiments/sweep_job_records.py rate    [--log2 34] [--pairs 3]
    python tools/experiments/sweep_job_records.py latency [--n 200]

rate: [0, 2^log2) of the 2^36 fixture's root at its threshold, as a sweep job alone (npow_submit_sweep) and
through npow_sweep, alternating; both hit sets are compared with the fixture's hits inside the range.  One JSON
line per run, then one with both arms' best rates and their ratio.
latency: n serial first-win searches at fffffff800000000 alone, then the same roots while one long sweep job
runs on the device (cancelled afterwards); time-to-work percentiles of both arms.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

SEND = 0xfffffff800000000


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_2p36.json")) as f:
        g = json.load(f)
    return bytes.fromhex(g["root"]), int(g["threshold"], 16), [int(h, 16) for h in g["hits"]]


def rate(eng, log2, pairs):
    root, thr, hits = fixture()
    count = 1 << log2
    want = [h for h in hits if h < count]
    best = {"job": 0.0, "npow_sweep": 0.0}
    for pair in range(pairs):
        for arm in ("job", "npow_sweep"):
            t = time.perf_counter()
            if arm == "job":
                r = eng.submit_sweep(root, thr, 0, count, device_mask=1).wait()
                got, ok = r.hits, r.status == _lib.NPOW_OK and r.nonces_done == count
            else:
                got, ok = eng.sweep(root, thr, 0, count, device_mask=1), True
            dt = time.perf_counter() - t
            gnps = count / dt / 1e9
            best[arm] = max(best[arm], gnps)
            print(json.dumps({"record": "sweep_rate", "arm": arm, "pair": pair, "log2_count": log2, "seconds": round(dt, 4),
                              "gnonce_per_s": round(gnps, 3), "hits": len(got), "exact": bool(ok and got == want)}),
                  flush=True)
    print(json.dumps({"record": "sweep_rate_summary", "log2_count": log2, "best_job": round(best["job"], 3),
                      "best_npow_sweep": round(best["npow_sweep"], 3),
                      "ratio_job_over_npow_sweep": round(best["job"] / best["npow_sweep"], 4)}), flush=True)


def ttw(eng, roots):
    out = []
    for r in roots:
        t = time.perf_counter()
        res = eng.submit(r, SEND, device_mask=1).wait()
        out.append((time.perf_counter() - t) * 1e3)
        assert res.status == _lib.NPOW_OK and res.value >= SEND
    return out


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def latency(eng, n):
    root, thr, _ = fixture()
    roots = [bytes([(i * 7 + k) & 0xff for k in range(32)]) for i in range(n)]
    for arm in ("alone", "beside_sweep_job"):
        job = eng.submit_sweep(root, thr, 0, 1 << 44, device_mask=1) if arm == "beside_sweep_job" else None
        if job:
            time.sleep(0.05)
        ms = ttw(eng, roots)
        line = {"record": "search_ttw", "arm": arm, "n": n, "p50_ms": round(statistics.median(ms), 3),
                "p90_ms": round(pct(ms, 0.9), 3), "p99_ms": round(pct(ms, 0.99), 3), "mean_ms": round(sum(ms) / n, 3)}
        if job:
            job.cancel()
            r = job.wait(30)
            line["sweep_job_nonces_done"] = r.nonces_done
            line["sweep_job_status"] = r.status
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rate", "latency"))
    ap.add_argument("--log2", type=int, default=34)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--n", type=int, default=200)
    a = ap.parse_args()
    eng = _lib.Engine()
    if a.what == "rate":
        rate(eng, a.log2, a.pairs)
    else:
        latency(eng, a.n)


if __name__ == "__main__":
    main()
