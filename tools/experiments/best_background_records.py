#!/usr/bin/env python3
"""Background best jobs against plain best jobs and npow_sweep, and what a search pays beside each (one GPU,
device 0).

    python tools/experiments/best_background_records.py rate    [--log2 34] [--rounds 3]
    python tools/experiments/best_background_records.py latency [--n 200]

rate: [0, 2^log2) of the 2^36 fixture's root alone, alternating: a background best job at floor 0
(npow_submit_best_background), a plain best job at floor 0 and npow_sweep at ffff000000000000.  Exact against each
other and against the fixture (tests/golden/sweep_2p36.json, hits at fffffff800000000): a best job's answer must be the
strongest of the fixture's hits inside the range, the earliest among equal ones, by the CPU's work value, and
npow_sweep's hit set must hold every one of those hits and nothing stronger than that answer.  One JSON line per run
(a best job's with its launches, cuts and records_max), then one with the arms' best rates and their ratios.
latency: n serial first-win searches at fffffff800000000 alone, then the same roots while one long plain best job
runs on the device, then while one long background best job does (each cancelled afterwards); time-to-work
percentiles of the three arms, and the job's launches, cuts, held time and records_max.
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
AUDIT = 0xffff000000000000


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_2p36.json")) as f:
        g = json.load(f)
    return bytes.fromhex(g["root"]), int(g["threshold"], 16), [int(h, 16) for h in g["hits"]]


def rate(eng, log2, rounds):
    root, _, hits = fixture()
    count = 1 << log2
    want_hits = [h for h in hits if h < count]
    # the range's maximum is its strongest hit (the earliest among equal ones), by the CPU's work value
    want = max(((eng.work_value(root, h), -h) for h in want_hits), default=None)
    arms = ("background_best_job", "best_job", "npow_sweep")
    best = dict.fromkeys(arms, 0.0)
    for rnd in range(rounds):
        for arm in arms:
            line = {}
            t = time.perf_counter()
            if arm == "npow_sweep":
                got = eng.sweep(root, AUDIT, 0, count, device_mask=1, cap=1 << 20)
                dt = time.perf_counter() - t
                top = max(((eng.work_value(root, h), -h) for h in got), default=None)
                ok = set(want_hits) <= set(got) and top == want and all(h < count for h in got)
                line = {"threshold": f"{AUDIT:016x}", "hits": len(got)}
            else:
                tk = eng.submit_best(root, 0, count, floor=0, device_mask=1, background=arm.startswith("background"))
                while not tk.info().finished:
                    time.sleep(0.0005)
                dt = time.perf_counter() - t
                i, h = tk.info(), tk.hold()
                r = tk.wait()
                ok = (r.status == _lib.NPOW_OK and r.nonces_done == count and want is not None
                      and (r.value, -r.nonce) == want)
                line = {"launches": i.launches, "launches_cut": h.launches_cut, "held_us": h.held_us,
                        "records": i.records, "records_max": i.records_max, "room": i.room,
                        "nonce": f"{r.nonce:016x}", "value": f"{r.value:016x}"}
            gnps = count / dt / 1e9
            best[arm] = max(best[arm], gnps)
            print(json.dumps({"record": "best_rate", "arm": arm, "round": rnd, "log2_count": log2,
                              "seconds": round(dt, 4), "gnonce_per_s": round(gnps, 3), "exact": bool(ok), **line}),
                  flush=True)
    print(json.dumps({"record": "best_rate_summary", "log2_count": log2,
                      **{"best_" + a: round(best[a], 3) for a in arms},
                      "ratio_background_over_npow_sweep": round(best["background_best_job"] / best["npow_sweep"], 4),
                      "ratio_job_over_npow_sweep": round(best["best_job"] / best["npow_sweep"], 4),
                      "ratio_background_over_job": round(best["background_best_job"] / best["best_job"], 4)}),
          flush=True)


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
    root, _, _ = fixture()
    roots = [bytes([(i * 7 + k) & 0xff for k in range(32)]) for i in range(n)]
    for arm in ("alone", "beside_best_job", "beside_background_best_job"):
        job = None
        if arm != "alone":
            job = eng.submit_best(root, 0, 1 << 44, floor=0, device_mask=1, background=arm.startswith("beside_back"))
            time.sleep(0.05)
        ms = ttw(eng, roots)
        line = {"record": "search_ttw", "arm": arm, "n": n, "p50_ms": round(statistics.median(ms), 3),
                "p90_ms": round(pct(ms, 0.9), 3), "p99_ms": round(pct(ms, 0.99), 3), "mean_ms": round(sum(ms) / n, 3)}
        if job:
            i, h = job.info(), job.hold()
            job.cancel()
            r = job.wait(30)
            valid = r.nonce is None or eng.work_value(root, r.nonce) == r.value
            line.update(best_job_nonces_done=r.nonces_done, best_job_status=r.status, best_job_valid=bool(valid),
                        launches=i.launches, launches_cut=h.launches_cut, held_us=h.held_us,
                        records_max=i.records_max, room=i.room)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rate", "latency"))
    ap.add_argument("--log2", type=int, default=34)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=200)
    a = ap.parse_args()
    eng = _lib.Engine()
    {"rate": lambda: rate(eng, a.log2, a.rounds), "latency": lambda: latency(eng, a.n)}[a.what]()


if __name__ == "__main__":
    main()
