#!/usr/bin/env python3
"""Background sweep jobs against plain sweep jobs and npow_sweep, and what a search pays beside each (one GPU,
device 0).

    python tools/experiments/sweep_background_records.py rate    [--log2 34] [--rounds 3]
    python tools/experiments/sweep_background_records.py latency [--n 200]
    python tools/experiments/sweep_background_records.py chunk

rate: [0, 2^log2) of the 2^36 fixture's root at its threshold as a background sweep job alone
(npow_submit_sweep_background), as a plain sweep job and through npow_sweep, alternating; every hit set is compared
with the fixture's hits inside the range.  One JSON line per run (a background job's with its launches and cuts), then
one with the arms' best rates and their ratios.
latency: n serial first-win searches at fffffff800000000 alone, then the same roots while one long plain sweep job
runs on the device, then while one long background sweep job does (each cancelled afterwards); time-to-work
percentiles of the three arms, and the background job's launches, cuts and held time.
chunk: the time of one chunk, the preemption bound.  A background job whose span is one chunk per workgroup of the
grid (grid x 8,192 nonces, read from the device's statistics) is one launch in which every workgroup hashes exactly
one chunk: the launch's kernel time is a chunk's time plus the launch's start and end.  Beside it, the same for two
and four chunks per workgroup, whose differences are chunk times without the start and end.
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
CHUNK = 16 * 512


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_2p36.json")) as f:
        g = json.load(f)
    return bytes.fromhex(g["root"]), int(g["threshold"], 16), [int(h, 16) for h in g["hits"]]


def rate(eng, log2, rounds):
    root, thr, hits = fixture()
    count = 1 << log2
    want = [h for h in hits if h < count]
    arms = ("background_job", "job", "npow_sweep")
    best = dict.fromkeys(arms, 0.0)
    for rnd in range(rounds):
        for arm in arms:
            line = {}
            t = time.perf_counter()
            if arm == "npow_sweep":
                got, ok = eng.sweep(root, thr, 0, count, device_mask=1), True
            else:
                tk = eng.submit_sweep(root, thr, 0, count, device_mask=1, background=arm == "background_job")
                while not tk.info().finished:
                    time.sleep(0.0005)
                dt = time.perf_counter() - t
                i = tk.info()
                line = {"launches": i.launches, "launches_cut": i.launches_cut, "held_us": i.held_us}
                r = tk.wait()
                got, ok = r.hits, r.status == _lib.NPOW_OK and r.nonces_done == count
            if arm == "npow_sweep":
                dt = time.perf_counter() - t
            gnps = count / dt / 1e9
            best[arm] = max(best[arm], gnps)
            print(json.dumps({"record": "sweep_rate", "arm": arm, "round": rnd, "log2_count": log2,
                              "seconds": round(dt, 4), "gnonce_per_s": round(gnps, 3), "hits": len(got),
                              "exact": bool(ok and got == want), **line}), flush=True)
    print(json.dumps({"record": "sweep_rate_summary", "log2_count": log2,
                      **{"best_" + a: round(best[a], 3) for a in arms},
                      "ratio_background_over_npow_sweep": round(best["background_job"] / best["npow_sweep"], 4),
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
    for arm in ("alone", "beside_sweep_job", "beside_background_sweep_job"):
        job = None
        if arm != "alone":
            job = eng.submit_sweep(root, thr, 0, 1 << 44, device_mask=1, background=arm.startswith("beside_back"))
            time.sleep(0.05)
        ms = ttw(eng, roots)
        line = {"record": "search_ttw", "arm": arm, "n": n, "p50_ms": round(statistics.median(ms), 3),
                "p90_ms": round(pct(ms, 0.9), 3), "p99_ms": round(pct(ms, 0.99), 3), "mean_ms": round(sum(ms) / n, 3)}
        if job:
            i = job.info()
            job.cancel()
            r = job.wait(30)
            line.update(sweep_job_nonces_done=r.nonces_done, sweep_job_status=r.status, launches=i.launches,
                        launches_cut=i.launches_cut, held_us=i.held_us)
        print(json.dumps(line), flush=True)


def chunk(eng):
    root, thr, _ = fixture()
    grid = eng.stats(0).grid
    res = {}
    for per_wg in (1, 2, 4, 1, 2, 4):
        count = grid * CHUNK * per_wg
        eng.reset_stats(0)
        tk = eng.submit_sweep(root, thr, 0, count, device_mask=1, background=True)
        r = tk.wait()
        s = eng.stats(0)
        assert r.status == _lib.NPOW_OK and r.nonces_done == count
        res.setdefault(per_wg, []).append(s.kernel_ms / max(1, s.launches))
        print(json.dumps({"record": "chunk_launch", "grid": grid, "chunks_per_workgroup": per_wg, "nonces": count,
                          "launches": s.launches, "kernel_ms": round(s.kernel_ms, 4)}), flush=True)
    m = {k: min(v) for k, v in res.items()}
    print(json.dumps({"record": "chunk_time", "grid": grid, "one_chunk_launch_ms": round(m[1], 4),
                      "chunk_ms_from_2_minus_1": round(m[2] - m[1], 4),
                      "chunk_ms_from_4_minus_2_halved": round((m[4] - m[2]) / 2, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rate", "latency", "chunk"))
    ap.add_argument("--log2", type=int, default=34)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=200)
    a = ap.parse_args()
    eng = _lib.Engine()
    {"rate": lambda: rate(eng, a.log2, a.rounds), "latency": lambda: latency(eng, a.n), "chunk": lambda: chunk(eng)}[
        a.what]()


if __name__ == "__main__":
    main()
