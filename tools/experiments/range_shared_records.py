#!/usr/bin/env python3
"""Shared sweep jobs against the plain and the background class, and what a search pays beside each (one GPU,
device 0).

    python tools/experiments/range_shared_records.py latency [--n 200]
    python tools/experiments/range_shared_records.py rate    [--log2 34] [--rounds 3]
    python tools/experiments/range_shared_records.py moves   [--seconds 3]

latency: n serial first-win searches at fffffff800000000 alone, then the same roots while one long plain sweep job
runs on the device, while a background one does and while a shared one does (each cancelled afterwards): time-to-work
percentiles of the four arms, the nonces each job hashed meanwhile, its launches, cuts, held time and moves.
rate: [0, 2^log2) of the 2^36 fixture's root at its threshold as a shared sweep job alone, as a background one and
through npow_sweep, alternating; every hit set is compared with the fixture's hits inside the range.
moves: a shared sweep job beside a serial client of receive-difficulty searches for `seconds`: the job's nonces per
second, the client's searches, the job's moves.  Run it twice, the second time with NANOPOW_TEST_HOOKS=1
NANOPOW_SHARED_NO_MOVES=1 (no workgroup moves to the job's entry): the difference is what the kernel's move buys.
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

SEND, RECEIVE = 0xfffffff800000000, 0xfffffe0000000000
CLASSES = {"plain": {}, "background": {"background": True}, "shared": {"shared": True}}


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_2p36.json")) as f:
        g = json.load(f)
    return bytes.fromhex(g["root"]), int(g["threshold"], 16), [int(h, 16) for h in g["hits"]]


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def job_line(job):
    i, s = job.info(), job.share()
    job.cancel()
    r = job.wait(30)
    return {"job_nonces_done": r.nonces_done, "job_status": r.status, "launches": i.launches,
            "launches_cut": i.launches_cut, "held_us": i.held_us, "moves": s.moves}


def latency(eng, n):
    root, thr, _ = fixture()
    roots = [bytes([(i * 7 + k) & 0xff for k in range(32)]) for i in range(n)]
    for arm in ("alone", "plain", "background", "shared"):
        job = None
        if arm != "alone":
            job = eng.submit_sweep(root, thr, 0, 1 << 44, device_mask=1, **CLASSES[arm])
            time.sleep(0.05)
        ms = []
        t0 = time.perf_counter()
        for r in roots:
            t = time.perf_counter()
            res = eng.submit(r, SEND, device_mask=1).wait()
            ms.append((time.perf_counter() - t) * 1e3)
            assert res.status == _lib.NPOW_OK and res.value >= SEND
        line = {"record": "search_ttw", "arm": arm, "n": n, "p50_ms": round(statistics.median(ms), 3),
                "p90_ms": round(pct(ms, 0.9), 3), "p99_ms": round(pct(ms, 0.99), 3), "mean_ms": round(sum(ms) / n, 3),
                "seconds": round(time.perf_counter() - t0, 3)}
        if job:
            line.update(job_line(job))
        print(json.dumps(line), flush=True)


def rate(eng, log2, rounds):
    root, thr, hits = fixture()
    count = 1 << log2
    want = [h for h in hits if h < count]
    for rnd in range(rounds):
        for arm in ("shared", "background", "npow_sweep"):
            line = {}
            t = time.perf_counter()
            if arm == "npow_sweep":
                got, ok = eng.sweep(root, thr, 0, count, device_mask=1), True
                dt = time.perf_counter() - t
            else:
                tk = eng.submit_sweep(root, thr, 0, count, device_mask=1, **CLASSES[arm])
                while not tk.info().finished:
                    time.sleep(0.0005)
                dt = time.perf_counter() - t
                i, s = tk.info(), tk.share()
                line = {"launches": i.launches, "launches_cut": i.launches_cut, "held_us": i.held_us, "moves": s.moves}
                r = tk.wait()
                got, ok = r.hits, r.status == _lib.NPOW_OK and r.nonces_done == count
            print(json.dumps({"record": "sweep_rate", "arm": arm, "round": rnd, "log2_count": log2,
                              "seconds": round(dt, 4), "gnonce_per_s": round(count / dt / 1e9, 3), "hits": len(got),
                              "exact": bool(ok and got == want), **line}), flush=True)


def moves(eng, seconds):
    root, thr, _ = fixture()
    off = os.environ.get("NANOPOW_TEST_HOOKS") == "1" and os.environ.get("NANOPOW_SHARED_NO_MOVES") == "1"
    job = eng.submit_sweep(root, thr, 0, 1 << 44, device_mask=1, shared=True)
    time.sleep(0.05)
    n0, t0, k, ms, dec, fin = job.info().nonces_done, time.perf_counter(), 0, [], [], []
    while time.perf_counter() - t0 < seconds:
        t = time.perf_counter()
        res = eng.submit(bytes([(k * 7 + j) & 0xff for j in range(32)]), RECEIVE, device_mask=1).wait_info()
        ms.append((time.perf_counter() - t) * 1e3)
        assert res.status == _lib.NPOW_OK
        dec.append(res.decide_us * 1e-3)
        fin.append(res.finish_us * 1e-3)
        k += 1
    dt = time.perf_counter() - t0
    n1 = job.info().nonces_done
    print(json.dumps({"record": "shared_beside_serial_client", "moves_enabled": not off, "seconds": round(dt, 3),
                      "searches": k, "search_p50_ms": round(statistics.median(ms), 3),
                      "decide_p50_ms": round(statistics.median(dec), 3),
                      "finish_p50_ms": round(statistics.median(fin), 3),
                      "job_gnonce_per_s": round((n1 - n0) / dt / 1e9, 3), **job_line(job)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("latency", "rate", "moves"))
    ap.add_argument("--log2", type=int, default=34)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=3.0)
    a = ap.parse_args()
    eng = _lib.Engine()
    {"latency": lambda: latency(eng, a.n), "rate": lambda: rate(eng, a.log2, a.rounds),
     "moves": lambda: moves(eng, a.seconds)}[a.what]()


if __name__ == "__main__":
    main()
