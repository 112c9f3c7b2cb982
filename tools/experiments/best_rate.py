"""Rates of a lone 2^34 best job (floor 0, floor fffff00000000000) against a lone 2^34 sweep job at
ffff000000000000, alternating three times on device 0 after one warm-up sweep job; the records the best jobs'
launches appended.  One JSON line each, on stdout and appended to bench_out/best_rate.jsonl
(profiles/r17a_best_rate.jsonl is one run's file).

    python tools/experiments/best_rate.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle  # noqa: E402
from nanopow import _lib  # noqa: E402

OUT = os.path.join(ROOT, "bench_out", "best_rate.jsonl")
ROOT_A = bytes(range(3, 35))
START, COUNT = 0x0123456789abcdef, 1 << 34


def emit(rec):
    print(json.dumps(rec), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")


def best(eng, floor, run):
    eng.reset_stats(0)
    t0 = time.perf_counter()
    t = eng.submit_best(ROOT_A, START, COUNT, floor=floor, device_mask=1)
    info = t.info()
    while not info.finished:
        time.sleep(0.002)
        info = t.info()
    dt = time.perf_counter() - t0
    r = t.wait(5)
    st = eng.stats(0)
    ok = r.status == _lib.NPOW_OK and oracle.work_value_hashlib(ROOT_A, r.nonce) == r.value and r.nonces_done == COUNT
    emit({"job": "best", "floor": f"{floor:016x}", "run": run, "seconds": round(dt, 4),
          "gnonce_per_s": round(COUNT / dt / 1e9, 3), "kernel_ms": round(st.kernel_ms, 2),
          "gnonce_per_s_kernel": round(COUNT / st.kernel_ms / 1e6, 3) if st.kernel_ms else None,
          "launches": info.launches, "records": info.records, "records_max": info.records_max, "room": info.room,
          "records_per_launch": round(info.records / max(info.launches, 1), 2),
          "nonce": f"{r.nonce:016x}", "value": f"{r.value:016x}", "valid": ok})
    return ok


def sweep(eng, run):
    thr = 0xffff000000000000
    eng.reset_stats(0)
    t0 = time.perf_counter()
    r = eng.submit_sweep(ROOT_A, thr, START, COUNT, device_mask=1, cap=1 << 20).wait(120)
    dt = time.perf_counter() - t0
    st = eng.stats(0)
    ok = r.status == _lib.NPOW_OK and r.nonces_done == COUNT
    emit({"job": "sweep", "threshold": f"{thr:016x}", "run": run, "seconds": round(dt, 4),
          "gnonce_per_s": round(COUNT / dt / 1e9, 3), "kernel_ms": round(st.kernel_ms, 2),
          "gnonce_per_s_kernel": round(COUNT / st.kernel_ms / 1e6, 3) if st.kernel_ms else None,
          "hits": r.total, "launches": st.launches, "valid": ok})
    return ok


def main():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    eng = _lib.Engine()
    ok = True
    sweep(eng, "warmup")
    for run in range(3):
        ok = sweep(eng, run) and ok
        ok = best(eng, 0, run) and ok
        ok = best(eng, 0xfffff00000000000, run) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
