#!/usr/bin/env python3
"""Relaxed request against a fresh search, at the C ABI ("Reserve hits").

Arm "relax": a search at the send difficulty with the receive difficulty as its reserve runs alone on device 0; once
its reserve holds a nonce, time npow_relax(receive) -> npow_wait_result returning (zero timeout: the answer is there).
Arm "fresh": npow_submit at the receive difficulty -> npow_wait_result returning, the same roots.
One JSON line: p50 / p90 / max of each arm in microseconds and the sample counts.

    python tools/experiments/reserve_relax_latency.py [--n 200]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

SEND, RECEIVE = 0xfffffff800000000, 0xfffffe0000000000


def pct(xs, p):
    xs = sorted(xs)
    return round(xs[min(len(xs) - 1, int(p * len(xs)))], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    args = ap.parse_args()
    eng = _lib.Engine()
    lib = eng.lib
    rng = random.Random(12)
    roots = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(args.n)]
    nonce, value, ans = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    relax_us, fresh_us, skipped = [], [], 0
    for i, root in enumerate(roots):
        t = eng.submit(root, SEND, start=i << 40, device_mask=1, reserve=RECEIVE)
        deadline = time.monotonic() + 5
        while t.reserve() is None and time.monotonic() < deadline:
            pass
        t0 = time.perf_counter()
        rc = lib.npow_relax(t.ticket, RECEIVE, ctypes.byref(ans))
        rc2 = lib.npow_wait_result(t.ticket, 0, ctypes.byref(nonce), ctypes.byref(value))
        t1 = time.perf_counter()
        if rc == _lib.NPOW_OK and ans.value == 1 and rc2 == _lib.NPOW_OK and value.value >= RECEIVE:
            relax_us.append((t1 - t0) * 1e6)
        else:
            skipped += 1  # (decided at the send difficulty before the relax)
            t.cancel()
        t.wait(30)
    for i, root in enumerate(roots):
        tk = ctypes.c_uint64(0)
        t0 = time.perf_counter()
        lib.npow_submit(root, RECEIVE, i << 40, 1, 0, None, ctypes.byref(tk))
        rc = lib.npow_wait_result(tk.value, -1, ctypes.byref(nonce), ctypes.byref(value))
        t1 = time.perf_counter()
        assert rc == _lib.NPOW_OK and value.value >= RECEIVE
        fresh_us.append((t1 - t0) * 1e6)
        lib.npow_wait(tk.value, -1, None, None, None)
    print(json.dumps({"relax_to_result_us": {"n": len(relax_us), "p50": pct(relax_us, 0.5), "p90": pct(relax_us, 0.9),
                                             "max": round(max(relax_us), 2)},
                      "fresh_receive_search_us": {"n": len(fresh_us), "p50": pct(fresh_us, 0.5),
                                                  "p90": pct(fresh_us, 0.9), "max": round(max(fresh_us), 2)},
                      "relax_not_answered": skipped}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
