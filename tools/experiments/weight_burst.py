#!/usr/bin/env python3
"""A burst of concurrent searches through the work pool on GPU 0, for A/B runs of the pool's entry choice.

Submits --n fresh roots at once at the send threshold (64 live per launch, the rest waiting), waits for all of
them, validates every result on the CPU and prints one JSON line: the device's hash rate over its kernel time, the
wall time and the early-finish / dynamic-entry counters.  --heavy-every K gives every K-th job weight 8 (needs a
library with npow_submit_weighted); the default is the unweighted pool.  NANOPOW_LIB selects the library.

    python tools/experiments/weight_burst.py [--n 256] [--heavy-every 0] [--tag NAME]
"""
import argparse
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

SEND = 0xfffffff800000000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--heavy-every", type=int, default=0)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    eng = _lib.engine()
    roots = [hashlib.blake2b(b"weight-burst" + i.to_bytes(8, "little"), digest_size=32).digest() for i in range(a.n)]
    warm = eng.search(bytes(32), 0xfffffe0000000000, device_mask=1)  # the first launch's one-off costs
    assert warm.status == _lib.NPOW_OK
    eng.reset_stats(0)
    t0 = time.perf_counter()
    tickets = []
    for i, r in enumerate(roots):
        kw = {"weight": 8} if a.heavy_every and i % a.heavy_every == 0 else {}
        tickets.append(eng.submit(r, SEND, start=i << 48, device_mask=1, **kw))
    done = 0
    for r, t in zip(roots, tickets):
        res = t.wait(120)
        assert res is not None and res.status == _lib.NPOW_OK, res
        assert eng.work_value(r, res.nonce) == res.value >= SEND
        done += res.nonces_done
    wall = time.perf_counter() - t0
    st = eng.stats(0)
    print(json.dumps({"tag": a.tag, "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "abi": eng.abi_version(), "n": a.n,
                      "heavy_every": a.heavy_every, "wall_s": round(wall, 4), "nonces": done,
                      "kernel_ms": round(st.kernel_ms, 3),
                      "gnonce_per_s_kernel": round(st.nonces / st.kernel_ms * 1e-6, 4) if st.kernel_ms else None,
                      "gnonce_per_s_wall": round(done / wall * 1e-9, 4), "clock_mhz": round(st.clock_mhz, 1),
                      "early_finishes": st.early_finishes, "early_mismatches": st.early_mismatches,
                      "dyn_entries": st.dyn_entries, "yields": st.yields}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
