"""Child process of tests/test_gpu_sweep_jobs.py: one sweep job split over G CU partitions.  Run with
NANOPOW_VIRTUAL_DEVICES=G (G logical devices over the one physical GPU, each with its own stream, hit
records and worker): npow_submit_sweep of [start, start + 2^22 + 3) at ffff000000000000 over every device
-- contiguous parts that differ in length by one (npow_pool_jobs.cpp submit_collecting), so hits lie on both
sides of every boundary the split cuts.  The merged hit set must equal the C oracle's and the devices'
nonce counters must add up to the range, each device holding its part.  Prints one JSON line; exits
non-zero on any mismatch."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle  # noqa: E402
from nanopow import _lib  # noqa: E402


def main():
    eng = _lib.Engine()
    G = eng.n_devices
    assert G == int(os.environ["NANOPOW_VIRTUAL_DEVICES"]), G
    root, thr = bytes(range(3, 35)), 0xffff000000000000
    start, count = 0xfedcba9876543211, (1 << 22) + 3
    for d in range(G):
        eng.reset_stats(d)
    r = eng.submit_sweep(root, thr, start, count, device_mask=0).wait(60)
    want = oracle.sweep(root, thr, start, count, threads=min(16, os.cpu_count() or 1))
    assert r is not None and r.status == _lib.NPOW_OK, r
    assert r.hits == want, (len(r.hits), len(want), sorted(set(r.hits) ^ set(want))[:8])
    assert r.total == len(want) and r.nonces_done == count
    per = [eng.stats(d).nonces for d in range(G)]
    share = [count // G + (1 if d < count % G else 0) for d in range(G)]
    assert per == share, (per, share)
    print(json.dumps({"ok": True, "devices": G, "hits": len(r.hits), "nonces_done": r.nonces_done,
                      "nonces_per_device": per,
                      "partitions": [[eng.stats(d).hip_device, eng.stats(d).cu_first, eng.stats(d).cus]
                                     for d in range(G)],
                      "affinity": [sum(eng.stats(d).affinity_checks for d in range(G)),
                                   sum(eng.stats(d).affinity_failures for d in range(G))]}), flush=True)


if __name__ == "__main__":
    main()
