"""Child process of tests/test_gpu_best_background.py: one background best job split over two CU partitions.
Run with NANOPOW_VIRTUAL_DEVICES=2 (two logical devices over the one physical GPU, each with its own stream, hit
records, claim counters, best words and worker): npow_submit_best_background of [start, start + 2^22) over both
devices with a 1-ms launch budget (each partition's half, 2^21 nonces, is well under a budget's worth: whether a
launch is cut is up to the box, and printed).  The result must be the oracle's argmax -- the fold is over devices as
it is over launches -- and the devices' nonce counters must add up to the range, each device holding its half.
Prints one JSON line; exits non-zero on any mismatch."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

import oracle  # noqa: E402
from nanopow import _lib  # noqa: E402

M64 = (1 << 64) - 1


def main():
    eng = _lib.Engine()
    G = eng.n_devices
    assert G == int(os.environ["NANOPOW_VIRTUAL_DEVICES"]) == 2, G
    root, start, count = bytes(range(3, 35)), 0x0123456789abcdef, 1 << 22
    v = oracle.work_values_range(root, start, count)
    m = int(np.argmax(v))
    for d in range(G):
        eng.reset_stats(d)
    eng.set_pool_tuning(budget_us=1000)
    t = eng.submit_best(root, start, count, device_mask=0, background=True)
    while not t.info().finished:
        time.sleep(0.001)
    i, h = t.info(), t.hold()
    r = t.wait(60)
    assert r is not None and r.status == _lib.NPOW_OK, r
    assert (r.nonce, r.value, r.nonces_done) == ((start + m) & M64, int(v[m]), count), (r, m)
    assert oracle.work_value_hashlib(root, r.nonce) == r.value
    assert h.background == 1 and i.records_max <= i.room, (i, h)
    per = [eng.stats(d).nonces for d in range(G)]
    assert per == [count // 2] * 2, per
    print(json.dumps({"ok": True, "devices": G, "nonce": f"{r.nonce:016x}", "value": f"{r.value:016x}",
                      "nonces_done": r.nonces_done, "nonces_per_device": per, "launches": i.launches,
                      "launches_cut": h.launches_cut, "held_us": h.held_us, "records_max": i.records_max,
                      "room": i.room,
                      "partitions": [[eng.stats(d).hip_device, eng.stats(d).cu_first, eng.stats(d).cus]
                                     for d in range(G)],
                      "affinity": [sum(eng.stats(d).affinity_checks for d in range(G)),
                                   sum(eng.stats(d).affinity_failures for d in range(G))]}), flush=True)


if __name__ == "__main__":
    main()
