"""Child process of tests/test_gpu_best.py: best jobs split over two CU partitions.  Run with
NANOPOW_VIRTUAL_DEVICES=2 (two logical devices over the one physical GPU, each with its own stream, hit records and
worker): npow_submit_best of [start, start + 2^23) over both devices -- contiguous halves, as npow_submit_sweep splits
a range -- must return the oracle's argmax, each device having hashed its half; and a range cut so that its maximum
lies in the second device's part (at that part's very first nonce when the array allows) must return it too: the
fold is over devices as it is over launches.  Prints one JSON line; exits non-zero on any mismatch."""
import json
import os
import sys

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
    root, start, count = bytes(range(3, 35)), 0x0123456789abcdef, 1 << 23
    v = oracle.work_values_range(root, start, count)
    m = int(np.argmax(v))
    for d in range(G):
        eng.reset_stats(d)
    r = eng.submit_best(root, start, count, device_mask=0).wait(60)
    assert r is not None and r.status == _lib.NPOW_OK, r
    assert (r.nonce, r.value, r.nonces_done) == ((start + m) & M64, int(v[m]), count), (r, m)
    assert oracle.work_value_hashlib(root, r.nonce) == r.value
    per = [eng.stats(d).nonces for d in range(G)]
    assert per == [count // 2, count // 2], per
    # the maximum in the second device's part: [start, start + 2m) puts it at that part's first nonce
    assert m >= 1, m
    n2 = min(2 * m, count)
    r2 = eng.submit_best(root, start, n2, device_mask=0).wait(60)
    assert r2 is not None and r2.status == _lib.NPOW_OK, r2
    assert (r2.nonce, r2.value, r2.nonces_done) == ((start + m) & M64, int(v[m]), n2), (r2, m, n2)
    first_part = n2 // 2 + n2 % 2
    print(json.dumps({"ok": True, "devices": G, "nonces_per_device": per, "argmax": m,
                      "second_half": {"count": n2, "winner_in_second_part": m >= first_part},
                      "partitions": [[eng.stats(d).hip_device, eng.stats(d).cu_first, eng.stats(d).cus]
                                     for d in range(G)],
                      "affinity": [sum(eng.stats(d).affinity_checks for d in range(G)),
                                   sum(eng.stats(d).affinity_failures for d in range(G))]}), flush=True)


if __name__ == "__main__":
    main()
