"""Child process of tests/test_gpu_weights.py: a crowded weighted table on a CU partition.  Run with
NANOPOW_VIRTUAL_DEVICES=8: logical device 0 is 32 CUs, a grid of 128 workgroups.  Twenty endless jobs of weight 8 and
one of weight 1 on that device: their weights sum to 161, more than the grid, so the table builder halves them
(nano-dpow_amd/csrc/npow_weights.h) and every job's run of the start map holds a workgroup.  Prints one JSON line
with every job's nonce count."""
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

M64 = (1 << 64) - 1


def main():
    eng = _lib.Engine()
    assert eng.n_devices == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    grid = eng.stats(0).grid
    rng = random.Random(77)
    weights = [8] * 20 + [1]
    toks = [_lib.CancelToken() for _ in weights]
    tickets = [eng.submit(bytes(rng.getrandbits(8) for _ in range(32)), M64, start=(i + 1) << 52, device_mask=1,
                          cancel=c, weight=w) for i, (w, c) in enumerate(zip(weights, toks))]
    time.sleep(0.25)
    for c in toks:
        c.set()
    done = []
    for t in tickets:
        res = t.wait(30)
        assert res is not None and res.status == _lib.NPOW_CANCELLED
        done.append(res.nonces_done)
    st = eng.stats(0)
    print(json.dumps({"grid": grid, "weights": weights, "nonces": done, "early_mismatches": st.early_mismatches,
                      "stale_missing": st.stale_missing}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
