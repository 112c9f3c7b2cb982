"""Child process of tests/test_gpu_crowded_tables.py: crowded tables on one 32-CU partition.  Run with
NANOPOW_VIRTUAL_DEVICES=8; everything goes to device 0 (device_mask 1), whose launches have G = 128 workgroups, so a
bounded entry of a table of 17, 48, 63 or 64 has 8 / 7, 3 / 2, 3 / 2 or 2 of them.  The scenarios are those of
tests/crowded_tables.py: sweep jobs beside a best job (the witness of the launch's regions), bounded first-win
searches (the pigeonhole on the launch counter), and sweep jobs stitched over launches of one wave iteration at
n = 64.  Prints one JSON line; exits non-zero on any mismatch."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import crowded_tables as ct  # noqa: E402
from nanopow import _lib  # noqa: E402

SIZES = [17, 48, 63, 64]


def main():
    eng = _lib.Engine()
    assert eng.n_devices == int(os.environ["NANOPOW_VIRTUAL_DEVICES"]) == 8, eng.n_devices
    grid = eng.stats(0).grid
    assert grid == 128 and eng.stats(0).cus == 32, (grid, eng.stats(0).cus)
    groups = [[grid // n + (1 if e < grid % n else 0) for e in (0, n - 1)] for n in SIZES]
    assert groups == [[8, 7], [3, 2], [3, 2], [2, 2]], groups
    sweeps = [ct.sweep_table(eng, n, ct.QUARTER, seed=700 + n) for n in SIZES]
    searches = [ct.search_table(eng, n, seed=800 + n) for n in SIZES]
    stitching = ct.stitch_table(eng, 64, seed=900)
    st = eng.stats(0)
    assert (st.invalid_work, st.early_mismatches, st.stale_missing) == (0, 0, 0), st
    print(json.dumps({"ok": True, "grid": grid, "groups": groups, "sweeps": sweeps, "searches": searches,
                      "stitching": stitching}), flush=True)


if __name__ == "__main__":
    main()
