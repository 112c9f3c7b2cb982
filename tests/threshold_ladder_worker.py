"""The flows of tests/test_gpu_threshold_ladder.py, and that file's child process (the engine reads its environment
once).  As a program: NANOPOW_VIRTUAL_DEVICES=2, the one-entry ladder (tests/threshold_ladder.py) on CU partition 1
alone with that grid's own sole hits, and one range's sweep-job and best-job ladders split over both partitions.  One
JSON line on stdout; every check that failed is listed in it.

Every expectation comes from the oracle and hashlib (threshold_ladder), none from the library, and every comparison of a
value with a threshold here is Python's int comparison."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))
sys.path.insert(0, HERE)

import search_position_worker as spw  # noqa: E402
import search_positions as sp  # noqa: E402
import threshold_ladder as tl  # noqa: E402
from nanopow import _lib  # noqa: E402
from oracle import work_value_hashlib  # noqa: E402

M64 = sp.M64
SWEEP_KINDS = ("blocking", "plain", "background", "shared")
BEST_KINDS = ("plain", "background", "shared")
_CLASS = {"plain": {}, "background": {"background": True}, "shared": {"shared": True}}


def later_search(eng, sh, pos, T, mask=1):
    """One unbounded search from h - pos at a threshold above value(h): nothing in its first window qualifies, so it
    must return a later nonce whose hashlib value is at or above T.  Returns what went wrong, or None."""
    assert T > sh.threshold
    t = eng.submit(sh.root, T, start=sp.start_of(sh, pos), device_mask=mask)
    info = t.wait_info(60)
    if info is None:
        t.cancel()
        t.wait(30)
        return {"anchor": sh.anchor, "pos": pos, "T": f"{T:016x}", "error": "no result within 60 s"}
    if (info.status == _lib.NPOW_OK and info.nonce != sh.h and
            work_value_hashlib(sh.root, info.nonce) == int(info.value) >= T):
        return None
    return {"anchor": sh.anchor, "pos": pos, "T": f"{T:016x}", "status": info.status, "nonce": f"{info.nonce:016x}",
            "h": f"{sh.h:016x}", "value": f"{info.value:016x}", "nonces_done": info.nonces_done}


def one_entry_ladder(eng, w, positions, mask=1):
    """Every rung of the window's m1 with h at each of the positions, one search at a time (a one-entry launch).
    [failures], each named by its rung."""
    failures = []
    for r in w.rungs:
        for pos in positions:
            bad = (spw.sole_search(eng, w.sh, pos, mask=mask, threshold=r.T) if r.meets else
                   later_search(eng, w.sh, pos, r.T, mask=mask))
            if bad:
                failures.append(dict(bad, rung=r.name, meets=r.meets))
    return failures


def sweep_ladder(eng, rl, kind, mask=1):
    """The range enumerated at every rung of its top three values: the blocking npow_sweep one call at a time, the
    jobs of a class submitted together.  [failures]."""
    rungs = tl.range_rungs(rl)
    if kind == "blocking":
        got = []
        for _, r in rungs:
            res = eng.sweep_result(rl.root, r.T, rl.start, rl.count, device_mask=mask)
            got.append((res.status, res.hits, res.total, rl.count))
    else:
        ts = [eng.submit_sweep(rl.root, r.T, rl.start, rl.count, device_mask=mask, **_CLASS[kind]) for _, r in rungs]
        got = []
        for t in ts:
            res = t.wait(60)
            if res is None:
                t.cancel()
                t.wait(30)
                got.append((None, [], 0, 0))
            else:
                got.append((res.status, res.hits, res.total, res.nonces_done))
    failures = []
    for (i, r), (status, hits, total, done) in zip(rungs, got):
        want = tl.expected_hits(rl, r.T)
        if not (status == _lib.NPOW_OK and hits == want and total == len(want) and done == rl.count):
            failures.append({"range": rl.name, "kind": kind, "value": i, "rung": r.name, "T": f"{r.T:016x}",
                             "status": status, "hits": [f"{h:016x}" for h in hits[:8]], "n_out": total,
                             "want": [f"{h:016x}" for h in want], "nonces_done": done})
    return failures


def best_ladder(eng, rl, kind, mask=1):
    """Best jobs of one class over the range, submitted together: the floor at every rung of the maximum -- the
    maximum, or exhausted with every nonce counted -- and at every rung of the second value: the maximum every time.
    [failures]."""
    (off, top), (_, second) = rl.top[0], rl.top[1]
    argmax = (rl.start + off) & M64
    floors = [(0, r) for r in tl.rungs(top)] + [(1, r) for r in tl.rungs(second)]
    ts = [eng.submit_best(rl.root, rl.start, rl.count, floor=r.T, device_mask=mask, **_CLASS[kind]) for _, r in floors]
    failures = []
    for (i, r), t in zip(floors, ts):
        res = t.wait(60)
        if res is None:
            t.cancel()
            t.wait(30)
        found = tl.best_of(rl, r.T)
        assert (found is not None) == (r.meets if i == 0 else True)
        if found is not None:
            ok = res is not None and tuple(res) == (_lib.NPOW_OK, argmax, top, rl.count)
        else:
            ok = res is not None and res.status == _lib.NPOW_EXHAUSTED and res.nonces_done == rl.count
        if not ok:
            failures.append({"range": rl.name, "kind": kind, "value": i, "rung": r.name, "floor": f"{r.T:016x}",
                             "result": None if res is None else [res.status, res.nonce and f"{res.nonce:016x}",
                                                                 res.value and f"{res.value:016x}", res.nonces_done],
                             "want": found and [f"{found[0]:016x}", f"{found[1]:016x}"]})
    return failures


def main():
    eng = _lib.Engine()
    assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    t0 = time.monotonic()
    grids = [spw.whole_window_device(eng, d, True) for d in range(2)]
    ws = tl.window_ladders(grids[1])
    rl = tl.range_ladders()[2]  # the ragged range across 2^64
    t1 = time.monotonic()
    failures, alone = [], 0
    with spw.tuned(eng):
        c0 = spw.counters(eng, [0, 1])
        for w in ws.values():
            ps = (0, w.sh.full - 1)
            failures += [dict(f, mask=2) for f in one_entry_ladder(eng, w, ps, mask=2)]
            alone += len(w.rungs) * len(ps)
        c1 = spw.counters(eng, [0, 1])
    split = 0
    for kind in ("plain", "background", "shared"):
        failures += [dict(f, mask=3) for f in sweep_ladder(eng, rl, kind, mask=3)]
        failures += [dict(f, mask=3) for f in best_ladder(eng, rl, kind, mask=3)]
        split += 8 * tl.LADDERED + 16
    print(json.dumps({"n_devices": eng.n_devices, "grids": grids, "alone": alone, "split": split, "failures": failures,
                      "bit31": sorted({tl.bit31(w.m1) for w in ws.values()}),
                      "deltas": [{k: b[k] - a[k] for k in spw.COUNTERS} for a, b in zip(c0, c1)],
                      "oracle_seconds": round(t1 - t0, 2), "gpu_seconds": round(time.monotonic() - t1, 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
