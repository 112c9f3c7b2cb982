"""The flows of tests/test_gpu_search_positions.py, and that file's child process (the engine reads its environment
once).  As a program: NANOPOW_VIRTUAL_DEVICES=2, the sole-hit searches (tests/search_positions.py) on CU partition 1
alone -- its own grid, its own window -- and split over both partitions, where partition 1's stride starts at
start + 2^63 (npow_pool_jobs.cpp pool_submit).  One JSON line on stdout; every check that failed is listed in it."""
import contextlib
import json
import os
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))
sys.path.insert(0, HERE)

import search_positions as sp  # noqa: E402
from nanopow import _lib  # noqa: E402

M64 = sp.M64
COUNTERS = ("yields", "dyn_entries", "invalid_work")


@contextlib.contextmanager
def tuned(eng):
    """16 wave iterations per launch -- well under a millisecond -- and a time budget that no such launch reaches, so
    every launch covers its whole window; restored afterwards."""
    eng.set_tuning(sp.TUNING)
    eng.set_pool_tuning(budget_us=400000)
    try:
        yield
    finally:
        eng.pool_config(64)
        eng.set_pool_tuning(budget_us=20000)
        eng.set_tuning(8192)


def whole_window_device(eng, dev, partition):
    """The device's grid, once it is known to start every one-entry search at block 0 of a launch of its own: no
    lingering launches (npow_pool.cpp lingers(): CU partitions of up to 32 CUs), which would take the search as a
    dynamic entry at each workgroup's current iteration."""
    st = eng.stats(dev)
    assert (st.cu_first >= 0) == partition and st.cus > 32, (st.cu_first, st.cus)
    assert not os.environ.get("NANOPOW_LINGER")
    return st.grid


def counters(eng, devices):
    return [{k: getattr(eng.stats(d), k) for k in COUNTERS} for d in devices]


def sole_search(eng, sh, pos, mask=1, start_shift=0, threshold=None):
    """One unbounded search whose first window has its only hit at `pos`.  Returns what went wrong, or None.
    threshold: another one that h alone meets, in (sh.second, value(h)] (tests/threshold_ladder.py); the search must
    still return h with value(h)."""
    T = sh.threshold if threshold is None else threshold
    assert sh.second < T <= sh.threshold
    t = eng.submit(sh.root, T, start=(sp.start_of(sh, pos) - start_shift) & M64, device_mask=mask)
    info = t.wait_info(60)
    if info is None:
        t.cancel()
        t.wait(30)
        return {"pos": pos, "coords": sp.coords_of(pos, sh.grid), "error": "no result within 60 s"}
    ok = (info.status == _lib.NPOW_OK and info.nonce == sh.h and info.value == sh.threshold and
          0 < info.nonces_done <= sh.full * info.n_devices and info.nonces_done % 64 == 0)
    if ok:
        return None
    return {"anchor": sh.anchor, "pos": pos, "coords": sp.coords_of(pos, sh.grid), "T": f"{T:016x}",
            "status": info.status, "nonce": f"{info.nonce:016x}", "want": f"{sh.h:016x}", "value": f"{info.value:016x}",
            "nonces_done": info.nonces_done, "winner_device": info.winner_device}


def copies_in_one_table(eng, sh, pos, n, hold_root, threshold=None, reserve=None, watch=None):
    """n identical searches adopted into ONE table of exactly those n entries (device 0).  A legacy sweep of 2^33
    nonces holds the device meanwhile (npow_host.h TaskLock; ~0.25 s): the pool worker adopts the first search when
    it is submitted, then waits for the device's lock (Worker::run); when the sweep returns, Worker::step adopts the
    others -- nothing is in flight, so none becomes a dynamic entry and nothing is yielded (Worker::adopt, dyn_add,
    yield_if_long) -- and Worker::launch builds one table of every active slot (build_table).  The sweep is known to
    hold the lock once one of its launches has retired, and to have held it through the last submit if it still
    runs then.  threshold: the copies' threshold where it is not value(h).  Returns (results, counter deltas).
    reserve: the copies' reserve threshold (tests/reserve_exact_worker.py); watch(tickets) is then called once the
    sweep has returned and all n are submitted -- it must leave every copy decided or cancelled -- and what it returns
    is the third item of the result."""
    T = sh.threshold if threshold is None else threshold
    kw = {} if reserve is None else {"reserve": reserve}
    watched = None
    before = eng.stats(0)
    th = threading.Thread(target=eng.sweep_result, args=(hold_root, M64, 1 << 50, 1 << 33), kwargs={"device_mask": 1})
    th.start()
    tickets = []
    try:
        deadline = time.monotonic() + 20
        while eng.stats(0).launches == before.launches:
            assert time.monotonic() < deadline and th.is_alive(), "the sweep that holds the device never started"
            time.sleep(0.0005)
        c0 = counters(eng, [0])[0]
        tickets = [eng.submit(sh.root, T, start=sp.start_of(sh, pos), device_mask=1, **kw) for _ in range(n)]
        held = th.is_alive()
    finally:
        th.join()
        try:
            if watch is not None and len(tickets) == n:
                watched = watch(tickets)
        except BaseException:
            for t in tickets:
                t.cancel()  # (a watch that failed half-way leaves no endless copy behind)
            raise
        finally:
            deadline = time.monotonic() + 30  # (for all of them: a copy that has not ended then is cancelled)
            results = [t.wait(max(0.0, deadline - time.monotonic())) for t in tickets]
            for t, r in zip(tickets, results):
                if r is None:
                    t.cancel()
                    t.wait(30)
    assert held, "the sweep ended before the last search was submitted"
    c1 = counters(eng, [0])[0]
    deltas = {k: c1[k] - c0[k] for k in COUNTERS}
    return (results, deltas) if watch is None else (results, deltas, watched)


def main():
    import oracle
    eng = _lib.Engine()
    assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    t0 = time.monotonic()
    grids = [whole_window_device(eng, d, True) for d in range(2)]
    grid = grids[1]
    failures, alone, split = [], 0, []
    with tuned(eng):
        c0 = counters(eng, [0, 1])
        for anchor in sp.ANCHORS:
            sh = sp.sole_hit(grid, anchor)
            # partition 1 alone: the corners and every fourth lane position, and a carry anchor's first crossing
            ps = sp.corners(grid) + sp.lane_positions(grid)[::4] + ([] if sh.boundary is None else [sp.first_carry(sh)])
            for pos in ps:
                bad = sole_search(eng, sh, pos, mask=2)
                alone += 1
                if bad:
                    failures.append(dict(bad, mask=2))
        # both partitions: the hit in partition 1's stride, and nothing at or above T in partition 0's first launches
        sh = sp.sole_hit(grid, "plain")
        F0 = sp.full(grids[0])
        tried = 0
        for pos in sp.corners(grid)[5::3] + sp.lane_positions(grid)[1::5]:
            if len(split) == 4 or tried == 8:
                break
            tried += 1
            start = (sp.start_of(sh, pos) - (1 << 63)) & M64
            if oracle.sweep(sh.root, sh.threshold, start, 4 * F0):
                continue
            t = eng.submit(sh.root, sh.threshold, start=start, device_mask=3)
            info = t.wait_info(60)
            rec = {"pos": pos, "coords": sp.coords_of(pos, grid), "status": info.status, "nonce": f"{info.nonce:016x}",
                   "winner_device": info.winner_device, "nonces_done": info.nonces_done}
            split.append(rec)
            if not (info.status == _lib.NPOW_OK and info.nonce == sh.h and info.value == sh.threshold and
                    info.winner_device == 1):
                failures.append(dict(rec, mask=3, want=f"{sh.h:016x}"))
        c1 = counters(eng, [0, 1])
    print(json.dumps({"n_devices": eng.n_devices, "grids": grids, "alone": alone, "split": split, "failures": failures,
                      "deltas": [{k: b[k] - a[k] for k in COUNTERS} for a, b in zip(c0, c1)],
                      "seconds": round(time.monotonic() - t0, 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
