"""The flows of tests/test_gpu_reserve_exact.py, and that file's child process (the engine reads its environment once).
As a program: NANOPOW_VIRTUAL_DEVICES=2, the sole-candidate flow on CU partition 1 alone (device_mask 2: its own grid,
its own window, the search starts at S itself) at the corners and every fourth lane position.  One JSON line on
stdout; every check that failed is listed in it.

The construction is tests/reserve_records.py: a record h of the 2^36 fixture, a search started at S = h - pos, so that
the first launch holds h at a chosen (iteration, workgroup, wave, lane), and Z nonces after h in which nothing can
displace it.  No flow waits a guessed time: each polls Ticket.reserve() against a deadline and gives up early only on
the device's `launches` counter, which steps as a launch retires (npow_pool.cpp Worker::retire_launches calls
account_launch, npow_engine.cpp `d.launches++;`) -- launches retire in order and at most two are in flight, so once
it has grown by BEHIND = 4 since before the submit, at least two launches of this search have retired and the first,
which covers h, lies behind.  (The device's `nonces` counter does not serve: Worker::credit_counts, `d_.nonces +=
c.done;`, credits a slot's count when the slot retires, so it stands still under a search that runs on.)"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))
sys.path.insert(0, HERE)

import reserve_records as rr  # noqa: E402
import search_position_worker as spw  # noqa: E402
import search_positions as sp  # noqa: E402
from nanopow import _lib  # noqa: E402

M64 = rr.M64
DEADLINE_S = 10
BEHIND = 4  # retired launches since before a submit after which the search's first launch is one of them


def pick(F):
    """Two records of the fixture for the window length F: the one with the longest quiet stretch after it (Z = 2^34
    if any record has it, else 2^33), and another whose high word differs from the first's if there is one.  Both
    have a low word that decides v against v - 1 and v + 1."""
    hits = rr.fixture()[1]
    r33 = [h for h in rr.records(F, rr.Z33) if rr.low_word_decides(hits[h])]
    r34 = [h for h in rr.records(F, rr.Z34) if rr.low_word_decides(hits[h])]
    assert len(r33) >= 3, "the fixture has too few records for this grid"
    first = (r34 or r33)[0]
    others = [h for h in r33 if h != first]
    second = next((h for h in others if hits[h] >> 32 != hits[first] >> 32), others[0])
    return first, second


def stretch(h, F):
    return rr.Z34 if h in rr.records(F, rr.Z34) else rr.Z33


def end(t, timeout=30):
    """Cancel and collect a ticket that a failed check may have left running."""
    if t is not None and t.result is None:
        t.cancel()
        t.wait(timeout)


def poll_for(eng, t, h, allowed, dev, launches0):
    """Ticket.reserve() until it holds h.  Returns (seen, why): seen the distinct (nonce, value) pairs in the order
    read, why None or what ended the polling otherwise -- a pair outside `allowed`, the deadline, or the device's
    launches counter BEHIND on with h still missing (read once more after the counter: the record of a launch is in
    pinned memory before the launch retires)."""
    seen = []
    deadline = time.monotonic() + DEADLINE_S
    behind = False
    while True:
        r = t.reserve()
        if r is not None:
            pair = (r.nonce, r.value)
            if not seen or seen[-1] != pair:
                seen.append(pair)
            if r.nonce == h:
                return seen, None
            if allowed.get(r.nonce) != r.value:
                return seen, f"{r.nonce:x} {r.value:016x} is no candidate of the first window"
        if behind:
            return seen, "the first launch has retired and the reserve does not hold h"
        if time.monotonic() >= deadline:
            return seen, f"no reserve with h within {DEADLINE_S} s"
        behind = eng.stats(dev).launches - launches0 >= BEHIND
        if not behind:
            time.sleep(0.0002)


def exact_one(eng, h, pos, grid, T, R, dev=0):
    """One search of the fixture root from S = h - pos at threshold T with the reserve threshold R <= v(h) < T, on
    device `dev` alone.  Returns None, or a record of what went wrong."""
    root, hits = rr.fixture()
    v, F = hits[h], sp.full(grid)
    S = h - pos
    assert 0 <= pos < F and 0 <= S and S + F <= rr.END and R <= v < T
    allowed = {n: x for n, x in rr.window_hits(S, F).items() if R <= x < T}
    assert allowed[h] == v and max(allowed.values()) == v
    bad, t, seen = [], None, []
    launches0 = eng.stats(dev).launches
    try:
        t = eng.submit(root, T, start=S, device_mask=1 << dev, reserve=R)
        seen, why = poll_for(eng, t, h, allowed, dev, launches0)
        if why:
            bad.append(why)
        else:
            if seen[-1] != (h, v):
                bad.append("the reserve holds h with another value")
            if [x for _, x in seen] != sorted(x for _, x in seen):
                bad.append("the reserve's value decreased")
            if len(allowed) == 1 and seen != [(h, v)]:
                bad.append("the first reserve was not h")
            if T == M64 and t.relax(v + 1) is not False:
                bad.append("relax(v + 1) was not lowered in place")
            if t.wait_result(0) is not None:
                bad.append("the search was decided above v(h)")
            if t.relax(v) is not True:
                bad.append("relax(v) was not answered at once")
            res = t.wait_result(0)
            if res is None or (res.status, res.nonce, res.value) != (_lib.NPOW_OK, h, v):
                bad.append(f"wait_result(0) after the answer: {res}")
            ri = t.reserve_info()
            if (ri.answered, ri.nonce, ri.value, ri.device) != (1, h, v, dev):
                bad.append(f"reserve_info: answered {ri.answered} nonce {ri.nonce:x} value {ri.value:016x} device "
                           f"{ri.device} candidates {ri.candidates}")
            info = t.wait_info(30)
            if info is None or (info.status, info.nonce, info.value, info.stale_hits, info.stale_wins) != \
                    (_lib.NPOW_OK, h, v, 0, 0):
                bad.append("wait_info: " + ("nothing within 30 s" if info is None else
                                            f"status {info.status} nonce {info.nonce:x} value {info.value:016x} "
                                            f"stale_hits {info.stale_hits} stale_wins {info.stale_wins}"))
            elif not 0 < info.nonces_done < stretch(h, F):
                bad.append(f"nonces_done {info.nonces_done}: the search left the stretch in which h is the record")
    finally:
        end(t)
    if not bad:
        return None
    return {"h": f"{h:x}", "pos": pos, "coords": sp.coords_of(pos, grid), "T": f"{T:016x}", "R": f"{R:016x}",
            "seen": [(f"{n:x}", f"{x:016x}") for n, x in seen], "bad": bad}


def exact_many(eng, h, positions, grid, rungs, dev=0):
    """exact_one over positions x rungs under search_position_worker.tuned().  Returns (searches, failures, counter
    deltas of the device)."""
    failures, n = [], 0
    with spw.tuned(eng):
        c0 = spw.counters(eng, [dev])[0]
        for rung in rungs:
            assert rung.candidate
            for pos in positions:
                bad = exact_one(eng, h, pos, grid, rung.T, rung.R, dev)
                n += 1
                if bad:
                    failures.append(dict(bad, rung=rung.name))
        c1 = spw.counters(eng, [dev])[0]
    return n, failures, {k: c1[k] - c0[k] for k in spw.COUNTERS}


def not_a_candidate(eng, h, pos, grid, dev=0):
    """T = 2^64 - 1, R = v(h) + 1: h is hashed in the first launch and must not be filed.  The host would drop a wrong
    record (pool_harvest_locked recomputes it), so `candidates` -- every record the host has read -- is the witness.
    Returns plain numbers."""
    root, hits = rr.fixture()
    v, F = hits[h], sp.full(grid)
    t = None
    with spw.tuned(eng):
        c0 = spw.counters(eng, [dev])[0]
        launches0 = eng.stats(dev).launches
        try:
            t = eng.submit(root, M64, start=h - pos, device_mask=1 << dev, reserve=v + 1)
            deadline = time.monotonic() + DEADLINE_S
            while eng.stats(dev).launches - launches0 < BEHIND:
                assert time.monotonic() < deadline, "the device's launches counter does not move"
                time.sleep(0.0002)
            ri = t.reserve_info()
            t.cancel()
            info = t.wait_info(30)
        finally:
            end(t)
        c1 = spw.counters(eng, [dev])[0]
    return {"candidates": ri.candidates, "value": ri.value, "nonce": ri.nonce, "status": info.status,
            "nonces_done": info.nonces_done, "F": F, "Z": stretch(h, F), "stale_hits": info.stale_hits,
            "deltas": {k: c1[k] - c0[k] for k in spw.COUNTERS}}


def copies(eng, h, pos, grid, n, hold_root):
    """n copies of one search (T = 2^64 - 1, R = v(h)) in one table of n entries
    (search_position_worker.copies_in_one_table).  Each copy hashes the blocks of its own workgroups only, so one copy
    alone passes h.  Returns plain numbers."""
    root, hits = rr.fixture()
    v, F = hits[h], sp.full(grid)
    sh = sp.SoleHit(grid, "fixture", None, root, None, h, v, F, None, None)
    out = {}

    def watch(tickets):
        deadline = time.monotonic() + DEADLINE_S
        infos = []
        while time.monotonic() < deadline:
            infos = [t.reserve_info() for t in tickets]
            if any(i.value for i in infos):
                infos = [t.reserve_info() for t in tickets]  # (every copy, after the first one was seen to hold one)
                break
            time.sleep(0.0002)
        out["reserves"] = [(i.nonce, i.value) for i in infos]
        out["candidates"] = [i.candidates for i in infos]
        holders = [k for k, i in enumerate(infos) if (i.nonce, i.value) == (h, v)]
        out["holders"] = holders
        if len(holders) == 1:
            t = tickets[holders[0]]
            out["answered"] = t.relax(v)
            res = t.wait_result(0)
            out["at_once"] = None if res is None else (res.status, res.nonce, res.value)
        for k, t in enumerate(tickets):
            if holders != [k] or out.get("answered") is not True:
                t.cancel()

    results, deltas, _ = spw.copies_in_one_table(eng, sh, pos, n, hold_root, threshold=M64, reserve=v, watch=watch)
    out["results"] = [None if r is None else (r.status, r.nonce, r.value, r.nonces_done) for r in results]
    out["deltas"] = deltas
    return out


def partition_positions(grid):
    return sp.corners(grid) + sp.lane_positions(grid)[::4]


def main():
    eng = _lib.Engine()
    assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    t0 = time.monotonic()
    grids = [spw.whole_window_device(eng, d, True) for d in range(2)]
    grid = grids[1]
    h, _ = pick(sp.full(grid))
    n, failures, deltas = exact_many(eng, h, partition_positions(grid), grid, rr.ladder(h)[:1], dev=1)
    print(json.dumps({"n_devices": eng.n_devices, "grids": grids, "h": f"{h:x}", "searches": n, "failures": failures,
                      "deltas": deltas, "seconds": round(time.monotonic() - t0, 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
