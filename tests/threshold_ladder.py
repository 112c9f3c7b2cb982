"""Thresholds whose low 32 bits decide (pure Python and the oracle: no GPU here).

Every result of the engine hangs on one 64-bit comparison, `value >= threshold` (npow_kernel.hip: `bool hit = value >=
thr;` in pool_body_ls2, `value >= cur` and `value >= ethr` in its hit branch, the ballot of npow_sweep_kernel_ls2).
rungs(v) places thresholds around a value v, inside v's own high word, so that each of these wrong comparisons gives a
wrong answer on at least one of them (WRONG below; tests/test_threshold_ladder_cpu.py shows it):

    high words only            the low words compared as signed integers
    both words required >=     > where >= is meant

Whether v meets a rung is worked out with Python's int comparison alone.  (A numpy uint64 compared with a Python integer
above 2^63 can pass through float64 on some numpy versions, which loses exactly the bits these tests are about; values
of one uint64 array are only ever compared with each other here.)

Two users.  Windows: the sole hit of tests/search_positions.py -- the maximum m1 of 3 F values stands far above the
second value m2, so any T in (m2, m1] keeps h the only hit of every window that holds it and any T above m1 leaves
none.  Ranges: the top three values of three ranges of 2^20 nonces of one root; the expected hit list of a threshold is
every nonce of the range whose value is >= T, ascending by nonce - start.
"""
import functools
import heapq
import os
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import oracle  # noqa: E402  (the checker)
import search_positions as sp  # noqa: E402

M64 = sp.M64
LO = 0xffffffff
NAMES = ("eq", "below", "above", "flip31", "lo0", "lomax", "hi-1", "hi+1")

Rung = namedtuple("Rung", "name T meets")
WindowLadder = namedtuple("WindowLadder", "sh m1 m2 rungs")
RangeLadder = namedtuple("RangeLadder", "name root start count top")  # top: four (offset, value), descending


def rungs(v):
    """The named thresholds around v, each with whether v meets it (`v >= T` on Python ints)."""
    assert 0 < v < M64
    hi, lo = v >> 32, v & LO
    assert 0 < hi < LO, hex(v)  # (hi-1 and hi+1 stay inside 64 bits)
    ts = (("eq", v), ("below", v - 1), ("above", v + 1), ("flip31", v ^ 0x80000000), ("lo0", hi << 32),
          ("lomax", (hi << 32) | LO), ("hi-1", ((hi - 1) << 32) | LO), ("hi+1", (hi + 1) << 32))
    assert tuple(n for n, _ in ts) == NAMES and all(0 <= t <= M64 for _, t in ts)
    return [Rung(n, t, v >= t) for n, t in ts]


def rung(v, name):
    return rungs(v)[NAMES.index(name)]


def bit31(v):
    return bool(v & 0x80000000)


def conditions(v, w):
    """What the ladder of v needs, w the next lower value of the window or range: None, or what is missing.  With
    v.hi - w.hi >= 2 every rung that v meets lies above w; with v.lo neither 0 nor ffffffff the rungs lo0, lomax and eq
    are three thresholds."""
    if (v >> 32) - (w >> 32) < 2:
        return f"{v:016x} stands less than two high words above {w:016x}"
    if v >> 32 >= LO:
        return f"the high word of {v:016x} is ffffffff"
    if v & LO in (0, LO):
        return f"the low word of {v:016x} is 0 or ffffffff"
    return None


def mixed(values):
    """Bit 31 set in one of the values and clear in another: flip31, lo0 and lomax then work in both directions."""
    return len({bit31(v) for v in values}) == 2


# ---- windows -------------------------------------------------------------------------------------------------
def _window(grid, anchor, first_seed=0, want_bit31=None):
    # (seed 0 on: the call the position tests make, so a process pays for each oracle run once)
    sh = sp.sole_hit(grid, anchor) if first_seed == 0 else sp.sole_hit(grid, anchor, sp.ITERS, first_seed)
    while conditions(sh.threshold, sh.second) or (want_bit31 is not None and bit31(sh.threshold) != want_bit31):
        sh = sp.sole_hit(grid, anchor, sp.ITERS, sh.seed + 1)  # (raises past search_positions.MAX_SEEDS)
    return sh


@functools.lru_cache(maxsize=None)
def window_ladders(grid):
    """{anchor: WindowLadder} of the grid's three sole hits: each the first seed that holds the conditions, and, where
    all three have the same bit 31, the last anchor moved on to the first seed with the other one."""
    shs = {a: _window(grid, a) for a in sp.ANCHORS}
    if not mixed([sh.threshold for sh in shs.values()]):
        a = sp.ANCHORS[-1]
        shs[a] = _window(grid, a, shs[a].seed + 1, not bit31(shs[a].threshold))
    out = {}
    for a, sh in shs.items():
        m1, m2 = sh.threshold, sh.second
        assert conditions(m1, m2) is None and m2 < m1 == oracle.work_value_hashlib(sh.root, sh.h)
        rs = rungs(m1)
        assert all(r.T > m2 for r in rs if r.meets) and all(r.T > m1 for r in rs if not r.meets)
        out[a] = WindowLadder(sh, m1, m2, rs)
    assert mixed([w.m1 for w in out.values()])
    return out


def two_anchors(grid):
    """Two of the grid's ladders, one with bit 31 of m1 set and one with it clear (the plain anchor first)."""
    ws = list(window_ladders(grid).values())
    other = next(w for w in ws[1:] if bit31(w.m1) != bit31(ws[0].m1))
    return [ws[0], other]


# ---- ranges --------------------------------------------------------------------------------------------------
COUNT = 1 << 20
RANGES = (("plain", 0x0123456789abcdef, COUNT),
          ("carry32", (1 << 32) - (1 << 19), COUNT),
          ("wrap64-ragged", (1 << 64) - (1 << 19) - 3, COUNT + 5))
LADDERED = 3  # values of each range


def range_root(k):
    return sp.root_of(3000 + k)


def _top(root, start, count, n):
    """[(offset, value)] of the n highest values of the range, descending, by int comparison; hashlib confirms them."""
    vals = oracle.work_values_range(root, start, count).tolist()  # Python ints
    top = heapq.nlargest(n, range(count), key=vals.__getitem__)
    for off in top:
        assert oracle.work_value_hashlib(root, (start + off) & M64) == vals[off], "the oracle's two restatements differ"
    return [(off, vals[off]) for off in top]


@functools.lru_cache(maxsize=None)
def range_ladders():
    """The three ranges of the first root whose top three values all hold the conditions (each against the next lower
    value of its range) and show both states of bit 31."""
    for k in range(sp.MAX_SEEDS):
        root = range_root(k)
        out = []
        for name, start, count in RANGES:
            top = _top(root, start, count, LADDERED + 1)
            if any(conditions(top[i][1], top[i + 1][1]) for i in range(LADDERED)):
                break
            out.append(RangeLadder(name, root, start, count, tuple(top)))
        if len(out) == len(RANGES) and mixed([v for r in out for _, v in r.top[:LADDERED]]):
            return tuple(out)
    raise AssertionError(f"no root below seed {sp.MAX_SEEDS} holds the conditions on all three ranges")


def expected_hits(rl, T):
    """Every nonce of the range whose value is >= T (int comparison), ascending by nonce - start.  T lies above the
    range's fourth value (every rung of its top three does), so the top four decide."""
    assert T > rl.top[LADDERED][1]
    return [(rl.start + off) & M64 for off in sorted(off for off, v in rl.top if v >= T)]


def range_rungs(rl):
    """[(i, Rung)]: every rung of the range's i-th value, i = 0 (the maximum), 1, 2."""
    return [(i, r) for i in range(LADDERED) for r in rungs(rl.top[i][1])]


def best_of(rl, floor):
    """(nonce, value) of the range's strongest nonce if it reaches the floor, else None."""
    off, v = rl.top[0]
    return ((rl.start + off) & M64, v) if v >= floor else None


# ---- the four wrong comparisons (what a mutated kernel would compute) ---------------------------------------------
def _signed(x):
    return x - (1 << 32) if x & 0x80000000 else x


def wrong_high_only(v, t):
    return (v >> 32) >= (t >> 32)


def wrong_signed_low(v, t):
    return (v >> 32) > (t >> 32) or ((v >> 32) == (t >> 32) and _signed(v & LO) >= _signed(t & LO))


def wrong_both_words(v, t):
    return (v >> 32) >= (t >> 32) and (v & LO) >= (t & LO)


def wrong_strict(v, t):
    return v > t


WRONG = {"high-only": wrong_high_only, "signed-low": wrong_signed_low, "both-words": wrong_both_words,
         "strict": wrong_strict}


def disagreements(wrong, v):
    """The rungs of v on which the wrong comparison differs from the right one."""
    return [r.name for r in rungs(v) if wrong(v, r.T) != r.meets]
