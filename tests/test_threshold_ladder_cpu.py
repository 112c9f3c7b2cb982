"""tests/threshold_ladder.py without a GPU: the rung table is integer comparison, the constructions hold their
conditions under the oracle for the grids and ranges the GPU tests use, and each of the four wrong comparisons the
ladder is built against disagrees with it somewhere -- no rung is decoration."""
import pytest

import oracle
import search_positions as sp
import threshold_ladder as tl

HAND_MADE = [0xffffff52197d1aae, 0xfffffe65be70d25e, 0x000000017fffffff, 0x0000000180000000, 0xfffffffe7fffffff,
             0xfffffffe80000000, 0x8000000000000001, 0x7ffffffffffffffe, 0x00000001fffffffe, 0xfffffffe00000001]


@pytest.mark.parametrize("v", HAND_MADE, ids=[f"{v:016x}" for v in HAND_MADE])
def test_rung_table_is_integer_comparison(v):
    hi, lo = v >> 32, v & tl.LO
    rs = tl.rungs(v)
    assert [r.name for r in rs] == list(tl.NAMES)
    want = {"eq": (v, True), "below": (v - 1, True), "above": (v + 1, False),
            "flip31": (v ^ 0x80000000, tl.bit31(v)), "lo0": (hi << 32, True),
            "lomax": ((hi << 32) | tl.LO, lo == tl.LO), "hi-1": (((hi - 1) << 32) | tl.LO, True),
            "hi+1": ((hi + 1) << 32, False)}
    for r in rs:
        assert (r.T, r.meets) == want[r.name], r.name
        assert r.meets == (v >= r.T) and 0 <= r.T <= tl.M64
        assert r.meets == (v.to_bytes(8, "big") >= r.T.to_bytes(8, "big"))  # (a second statement of the order)
    assert tl.rung(v, "flip31") == rs[3]
    # every rung but hi-1 and hi+1 lies inside v's own high word
    assert all((r.T >> 32) == hi for r in rs[:6]) and rs[6].T >> 32 == hi - 1 and rs[7].T >> 32 == hi + 1


def test_conditions():
    assert tl.conditions(0xffffff5200000001, 0xffffff50ffffffff) is None
    assert "two high words" in tl.conditions(0xffffff5200000001, 0xffffff51ffffffff)
    assert "high word" in tl.conditions(0xffffffff00000001, 0xffffff0000000000)
    assert "low word" in tl.conditions(0xffffff5200000000, 0xffffff0000000000)
    assert "low word" in tl.conditions(0xffffff52ffffffff, 0xffffff0000000000)
    assert tl.mixed([0x80000000, 0x7fffffff]) and not tl.mixed([1, 2]) and not tl.mixed([0x80000000, 0xffffffff])


@pytest.mark.parametrize("grid", [1024, 512, 128])
def test_windows_hold_the_conditions(grid):
    """The whole MI355X (grid 1024), one of two CU partitions (512) and a 32-CU partition (128)."""
    ws = tl.window_ladders(grid)
    assert tuple(ws) == sp.ANCHORS
    for a, w in ws.items():
        sh = w.sh
        assert sh.seed < sp.MAX_SEEDS and sh.full == sp.full(grid)
        assert w.m1 == sh.threshold == oracle.work_value_hashlib(sh.root, sh.h) and w.m2 == sh.second < w.m1
        assert tl.conditions(w.m1, w.m2) is None and (w.m1 >> 32) - (w.m2 >> 32) >= 2
        assert [r.meets for r in w.rungs] == [True, True, False, tl.bit31(w.m1), True, False, True, False]
        # T in (m2, m1] for the rungs m1 meets, T above m1 for the others: h alone, or nothing, in every window with h
        assert all(w.m2 < r.T <= w.m1 if r.meets else r.T > w.m1 for r in w.rungs)
        print(f"grid {grid} {a}: seed {sh.seed}, m1 {w.m1:016x}, m2 {w.m2:016x}, m1.hi - m2.hi "
              f"{(w.m1 >> 32) - (w.m2 >> 32)}, bit 31 {'set' if tl.bit31(w.m1) else 'clear'}")
    assert tl.mixed([w.m1 for w in ws.values()])
    two = tl.two_anchors(grid)
    assert two[0].sh.anchor == "plain" and tl.mixed([w.m1 for w in two])


def test_window_second_value_under_the_oracle():
    """Grid 8 (F = 2^16): `second` is the highest value of the 3 F other than value(h), by int comparison, and a sweep
    at each rung returns h alone or nothing in the two extreme windows that hold h."""
    for a in sp.ANCHORS:
        sh = sp.sole_hit(8, a)
        vals = oracle.work_values_range(sh.root, sh.base, 3 * sh.full).tolist()
        off = (sh.h - sh.base) & sp.M64
        assert vals[off] == sh.threshold and max(vals[:off] + vals[off + 1:]) == sh.second < sh.threshold
        if tl.conditions(sh.threshold, sh.second):
            continue
        for r in tl.rungs(sh.threshold):
            for pos in (0, sh.full - 1):
                got = oracle.sweep(sh.root, r.T, sp.start_of(sh, pos), sh.full)
                assert got == ([sh.h] if r.meets else []), (a, r.name, pos)


def test_ranges_hold_the_conditions():
    rls = tl.range_ladders()
    assert [(r.name, r.start, r.count) for r in rls] == list(tl.RANGES) and len({r.root for r in rls}) == 1
    assert rls[1].start < 1 << 32 < rls[1].start + rls[1].count
    assert rls[2].start + rls[2].count > 1 << 64 and rls[2].count % 64 != 0
    laddered = []
    for rl in rls:
        vs = [v for _, v in rl.top]
        assert len(vs) == tl.LADDERED + 1 and vs == sorted(vs, reverse=True)
        for i in range(tl.LADDERED):
            assert tl.conditions(vs[i], vs[i + 1]) is None
        laddered += vs[:tl.LADDERED]
        rungs = tl.range_rungs(rl)
        assert len(rungs) == 8 * tl.LADDERED
        for i, r in rungs:
            want = tl.expected_hits(rl, r.T)
            # the oracle's own sweep (a C comparison of two uint64) and hashlib agree with the int comparison
            assert oracle.sweep(rl.root, r.T, rl.start, rl.count) == want, (rl.name, i, r.name)
            assert all(oracle.work_value_hashlib(rl.root, n) >= r.T for n in want)
            assert len(want) == i + (1 if r.meets else 0)
            assert ((rl.start + rl.top[i][0]) & tl.M64 in want) == r.meets
            assert want == sorted(want, key=lambda n: (n - rl.start) & tl.M64)
        assert tl.best_of(rl, vs[0]) == ((rl.start + rl.top[0][0]) & tl.M64, vs[0])
        assert tl.best_of(rl, vs[0] + 1) is None
    assert tl.mixed(laddered)


SET, CLEAR = 0xfffffe65be70d25e, 0xffffff52197d1aae  # bit 31 of the low word set, and clear


def test_each_wrong_comparison_fails_the_rungs_meant_for_it():
    """The table of the module's docstring, per wrong comparison and state of bit 31."""
    assert tl.bit31(SET) and not tl.bit31(CLEAR)
    assert tl.disagreements(tl.wrong_high_only, SET) == ["above", "lomax"]
    assert tl.disagreements(tl.wrong_high_only, CLEAR) == ["above", "flip31", "lomax"]
    assert tl.disagreements(tl.wrong_signed_low, SET) == ["flip31", "lo0"]
    assert tl.disagreements(tl.wrong_signed_low, CLEAR) == ["flip31", "lomax"]
    assert tl.disagreements(tl.wrong_both_words, SET) == ["hi-1"] == tl.disagreements(tl.wrong_both_words, CLEAR)
    assert tl.disagreements(tl.wrong_strict, SET) == ["eq"] == tl.disagreements(tl.wrong_strict, CLEAR)
    assert tl.disagreements(lambda v, t: v >= t, SET) == [] == tl.disagreements(lambda v, t: v >= t, CLEAR)


def test_no_rung_is_decoration():
    """Every rung but `below` (the control beside `eq`) is the only one, for some wrong comparison and bit 31, or one
    of the few, that catches it; and the laddered values of every construction catch all four."""
    caught = set()
    for wrong in tl.WRONG.values():
        for v in (SET, CLEAR):
            caught |= set(tl.disagreements(wrong, v))
    assert caught == set(tl.NAMES) - {"below", "hi+1"}
    # hi+1: a comparison of the low words alone (a 32-bit test on the wrong half) accepts it
    assert not tl.rung(CLEAR, "hi+1").meets and (CLEAR & tl.LO) >= (tl.rung(CLEAR, "hi+1").T & tl.LO)
    values = [w.m1 for w in tl.window_ladders(1024).values()]
    for rl in tl.range_ladders():
        values += [v for _, v in rl.top[:tl.LADDERED]]
    for name, wrong in tl.WRONG.items():
        assert any(tl.disagreements(wrong, v) for v in values), name
