"""tests/search_positions.py without a GPU: the position mapping is a bijection of a launch's window, the seed search
holds its condition under the oracle, and it reproduces the three results worked out for the whole MI355X (grid 1024,
F = 2^23)."""
import numpy as np
import pytest

import oracle
import search_positions as sp


@pytest.mark.parametrize("grid", [8, 12, 1024])
def test_mapping_is_a_bijection(grid):
    F = sp.full(grid)
    it, g, wv, lane = np.meshgrid(np.arange(sp.ITERS), np.arange(grid), np.arange(sp.WAVES), np.arange(sp.LANES),
                                  indexing="ij")
    pos = ((it * grid * sp.WAVES + g * sp.WAVES + wv) * sp.LANES + lane).ravel()
    assert pos.size == F and np.array_equal(np.sort(pos), np.arange(F))
    # the scalar functions are that mapping and its inverse (every position of the small grids, a stride of the large)
    for p in range(0, F, 1 if grid < 1024 else 4099):
        c = sp.coords_of(p, grid)
        assert sp.pos_of(*c, grid) == p
        assert c[0] < sp.ITERS and c[1] < grid and c[2] < sp.WAVES and c[3] < sp.LANES
    flat = pos.reshape(sp.ITERS, grid, sp.WAVES, sp.LANES)
    for c in [(0, 0, 0, 0), (sp.ITERS - 1, grid - 1, sp.WAVES - 1, sp.LANES - 1), (3, grid // 2, 5, 17)]:
        assert sp.pos_of(*c, grid) == flat[c]
    # a wave's consecutive iterations are one step apart
    assert sp.pos_of(1, 0, 0, 0, grid) - sp.pos_of(0, 0, 0, 0, grid) == sp.step(grid) == F // sp.ITERS


@pytest.mark.parametrize("grid", [8, 1024])
def test_position_lists(grid):
    F = sp.full(grid)
    cs = [sp.coords_of(p, grid) for p in sp.corners(grid)]
    assert len(set(cs)) == 16
    assert {c[0] for c in cs} == {0, 15} and {c[1] for c in cs} == {0, grid - 1}
    assert {c[2] for c in cs} == {0, 7} and {c[3] for c in cs} == {0, 63}
    ls = [sp.coords_of(p, grid) for p in sp.lane_positions(grid)]
    assert [c[3] for c in ls] == list(range(64))
    assert {c[0] for c in ls} == set(range(16)) and {c[2] for c in ls} == set(range(8))
    assert {c[1] % 8 for c in ls} == set(range(8))
    bs = sp.iteration_boundaries(grid)
    assert bs == [F // 16 - 1, F // 16, F // 2 - 1, F // 2, 15 * F // 16 - 1, 15 * F // 16]
    assert [sp.coords_of(p, grid) for p in bs[:2]] == [(0, grid - 1, 7, 63), (1, 0, 0, 0)]


@pytest.mark.parametrize("anchor", sp.ANCHORS)
def test_seed_search_holds_its_condition(anchor):
    """Grid 8 (F = 2^16): h is the only nonce at or above T in every window of length F that holds it -- checked on
    each of the anchor's positions and on the two extreme windows, against the oracle's sweep."""
    sh = sp.sole_hit(8, anchor)
    F = sh.full
    assert F == 1 << 16
    assert oracle.work_value_hashlib(sh.root, sh.h) == sh.threshold == oracle.work_value(sh.root, sh.h)
    assert F <= ((sh.h - sh.base) & sp.M64) < 2 * F
    for pos in sp.positions(sh) + [0, F - 1]:
        start = sp.start_of(sh, pos)
        assert oracle.sweep(sh.root, sh.threshold, start, F) == [sh.h], (anchor, pos)
    if sh.boundary is not None:
        assert ((sh.h - sh.boundary) & sp.M64) < F // 2
        ps = sp.positions(sh)
        crossing = [p for p in ps if sp.carried(sh, p)]
        # the corners of the last iteration cross the boundary, and so does the position added for it
        assert set(sp.corners(8)[8:]) <= set(crossing) and sp.first_carry(sh) in crossing
        for p in crossing:
            it = sp.coords_of(p, 8)[0]
            first = (sh.h - it * sp.step(8)) & sp.M64  # the winning wave's nonce in its iteration 0
            assert it >= 1 and ((first - sh.base) & sp.M64) < 3 * F // 2 <= ((sh.h - sh.base) & sp.M64)
    else:
        assert not any(sp.carried(sh, p) for p in sp.positions(sh))


@pytest.mark.parametrize("anchor,seed,h,t", [("plain", 1, 0x012345678a2e38d9, 0xffffff52197d1aae),
                                             ("carry32", 9, 0x00000001000a99a0, 0xfffffee734401d63),
                                             ("wrap64", 9, 0x000000000038b458, 0xfffffe65be70d25e)],
                         ids=sp.ANCHORS)
def test_whole_device_results(anchor, seed, h, t):
    sh = sp.sole_hit(1024, anchor)
    assert sh.full == 1 << 23
    assert (sh.seed, sh.h, sh.threshold) == (seed, h, t)
