"""The sole-hit construction of tests/test_gpu_search_positions.py (pure Python and the oracle: no GPU here).

A one-entry launch of the unbounded first-win kernel (npow_kernel.hip pool_body_ls2<false>) covers the window
[base, base + F), F = grid * 8 * iters * 64 (npow_internal.h PoolShape::full; iters = PoolShape::launch_iters, half of
npow_set_tuning's iters_per_launch), unless it ends on its time budget.  Wave wv of workgroup g hashes, in its
iteration it, block b = it * K + g * 8 + wv with K = grid * 8, and its lane hashes nonce base + b * 64 + lane
(pool_load_ls, PoolCursor).  So a position of the window is (it, g, wv, lane), and

    pos = ((it * K + g * 8 + wv) * 64) + lane.

If exactly one nonce h of the window reaches the threshold, a search started at h - pos must return h, whatever pos is:
the hit then sits in the chosen iteration, workgroup, wave and lane.  sole_hit() finds such an h for an anchor A: the
unique maximum of the 3 F values from A on, taken only if it lies in the middle third -- then h is the only nonce at
or above T = value(h) in every window of length F that holds it.  Three anchors: a plain one, one whose windows cross
2^32 (a wave's `nonce += step` carries into the high word before it reaches h) and one whose windows wrap 2^64.
"""
import functools
import hashlib
import os
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import oracle  # noqa: E402  (the checker)

M64 = (1 << 64) - 1
WAVES = 8       # per workgroup (npow_internal.h kLsWaves)
LANES = 64
TUNING = 32     # npow_set_tuning's iters_per_launch in these tests ...
ITERS = 16      # ... that is 16 wave iterations per launch (PoolShape::launch_iters)
MAX_SEEDS = 32
ANCHORS = ("plain", "carry32", "wrap64")

SoleHit = namedtuple("SoleHit", "grid anchor seed root base h threshold full boundary second")


def full(grid, iters=ITERS):
    """Nonces of one launch's window (PoolShape::full)."""
    return grid * WAVES * iters * LANES


def step(grid):
    """A wave's `nonce += step` between two iterations: K * 64."""
    return grid * WAVES * LANES


def pos_of(it, g, wv, lane, grid):
    assert 0 <= g < grid and 0 <= wv < WAVES and 0 <= lane < LANES and it >= 0
    return ((it * grid * WAVES + g * WAVES + wv) * LANES) + lane


def coords_of(pos, grid):
    """The inverse of pos_of: (it, g, wv, lane)."""
    b, lane = divmod(pos, LANES)
    it, j = divmod(b, grid * WAVES)
    g, wv = divmod(j, WAVES)
    return it, g, wv, lane


def root_of(k):
    return hashlib.blake2b(b"nanopow-edge" + k.to_bytes(8, "little"), digest_size=32).digest()


def anchor_base(anchor, F):
    """The first nonce of the anchor's 3 F values, and the boundary its windows cross (None: the plain anchor)."""
    if anchor == "plain":
        return 0x0123456789abcdef, None
    if anchor == "carry32":
        return (1 << 32) - 3 * F // 2, 1 << 32
    if anchor == "wrap64":
        return ((1 << 64) - 3 * F // 2) & M64, 0
    raise ValueError(anchor)


@functools.lru_cache(maxsize=None)
def sole_hit(grid, anchor, iters=ITERS, first_seed=0):
    """The first seed k >= first_seed whose root has a unique maximum in the middle third of the 3 F values from the
    anchor on -- for the carry anchors in its second half, at or past the boundary.  A condition, not a measurement: at
    most MAX_SEEDS seeds.  `second` is the next lower of the 3 F values (tests/threshold_ladder.py: any threshold above
    it and up to value(h) keeps h the only hit)."""
    F = full(grid, iters)
    base, boundary = anchor_base(anchor, F)
    lo = F if boundary is None else 3 * F // 2
    for k in range(first_seed, MAX_SEEDS):
        root = root_of(k)
        v = oracle.work_values_range(root, base, 3 * F)
        off = int(v.argmax())
        t = int(v[off])
        if not lo <= off < 2 * F or int((v == v[off]).sum()) != 1:
            continue
        h = (base + off) & M64
        assert oracle.work_value_hashlib(root, h) == t, "the oracle's two restatements differ"
        v[off] = 0  # (the array is this call's own; values of one dtype compare exactly)
        return SoleHit(grid, anchor, k, root, base, h, t, F, boundary, int(v.max()))
    raise AssertionError(f"no seed from {first_seed} to {MAX_SEEDS - 1} has its unique maximum in the middle third "
                         f"(grid {grid}, {anchor})")


def carried(sh, pos):
    """A carry anchor's position at which the winning wave crosses the boundary in a `nonce += step`: its first nonce,
    h - it * step, lies before the boundary and h at or past it, so it >= 1."""
    if sh.boundary is None:
        return False
    it = coords_of(pos, sh.grid)[0]
    return it * step(sh.grid) > ((sh.h - sh.boundary) & M64)


def corners(grid, iters=ITERS):
    return [pos_of(it, g, wv, lane, grid) for it in (0, iters - 1) for g in (0, grid - 1) for wv in (0, WAVES - 1)
            for lane in (0, LANES - 1)]


def lane_positions(grid, iters=ITERS):
    """For L in 0..63: every lane, wave, iteration (iters <= 64) and XCD shard g % 8."""
    return [pos_of(L % iters, (L * grid // 64 + L) % grid, L % WAVES, L, grid) for L in range(64)]


def iteration_boundaries(grid, iters=ITERS):
    return [it * step(grid) - d for it in (1, iters // 2, iters - 1) for d in (1, 0)]


def first_carry(sh):
    """A carry anchor's earliest iteration whose wave has carried before it reaches h, at an inner wave and lane."""
    it = ((sh.h - sh.boundary) & M64) // step(sh.grid) + 1
    return pos_of(it, 1, 1, 1, sh.grid)


def positions(sh, iters=ITERS):
    ps = corners(sh.grid, iters) + lane_positions(sh.grid, iters) + iteration_boundaries(sh.grid, iters)
    if sh.boundary is not None:
        ps.append(first_carry(sh))
    assert all(0 <= p < sh.full for p in ps)
    return ps


def start_of(sh, pos):
    return (sh.h - pos) & M64
