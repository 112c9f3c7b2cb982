"""The record construction of tests/test_gpu_reserve_exact.py (pure Python and hashlib: no GPU here).

The root of tests/golden/sweep_2p36_hashlib.json has every nonce of [0, 2^36) with a work value at or above
OLD = fffffff800000000 pinned by hashlib: 126 hits.  For a reserve threshold R >= OLD every reserve candidate of a
search of that root inside the range is therefore known without hashing anything.

A fixture hit h is a *record* for a window length F (the nonces of one launch, tests/search_positions.py full()) and a
stretch Z if no fixture hit with a higher value lies in [h - F, h + Z] and h + Z <= 2^36.  A search started at
S = h - pos, pos < F, then covers h in its first launch at the chosen (iteration, workgroup, wave, lane), and for Z more
nonces

* nothing at or above v(h) + 1 exists, so a search at T = v(h) + 1 cannot be decided, and
* at T = 2^64 - 1 nothing can displace h in the reserve:

"poll Ticket.reserve() until it holds h" has one right outcome.  Lower hits of the window may be filed first where R
admits them (lower_in_window); with R = v(h) or v(h) - 1 h is the window's only candidate.

The key buckets: the kernel orders candidates by value >> 20 (npow_reserve_key.h pool_reserve_key).  The 126 values fall in
126 buckets, so no two tie there (tests/test_reserve_records_cpu.py).
"""
import functools
import hashlib
import json
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = (1 << 64) - 1
LO = 0xffffffff
OLD = 0xfffffff800000000
END = 1 << 36          # the fixture covers [0, END)
Z33, Z34 = 1 << 33, 1 << 34
SOLO_S, SOLO_N = 0x846e097c0, 1 << 34  # tests/test_gpu_reserve.py's solo launch: [S, S + 2^34)

Rung = namedtuple("Rung", "name T R candidate")


def value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


@functools.lru_cache(maxsize=None)
def fixture():
    """(root, {nonce: hashlib value}) of the 2^36 sweep fixture; every value recomputed here."""
    with open(os.path.join(HERE, "golden", "sweep_2p36_hashlib.json")) as f:
        g = json.load(f)
    root = bytes.fromhex(g["root"])
    assert int(g["threshold"], 16) == OLD and int(g["start"], 16) == 0 and g["count"] == END
    hits = {int(h, 16): value(root, int(h, 16)) for h in g["hits"]}
    assert len(hits) == 126 and all(v >= OLD for v in hits.values())
    return root, hits


def hits_in(lo, hi):
    """The fixture hits of [lo, hi), in nonce order."""
    assert 0 <= lo <= hi <= END, "outside the fixture's range: nothing is known there"
    return sorted(n for n in fixture()[1] if lo <= n < hi)


def records(F, Z):
    """The fixture hits h with no higher value in [h - F, h + Z], h - F >= 0 and h + Z <= 2^36, in nonce order."""
    hits = fixture()[1]
    out = []
    for h in sorted(hits):
        if h - F < 0 or h + Z > END:
            continue
        if all(hits[n] <= hits[h] for n in hits_in(h - F, min(h + Z + 1, END))):
            out.append(h)
    return out


def low_word_decides(v):
    """v's low word is neither 0 nor ffffffff: v - 1, v and v + 1 share v's high word, so a comparison of the high
    words alone cannot tell them apart."""
    return v & LO not in (0, LO)


def ladder(h):
    """The (T, R) rungs of a record h.  candidate: whether h is a reserve candidate under the rung, that is
    R <= v(h) < T -- worked out with Python's int comparison alone."""
    v = fixture()[1][h]
    assert OLD < v < M64 - 1
    out = []
    for tn, T in (("max", M64), ("v+1", v + 1)):
        for rn, R in (("v", v), ("v-1", v - 1), ("old", OLD)):
            out.append(Rung(f"T={tn},R={rn}", T, R, R <= v < T))
    out.append(Rung("T=max,R=v+1", M64, v + 1, v + 1 <= v < M64))
    assert [r.candidate for r in out] == [True] * 6 + [False] and all(OLD <= r.R <= r.T for r in out)
    return out


def lower_in_window(h, F):
    """The fixture hits below v(h) that share some window of length F with h: those of (h - F, h + F)."""
    hits = fixture()[1]
    return [n for n in hits_in(max(h - F + 1, 0), min(h + F, END)) if n != h and hits[n] < hits[h]]


def window_hits(S, F):
    """{nonce: value} of the fixture hits of the first launch's window [S, S + F)."""
    hits = fixture()[1]
    return {n: hits[n] for n in hits_in(S, S + F)}


def running_records(S, n):
    """The prefix maxima, in nonce order, of the fixture hits of [S, S + n): what a reserve at R = OLD could hold if
    the range were hashed in order.  One launch does not hash in order (its workgroups drift apart:
    tests/test_gpu_reserve_exact.py test_best_so_far_of_one_long_launch), so only the last of them, the range's
    maximum, is asserted on the GPU."""
    hits = fixture()[1]
    out, best = [], 0
    for x in hits_in(S, S + n):
        if hits[x] > best:
            best = hits[x]
            out.append(x)
    return out


def key_bucket(v):
    """The bucket of 2^20 values that v falls in; the key itself is checked where it is defined, by the compiled header
    (tests/test_reserve_records_cpu.py)."""
    return v >> 20
