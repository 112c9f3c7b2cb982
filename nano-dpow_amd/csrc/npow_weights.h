// npow_weights.h -- job weights of the work pool as a launch's table carries them (host side; no HIP types, so
// the table builder's rule can be compiled and checked on its own: tests/test_weights_cpu.py).
#pragma once
#include <stdint.h>

namespace npow {

constexpr uint32_t kWshOne = 3;  // PoolEntry::wsh of weight 1
constexpr uint32_t kWshBg = 4;   // bit 2 of PoolEntry::wsh: the entry's background flag again (PoolEntry::bg), for
                                 // the kernel's pick, which loads this word anyway; every reader of the shift masks & 3
inline uint32_t pool_wsh(uint32_t weight) {  // weight in {1, 2, 4, 8} -> 3 - log2(weight)
  return weight >= 8 ? 0u : weight >= 4 ? 1u : weight >= 2 ? 2u : 3u;
}

// The start map: workgroup g of a launch whose table weights sum to wsum starts on the entry whose run of the
// cumulative weights holds pool_start_pos(g, wsum) in [0, wsum): the fractional part of g times the golden ratio,
// scaled.  Any stretch of consecutive workgroup indices is then spread almost evenly over [0, wsum), which matters
// twice: workgroups are dispatched in index order, four per CU, and a SIMD favours its oldest waves, so the first
// CUs-many indices hash several times as fast as the last (a map of contiguous runs, g % wsum, gave the first
// entries of a crowded table all the fast workgroups: measured 7 : 1 between equal jobs on a 32-CU partition); and
// workgroup counts are balanced per XCD shard (g mod 8), which a modulus sharing a factor with 8 aliases with.
#if defined(__HIPCC__)
#define NPOW_HD __host__ __device__
#else
#define NPOW_HD
#endif
NPOW_HD inline uint32_t pool_start_pos(uint32_t g, uint32_t wsum) {
  return (uint32_t)(((uint64_t)(uint32_t)(g * 0x9E3779B9u) * wsum) >> 32);
}

// Promotion (npow_promote): the host raises the weight of a job some running launch holds by writing the slot's
// pinned boost word, (gen << 2) | wsh of the job's raw new weight, and then bumping the promotion counter (the high
// half of PoolMailbox::kills).  One poller of each launch copies the words of its live entries into device memory
// (PoolDevState::boost) as (gen << 2) | level, level = 3 - wsh = log2(weight): generations and, within one, weights
// only grow, so the mirror is raised with an atomic max and two relays racing on one slot cannot leave the older
// word behind.  An entry's effective shift is the mirror's when its generation is the entry's own, on the launch's
// scale (its table's weights were halved `wdown` times, PoolTable::wdown: floor at weight 1 = shift 3, which is
// what pool_table_weights and Worker::dyn_add give a job of that weight); otherwise the entry's own wsh.
NPOW_HD inline uint64_t pool_boost_word(uint64_t gen, uint32_t wsh) { return (gen << 2) | (wsh & 3u); }
NPOW_HD inline uint64_t pool_boost_gen(uint64_t word) { return word >> 2; }
NPOW_HD inline uint32_t pool_boost_wsh(uint64_t word) { return (uint32_t)word & 3u; }
NPOW_HD inline uint64_t pool_boost_mirror(uint64_t word) { return (word & ~3ull) | (3u - ((uint32_t)word & 3u)); }
NPOW_HD inline uint32_t pool_promoted_wsh(uint32_t wsh, uint32_t wdown) {  // min(3, wsh + wdown)
  const uint32_t s = (wsh & 3u) + wdown;
  return s < 3u ? s : 3u;
}
NPOW_HD inline uint32_t pool_eff_wsh(uint64_t mirror, uint64_t gen, uint32_t own_wsh, uint32_t wdown) {
  return (mirror >> 2) == gen ? pool_promoted_wsh(3u - ((uint32_t)mirror & 3u), wdown) : (own_wsh & 3u);
}
// The balancing rule of ls2_poll: a workgroup of an entry with `mine` workgroups (shift sm) moves to one with `q`
// (shift sq) when, with it there, that entry still holds no more for its weight than this one without it.
NPOW_HD inline bool pool_should_move(unsigned long long q, uint32_t sq, unsigned long long mine, uint32_t sm) {
  return ((q + 1) << sq) + (1ull << sm) <= (mine << sm);
}

// The weights a launch of `grid` workgroups gives its n unbounded table entries, from the jobs' weights w[0..n)
// (each 1, 2, 4 or 8): wsh[i] = PoolEntry::wsh of entry i; *down = how many times every weight was halved (the
// launch's dynamic entries are halved alike, Worker::dyn_add); returns PoolTable::wsum, the start map's modulus,
// or 0 for the plain g % n start.
//  * Every weight equal (all 1, but also all 8): g % n deals equal shares exactly, so no map (0); the entries keep
//    their true wsh, against which a dynamic entry of another weight is compared.
//  * Otherwise the map above.  An entry on which no workgroup starts would -- the kernel balancing only toward
//    dynamic entries -- stay without one, launch after launch; with g % n and n <= 64 every entry has one.  So the
//    builder walks the grid through the map, and while some entry is left empty (a crowded table on a small grid:
//    a CU partition's is 128, and twenty jobs of weight 8 beside a light one sum to 161) it halves every weight,
//    floor 1, and tries again.  Halving flattens the ratios between the heaviest and the lightest jobs (8 : 1
//    becomes 4 : 1), only in tables that crowded.  If the halved weights are all equal, the table is dealt g % n (0).
inline uint32_t pool_table_weights(const uint32_t* w, uint32_t n, uint32_t grid, uint32_t* wsh, uint32_t* down) {
  *down = 0;
  for (uint32_t k = 0;; ++k) {
    uint32_t sum = 0, prefix[64];
    bool equal = true;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t eff = (w[i] >> k) ? (w[i] >> k) : 1u;
      wsh[i] = pool_wsh(eff);
      sum += eff;
      if (i < 64) prefix[i] = sum;
      equal = equal && wsh[i] == wsh[0];
    }
    *down = k;
    if (equal || n > 64) return 0;
    uint64_t started = 0;  // bit i: some workgroup starts on entry i
    for (uint32_t g = 0; g < grid; ++g) {
      const uint32_t r = pool_start_pos(g, sum);
      uint32_t e = 0;
      while (e + 1 < n && prefix[e] <= r) ++e;  // = the number of entries whose inclusive prefix sum is <= r
      started |= 1ull << e;
    }
    if (started == (n == 64 ? ~0ull : (1ull << n) - 1)) return sum;
  }
}

// Tables with bounded entries (shared range jobs, npow_submit_sweep_shared).  A dense bounded entry (a bounded search,
// a plain sweep or best job) is hashed by its own workgroups only, rank g / n of those with g % n == e (pool_load_ls),
// so a table that holds one is dealt g % n.  A claimed entry (kEntryClaim) takes its chunks from a counter and needs
// nothing of g % n: a table whose bounded entries are all claimed gets a start map over its jobs' weights by the rule
// above -- a workgroup starts on every entry, a crowded table is halved, equal weights give g % n.
//
// Its map is not pool_start_pos: that one's discrepancy is up to two workgroups per entry, which is nothing to a
// search's share and too much for a range job of weight 1 beside heavy searches on a small grid (13 workgroups of 128
// where its share is 14.2).  The claimed map is exact: workgroup g takes place p = g * mult mod grid, a permutation
// of the grid's places since mult is prime to grid, and stands at position p * csum / grid of [0, csum), so an entry
// whose run of the cumulative weights is [a, b) starts floor or ceil of grid * (b - a) / csum workgroups, give or take
// the one that straddles an end: within one workgroup of its share.  mult is an integer near grid / golden ratio
// that is prime to grid (pool_claimed_mult), so consecutive workgroups still spread over the whole map (dispatch
// order, pool_start_pos's reason), and since a prime to a grid of a multiple of 8 is odd, each XCD shard (g mod 8)
// takes every eighth place.
// Only the bounded kernels deal it (PoolTable::pad carries csum and mult, PoolTable::wsum stays 0: ls2_pick, which
// the unbounded kernels share, joins the entry it is given).
NPOW_HD inline uint32_t pool_claimed_pos(uint32_t g, uint32_t csum, uint32_t grid, uint32_t mult) {
  return (uint32_t)((uint64_t)(uint32_t)(((uint64_t)g * mult) % grid) * csum / grid);
}
// (Nearest alone is not enough: places g * mult mod grid spread evenly over every stretch of workgroups only if the
// continued fraction of mult / grid has small partial quotients -- 317 / 512 is within 0.001 of the golden ratio and
// left an entry of share 5 with 2 of a quarter's workgroups.  So of the multipliers prime to grid within grid / 8 of
// grid / golden ratio the one whose largest partial quotient is smallest, the nearest among equals.)
inline uint32_t pool_claimed_mult(uint32_t grid) {
  if (grid < 3) return 1;
  const uint32_t a = (uint32_t)((uint64_t)grid * 0x9E3779B9u >> 32);  // grid x 0.618...
  const uint32_t lo = a > grid / 8 + 1 ? a - grid / 8 : 1, hi = a + grid / 8 + 1 < grid ? a + grid / 8 + 1 : grid;
  uint32_t best = 1, best_q = ~0u, best_d = ~0u;
  for (uint32_t c = lo; c < hi; ++c) {
    uint32_t x = grid, y = c, q = 0;  // Euclid: the quotients are the continued fraction's, x ends as the gcd
    while (y) {
      if (x / y > q) q = x / y;
      const uint32_t t = x % y;
      x = y;
      y = t;
    }
    const uint32_t d = c > a ? c - a : a - c;
    if (x == 1 && (q < best_q || (q == best_q && d < best_d))) {
      best = c;
      best_q = q;
      best_d = d;
    }
  }
  return best;
}
// PoolTable::pad of such a table: bit 0 is kTabNoMoves (npow_internal.h), bits 1..10 csum (at most 64 entries of
// weight 8), bits 16..31 mult (grids below 2^16; a larger one is dealt g % n).
constexpr uint32_t kTabClaimedSumShift = 1, kTabClaimedSumMask = 0x3ffu, kTabClaimedMultShift = 16;
NPOW_HD inline uint32_t pool_claimed_pad(uint32_t csum, uint32_t mult) {
  return (csum << kTabClaimedSumShift) | (mult << kTabClaimedMultShift);
}
NPOW_HD inline uint32_t pool_claimed_pad_sum(uint32_t pad) { return (pad >> kTabClaimedSumShift) & kTabClaimedSumMask; }
NPOW_HD inline uint32_t pool_claimed_pad_mult(uint32_t pad) { return pad >> kTabClaimedMultShift; }

// kind[i]: what entry i is.  Returns csum, the claimed map's modulus, or 0 for g % n (a dense entry, equal weights,
// a grid of 2^16 workgroups or more); wsh[] and *down as pool_table_weights sets them -- the jobs' weights halved
// *down times, floor 1, until a workgroup starts on every entry -- and for a table with a dense entry the jobs' own
// shifts, not halved.  mult: pool_claimed_mult(grid).
enum : uint8_t { kTableUnbounded = 0, kTableDense = 1, kTableClaimed = 2 };
inline uint32_t pool_table_weights_claimed(const uint32_t* w, const uint8_t* kind, uint32_t n, uint32_t grid,
                                           uint32_t mult, uint32_t* wsh, uint32_t* down) {
  bool dense = false;
  for (uint32_t i = 0; i < n; ++i) dense = dense || kind[i] == kTableDense;
  *down = 0;
  if (dense || n > 64 || grid >= (1u << 16)) {
    for (uint32_t i = 0; i < n; ++i) wsh[i] = pool_wsh(w[i]);
    return 0;
  }
  for (uint32_t k = 0;; ++k) {
    uint32_t sum = 0, prefix[64];
    bool equal = true;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t eff = (w[i] >> k) ? (w[i] >> k) : 1u;
      wsh[i] = pool_wsh(eff);
      sum += eff;
      prefix[i] = sum;
      equal = equal && wsh[i] == wsh[0];
    }
    *down = k;
    if (equal) return 0;
    uint64_t started = 0;  // bit i: some workgroup starts on entry i
    for (uint32_t g = 0; g < grid; ++g) {
      const uint32_t r = pool_claimed_pos(g, sum, grid, mult);
      uint32_t e = 0;
      while (e + 1 < n && prefix[e] <= r) ++e;
      started |= 1ull << e;
    }
    if (started == (n == 64 ? ~0ull : (1ull << n) - 1)) return sum;
  }
}

// Background searches (npow_submit_background): an entry is foreground (every search above) or background
// (PoolEntry::bg).  A background entry is hashed only by workgroups no live foreground entry of its launch wants.
//  * Effective class: a background entry counts as foreground once its slot's boost mirror carries the entry's own
//    generation -- npow_promote lifts a background job through the same word and relay that raise a weight.  Classes
//    only ever change from background to foreground.
NPOW_HD inline bool pool_eff_background(uint32_t bg_flag, uint64_t mirror, uint64_t gen) {
  return bg_flag != 0 && (mirror >> 2) != gen;
}
//  * Pick order (ls2_choose takes the smallest key): every foreground entry sorts before any background one; within
//    a class the key is the workgroup count shifted by the entry's wsh, and background entries compare as weight 1
//    among themselves.  The high 32 bits of the pick key; counts are per XCD shard (< 2^27).
NPOW_HD inline uint32_t pool_pick_key(bool bg, unsigned long long wgs, uint32_t wsh) {
  return (bg ? 0x40000000u : 0u) | (uint32_t)(wgs << (bg ? kWshOne : (wsh & 3u)));
}
//  * Move rule (ls2_poll): a workgroup on a background entry moves to a live unbounded foreground entry whatever the
//    counts; one on a foreground entry never moves to a background entry; within a class pool_should_move decides.
//    Moves across classes go one way only and classes only rise, so no pair of entries admits a move in both
//    directions: across classes by construction, within one by pool_should_move's own argument.
NPOW_HD inline bool pool_should_move_class(bool q_bg, unsigned long long q, uint32_t sq, bool mine_bg,
                                           unsigned long long mine, uint32_t sm) {
  if (q_bg != mine_bg) return mine_bg;
  return mine_bg ? pool_should_move(q, kWshOne, mine, kWshOne) : pool_should_move(q, sq, mine, sm);
}
//  * Start map: pool_table_weights for a table of n <= 64 unbounded entries of which bg[i] != 0 are background.
//    No background entry: exactly pool_table_weights.  Only background entries: every wsh is kWshOne and the table is
//    dealt g % n (returns 0), as an equal-weight table.  Both classes: a background entry weighs 0 in the map (the
//    kernel gives its lane weight 0, ls2_pick), the returned wsum is the sum of the foreground weights -- non-zero
//    also when they are all equal, since g % n would start workgroups on the background entries -- and the halving rule
//    (a workgroup starts on every entry) applies to the foreground entries only: a background entry that starts
//    with none receives workgroups through ls2_choose once the foreground entries end.  Should the map leave a
//    foreground entry empty even with every weight at 1 (a grid far smaller than any device's), the flags are
//    cleared -- bg[] is in/out -- and the table runs as pool_table_weights deals it, its background jobs at weight 1.
inline uint32_t pool_table_weights_bg(const uint32_t* w, uint8_t* bg, uint32_t n, uint32_t grid, uint32_t* wsh,
                                      uint32_t* down) {
  uint32_t nbg = 0;
  for (uint32_t i = 0; i < n; ++i) nbg += bg[i] ? 1u : 0u;
  if (nbg == 0 || n > 64) {
    for (uint32_t i = 0; i < n; ++i) bg[i] = 0;
    return pool_table_weights(w, n, grid, wsh, down);
  }
  *down = 0;
  if (nbg == n) {
    for (uint32_t i = 0; i < n; ++i) wsh[i] = kWshOne;
    return 0;
  }
  for (uint32_t k = 0;; ++k) {
    uint32_t sum = 0, prefix[64];
    uint64_t want = 0;  // bit i: entry i is foreground
    bool ones = true;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t eff = bg[i] ? 0u : ((w[i] >> k) ? (w[i] >> k) : 1u);
      wsh[i] = bg[i] ? kWshOne : pool_wsh(eff);
      sum += eff;
      prefix[i] = sum;
      if (!bg[i]) want |= 1ull << i;
      ones = ones && eff <= 1u;
    }
    *down = k;
    uint64_t started = 0;
    for (uint32_t g = 0; g < grid; ++g) {
      const uint32_t r = pool_start_pos(g, sum);
      uint32_t e = 0;
      while (e + 1 < n && prefix[e] <= r) ++e;
      started |= 1ull << e;
    }
    if (started == want) return sum;
    if (ones) break;
  }
  uint32_t plain[64];
  for (uint32_t i = 0; i < n; ++i) {
    plain[i] = bg[i] ? 1u : w[i];
    bg[i] = 0;
  }
  return pool_table_weights(plain, n, grid, wsh, down);
}

}  // namespace npow
