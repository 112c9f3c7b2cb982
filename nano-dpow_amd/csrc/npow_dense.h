// npow_dense.h -- the dense geometry of a bounded entry (bounded searches, sweep jobs, best jobs), shared by the pool
// kernel and the host (no HIP types, so it compiles and is checked on its own: tests/test_dense_cpu.py).
//
// A launch of G workgroups holds a table of n entries.  Bounded entry e is hashed by its own workgroups only: those
// with g % n == e, dense_groups(G, n, e) of them, workgroup g being the entry's rank g / n.  A workgroup has
// kDenseWaves waves, each of which hashes one 64-nonce block per iteration: wave `wave` of rank r hashes block
//   b = it * K + 8 r + wave,   K = 8 * dense_groups(G, n, e),   nonce = base + 64 b + lane (mod 2^64),
// for it = 0 .. it_end - 1, so one iteration of all the entry's workgroups covers K consecutive blocks and the
// iterations follow one another: dense over [0, count), every nonce once.  The lanes of the entry's last block past
// `count` are masked (dense_block_lanes), as is every lane of a block past the last.
//
// it_end is the iteration count of the workgroup's FIRST wave, taken by all eight: every iteration of the kernel's loop
// ends in a workgroup barrier, so the waves of a workgroup must run the same number of iterations (a wave whose own
// blocks run out one iteration sooner hashes a masked block instead).  The host gives a launch at most
// dense_own(G, n, e, iters) nonces of an entry, which keeps it_end <= iters.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPOW_DENSE_HD __host__ __device__
#else
#define NPOW_DENSE_HD
#endif

namespace npow {

constexpr uint32_t kDenseWaves = 8;  // waves per workgroup, one 64-nonce block each per iteration (kLsWaves)

// Workgroups of entry e in a table of n entries over G workgroups (g % n == e): the first G % n entries have one more.
NPOW_DENSE_HD inline uint32_t dense_groups(uint32_t G, uint32_t n, uint32_t e) {
  return G / n + (e < G % n ? 1u : 0u);
}
// Workgroup g: the entry it owns, its rank among that entry's workgroups, and its first wave's block in iteration 0.
NPOW_DENSE_HD inline uint32_t dense_entry(uint32_t g, uint32_t n) { return g % n; }
NPOW_DENSE_HD inline uint32_t dense_rank(uint32_t g, uint32_t n) { return g / n; }
NPOW_DENSE_HD inline uint32_t dense_first_slot(uint32_t g, uint32_t n) { return dense_rank(g, n) * kDenseWaves; }
// K: the blocks one iteration of the entry's workgroups covers.
NPOW_DENSE_HD inline uint32_t dense_stride(uint32_t G, uint32_t n, uint32_t e) {
  return kDenseWaves * dense_groups(G, n, e);
}
// 64-nonce blocks of a span (the last one may be ragged; count >= 1, below 2^38).
NPOW_DENSE_HD inline uint32_t dense_blocks(uint64_t count) { return (uint32_t)((count + 63) / 64); }
// Iterations of the workgroup whose first wave starts at block j0: the iterations `it` with it * K + j0 < blocks.
NPOW_DENSE_HD inline uint32_t dense_it_end(uint32_t blocks, uint32_t j0, uint32_t K) {
  return blocks > j0 ? (blocks - j0 + K - 1) / K : 0u;
}
// The entry's last block and the lanes of it that lie in the span (64 = full).
NPOW_DENSE_HD inline uint32_t dense_last_b(uint32_t blocks) { return blocks - 1u; }
NPOW_DENSE_HD inline uint32_t dense_tail(uint64_t count, uint32_t last_b) {
  return (uint32_t)(count - (uint64_t)last_b * 64);
}
// The lanes of block b in range (the kernel's lane mask, and what the wave adds to its count of nonces done).
NPOW_DENSE_HD inline uint32_t dense_block_lanes(uint32_t b, uint32_t last_b, uint32_t tail) {
  return b < last_b ? 64u : (b == last_b ? tail : 0u);
}
// Nonces entry e of n can cover in one launch of `iters` wave iterations, and what a whole launch can.
NPOW_DENSE_HD inline uint64_t dense_own(uint32_t G, uint32_t n, uint32_t e, uint32_t iters) {
  return (uint64_t)dense_groups(G, n, e) * kDenseWaves * iters * 64;
}
NPOW_DENSE_HD inline uint64_t dense_full(uint32_t G, uint32_t iters) {
  return (uint64_t)G * kDenseWaves * iters * 64;
}

}  // namespace npow
