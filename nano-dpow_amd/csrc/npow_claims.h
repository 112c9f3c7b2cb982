// npow_claims.h -- the chunk geometry of a claimed collecting entry (background sweep jobs,
// npow_submit_sweep_background), shared by the pool kernel and the host (no HIP types, so it compiles and is checked on
// its own: tests/test_claims_cpu.py).
//
// A claimed entry's launch span is `count` nonces from `base` (mod 2^64), at most what a bounded entry takes (well
// below 2^41).  It is cut into rows of kClaimRowNonces nonces -- 8 consecutive 64-nonce blocks, one per wave of a
// workgroup, as npow_sweep_kernel_ls2's rows -- and into chunks of kClaimRows rows.  A workgroup takes the next chunk
// index from the launch's claim counter of the slot (PoolHits::claim) and hashes that chunk to its end; a launch that
// stops early (its time budget, a yield) has issued k < chunks claims, and what it covered is the contiguous prefix of
// those k chunks: the host credits claim_prefix(count, k) nonces and hands the rest back to the job.
//
// kClaimRows = 16: a workgroup iteration (one row) takes 8 waves x ~4,246 SIMD cycles, about 15 us at 2.3 GHz (an
// estimate from the cycles per hash, not a measurement), so a chunk is ~0.25 ms -- the time a running launch needs to
// end once a search wants the device -- against one atomic and two workgroup barriers (~1 us) per claim.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPOW_CLAIM_HD __host__ __device__
#else
#define NPOW_CLAIM_HD
#endif

namespace npow {

constexpr uint32_t kClaimRows = 16;                                     // R: rows per chunk
constexpr uint32_t kClaimRowBlocks = 8;                                 // 64-nonce blocks per row (kLsWaves)
constexpr uint64_t kClaimRowNonces = 64ull * kClaimRowBlocks;           // 512
constexpr uint64_t kClaimChunkNonces = kClaimRowNonces * kClaimRows;    // 8,192

// Rows of a span (the last one may be ragged), and its chunks (the last one may hold fewer rows).
NPOW_CLAIM_HD inline uint32_t claim_rows(uint64_t count) {
  return (uint32_t)((count + kClaimRowNonces - 1) / kClaimRowNonces);
}
NPOW_CLAIM_HD inline uint32_t claim_chunks(uint64_t count) {
  return (uint32_t)((count + kClaimChunkNonces - 1) / kClaimChunkNonces);
}
// Chunk c: its first nonce as an offset into the span, and how many nonces of the span it holds (0 past the end).
NPOW_CLAIM_HD inline uint64_t claim_chunk_first(uint32_t c) { return (uint64_t)c * kClaimChunkNonces; }
NPOW_CLAIM_HD inline uint64_t claim_chunk_nonces(uint64_t count, uint32_t c) {
  const uint64_t first = claim_chunk_first(c);
  if (first >= count) return 0;
  return count - first < kClaimChunkNonces ? count - first : kClaimChunkNonces;
}
// The rows [first, end) of chunk c within a span of `rows` rows.
NPOW_CLAIM_HD inline uint32_t claim_row_first(uint32_t c) { return c * kClaimRows; }
NPOW_CLAIM_HD inline uint32_t claim_row_end(uint32_t rows, uint32_t c) {
  const uint32_t first = claim_row_first(c);
  return rows - first < kClaimRows ? rows : first + kClaimRows;  // (c < chunks, so first < rows)
}
// The lanes of 64-nonce block b that lie in the span (the kernel's lane mask).
NPOW_CLAIM_HD inline uint32_t claim_block_lanes(uint64_t count, uint64_t b) {
  const uint64_t first = b * 64;
  if (first >= count) return 0;
  return count - first < 64 ? (uint32_t)(count - first) : 64u;
}
// The nonces covered by a launch whose counter reads `claims`: the first min(claims, chunks) chunks.  (The counter
// runs past `chunks` by one for every workgroup that found the span used up.)
NPOW_CLAIM_HD inline uint64_t claim_prefix(uint64_t count, uint64_t claims) {
  const uint64_t chunks = claim_chunks(count);
  if (claims >= chunks) return count;
  return claims * kClaimChunkNonces;
}

}  // namespace npow
