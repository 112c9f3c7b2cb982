// npow_reserve_key.h -- the key that orders a slot's reserve candidates (PoolDevState::reserve_best), shared by the
// pool kernel and the host (no HIP types, so it compiles and is checked on its own: tests/test_reserve_records_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPOW_RESERVE_KEY_HD __host__ __device__
#else
#define NPOW_RESERVE_KEY_HD
#endif

namespace npow {

// The key of a reserve candidate: the slot's generation above 24 bits of the value.  Reserve thresholds are at least
// NPOW_RESERVE_MIN (fffff00000000000), so a candidate's top 20 bits are ones and bits 43..20 order candidates to one
// part in 2^24 of that range; two that tie there are as good as each other.  Generations stay below 2^40 (one per
// adoption: centuries at any rate a GPU can be armed).
NPOW_RESERVE_KEY_HD inline unsigned long long pool_reserve_key(uint64_t gen, uint64_t value) {
  return (unsigned long long)((gen << 24) | ((value >> 20) & 0xffffffull));
}

}  // namespace npow
