// npow_best.h -- the fold of a best job's records (npow_submit_best: the strongest nonce of a range), host side only
// and free of HIP types, so it compiles and is checked on its own (tests/test_best_cpu.py).
//
// A best job's entries (PoolEntry::bounded kEntryBest) append to the launch's hit records every nonce whose wave
// found it at or above the best value the launch had seen (npow_kernel.hip, ls2_best): a handful per launch, among
// them the launch's true maximum.  The host recomputes each record's value on the CPU and folds it into the job's
// best with the rule below, over launches and devices alike: the higher value wins, and among equal values the
// nonce nearest the start of the job's range (nonce - start, mod 2^64).  The rule is a total order on (value,
// offset), so the result does not depend on the order the records come in.
#pragma once
#include <stdint.h>

namespace npow {

struct BestFold {
  uint64_t nonce = 0, value = 0;
  bool found = false;  // a record at or above the floor has been folded in
};

// Is (value, nonce) better than what b holds, for a range starting at `start`?
inline bool best_beats(const BestFold& b, uint64_t start, uint64_t nonce, uint64_t value) {
  if (!b.found) return true;
  if (value != b.value) return value > b.value;
  return nonce - start < b.nonce - start;
}

// Fold one validated record; one below the job's floor is no candidate.  Returns whether it became the best.
inline bool best_fold(BestFold& b, uint64_t start, uint64_t floor, uint64_t nonce, uint64_t value) {
  if (value < floor || !best_beats(b, start, nonce, value)) return false;
  b.nonce = nonce;
  b.value = value;
  b.found = true;
  return true;
}

// The watch the job's next entry carries (PoolEntry::threshold): its best value so far, or the floor before any.
// Ties enter the kernel's branch (value >= watch), so a nonce equal to the best but nearer the start is still seen.
inline uint64_t best_watch(const BestFold& b, uint64_t floor) { return b.found && b.value > floor ? b.value : floor; }

}  // namespace npow
