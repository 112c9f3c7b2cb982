// npow_credit.h -- what a retired launch is credited with for one collecting entry (sweep jobs and best jobs, plain or
// background), host side only and free of HIP types, so it compiles and is checked on its own
// (tests/test_best_background_cpu.py).
//
// A plain collecting entry's launch hashed its whole span.  A claimed one (kEntryClaim, the background class:
// npow_submit_sweep_background, npow_submit_best_background) hashed the first `claims` chunks of it (npow_claims.h); a
// launch that a yield or its time budget cut short leaves a remainder, which goes back to the front of the device's
// queue of ranges.  The queue is kept in range order, by (base - start) mod 2^64: with two launches in flight the later
// one's span lies after this one's, and the remainder of the earlier one must be issued first again.
// Worker::collect_sweep and Worker::collect_best (npow_pool.cpp) both credit through credit_launch: what a launch
// covered does not depend on what its records mean.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <deque>

#include "npow_claims.h"

namespace npow {

// [base, base + count) mod 2^64: nonces of a job still to be handed to launches
struct Range {
  uint64_t base, count;
};

struct LaunchCredit {
  uint64_t covered;  // nonces of the span the launch hashed: a prefix of it
  bool cut;          // it left a remainder, now at its place in `todo`
};

// Entry [base, base + count) of a retired launch, of a job whose range starts at `start`.  claim: the entry was a
// claimed one, and the launch's claim counter of its slot reads `claims`.
inline LaunchCredit credit_launch(std::deque<Range>& todo, uint64_t start, uint64_t base, uint64_t count, bool claim,
                                  uint64_t claims) {
  LaunchCredit r{count, false};
  if (!claim) return r;
  r.covered = claim_prefix(count, claims);
  if (r.covered == count) return r;
  r.cut = true;
  todo.push_front({base + r.covered, count - r.covered});
  std::sort(todo.begin(), todo.end(),
            [start](const Range& x, const Range& y) { return x.base - start < y.base - start; });
  return r;
}

}  // namespace npow
