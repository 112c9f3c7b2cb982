"""What a cut launch of a background best job is credited with, and what its records fold to, on the CPU.

A stand-alone C++ program with its own main includes the crediting step both collectors call
(nano-dpow_amd/csrc/npow_credit.h) with npow_claims.h and npow_best.h, is built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly.  For spans of 1, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193 and
3 * 8192 + 65 nonces and every claim count from 0 to chunks + 3 it replays a job through launches cut at that count:
a launch hashes the first `claims` chunks of its span as the kernel walks them, each chunk's records are the running
maxima of its nonces' synthetic values from the entry's watch on (best_watch of what the host has folded), the host
folds the chunks' records out of order, credits through credit_launch and issues the remainder again.  Checked:

* every nonce is hashed -- and credited -- exactly once, and the queue of ranges stays in range order with two
  launches in flight;
* the fold is the brute-force argmax, first occurrence (smallest nonce - start), also with equal maxima planted in
  different chunks, from bases that wrap at 2^64, and under a floor nothing reaches.

No GPU here; the kernel itself is tests/test_gpu_best_background.py.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nano-dpow_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>
#include "npow_best.h"
#include "npow_claims.h"
#include "npow_credit.h"
using namespace npow;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
  fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
typedef unsigned long long ull;

struct Job {
  uint64_t start, total, floor;
  std::vector<uint64_t> value;  // by offset
  std::vector<uint8_t> cover;
  uint64_t v(uint64_t nonce) const { return value[nonce - start]; }
};

static uint64_t mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}

// One launch of the span s with `claims` on its counter: the kernel's walk of the first min(claims, chunks) chunks,
// each chunk's records the running maxima (>=) of its nonces from `watch` on.  Returns the nonces walked.
static uint64_t launch(Job& j, const Range& s, uint64_t claims, uint64_t watch,
                       std::vector<std::vector<uint64_t>>& records) {
  const uint32_t chunks = claim_chunks(s.count), rows = claim_rows(s.count);
  const uint32_t k = claims < chunks ? (uint32_t)claims : chunks;
  uint64_t done = 0;
  for (uint32_t c = 0; c < k; ++c) {
    std::vector<uint64_t> rec;
    uint64_t w = watch;  // a workgroup that comes to the chunk knowing nothing but the entry's threshold
    for (uint32_t row = claim_row_first(c); row < claim_row_end(rows, c); ++row)
      for (uint32_t wave = 0; wave < kClaimRowBlocks; ++wave) {
        const uint64_t b = (uint64_t)row * kClaimRowBlocks + wave;
        const uint32_t lanes = claim_block_lanes(s.count, b);
        for (uint32_t lane = 0; lane < lanes; ++lane) {
          const uint64_t nonce = s.base + 64 * b + lane;  // wraps mod 2^64
          CHECK(nonce - j.start < j.total, "nonce %llx outside the job", (ull)nonce);
          CHECK(j.cover[nonce - j.start] < 255, "overflow");
          j.cover[nonce - j.start]++;
          if (j.v(nonce) >= w) {
            w = j.v(nonce);
            rec.push_back(nonce);
          }
        }
        done += lanes;
      }
    records.push_back(rec);
  }
  return done;
}

static bool in_order(const std::deque<Range>& todo, uint64_t start) {
  for (size_t i = 1; i < todo.size(); ++i)
    if (!(todo[i - 1].base - start < todo[i].base - start)) return false;
  return true;
}

// The job through launches of up to `span` nonces, each cut at `claims` (a launch that could cover nothing runs one
// chunk instead, so the job ends); two: a second launch is in flight while the first retires.
static void replay(Job& j, uint64_t span, uint64_t claims, bool two, unsigned* launches_cut) {
  std::fill(j.cover.begin(), j.cover.end(), 0);
  std::deque<Range> todo{{j.start, j.total}};
  BestFold best;
  uint64_t credited = 0;
  auto take = [&](Range& out) {
    if (todo.empty()) return false;
    Range& r = todo.front();
    out = {r.base, r.count < span ? r.count : span};
    r.base += out.count;
    r.count -= out.count;
    if (r.count == 0) todo.pop_front();
    return true;
  };
  bool first = true;
  auto retire = [&](const Range& s, uint64_t watch) {
    const uint64_t k = first || claims ? claims : 1;
    first = false;
    std::vector<std::vector<uint64_t>> records;
    const uint64_t done = launch(j, s, k, watch, records);
    // the fold, the chunks' records delivered out of order (last chunk first, each chunk's own reversed): each value
    // recomputed, a nonce outside the span never accepted
    for (size_t c = records.size(); c-- > 0;)
      for (size_t i = records[c].size(); i-- > 0;) {
        CHECK(records[c][i] - s.base < s.count, "a record outside its launch's span");
        best_fold(best, j.start, j.floor, records[c][i], j.v(records[c][i]));
      }
    const LaunchCredit cr = credit_launch(todo, j.start, s.base, s.count, true, k);
    CHECK(cr.covered == done, "launch of %llu cut at %llu: hashed %llu, credited %llu", (ull)s.count, (ull)k, (ull)done,
          (ull)cr.covered);
    CHECK(cr.cut == (cr.covered < s.count), "cut flag");
    CHECK(in_order(todo, j.start), "the queue of ranges left range order");
    if (cr.cut) {
      ++*launches_cut;
      CHECK(todo.front().base == s.base + cr.covered || two, "the remainder is not at the front");
    }
    credited += cr.covered;
  };
  unsigned guard = 0;
  while (!todo.empty()) {
    Range a, b;
    take(a);
    const uint64_t watch = best_watch(best, j.floor);  // both tables are built before either launch retires
    const bool second = two && take(b);
    retire(a, watch);
    if (second) retire(b, watch);
    CHECK(++guard < 100000, "no progress");
  }
  CHECK(credited == j.total, "credited %llu of %llu", (ull)credited, (ull)j.total);
  for (uint64_t i = 0; i < j.total; ++i)
    CHECK(j.cover[i] == 1, "offset %llu hashed %u times (total %llu, span %llu, claims %llu)", (ull)i, j.cover[i],
          (ull)j.total, (ull)span, (ull)claims);
  // brute force: argmax, first occurrence, at or above the floor
  bool found = false;
  uint64_t bo = 0;
  for (uint64_t i = 0; i < j.total; ++i)
    if (j.value[i] >= j.floor && (!found || j.value[i] > j.value[bo])) {
      found = true;
      bo = i;
    }
  CHECK(best.found == found, "found %d, brute force %d", (int)best.found, (int)found);
  if (found)
    CHECK(best.nonce == j.start + bo && best.value == j.value[bo],
          "fold (%llx, %llu), brute force (%llx, %llu): total %llu span %llu claims %llu", (ull)best.nonce,
          (ull)best.value, (ull)(j.start + bo), (ull)j.value[bo], (ull)j.total, (ull)span, (ull)claims);
}

// a plain entry is credited whole and leaves the queue alone
static void plain() {
  std::deque<Range> todo{{100, 5}};
  const LaunchCredit cr = credit_launch(todo, 0, 10, 3 * kClaimChunkNonces, false, 1);
  CHECK(cr.covered == 3 * kClaimChunkNonces && !cr.cut && todo.size() == 1 && todo[0].base == 100, "plain entry");
}

int main() {
  const uint64_t C = kClaimChunkNonces;
  static_assert(kClaimChunkNonces == 8192, "a chunk is 8,192 nonces");
  const uint64_t counts[] = {1, 63, 64, 65, 511, 512, 513, C - 1, C, C + 1, 3 * C + 65};
  const uint64_t starts[] = {0x0123456789abcdefull, 0ull - 12345};
  unsigned cases = 0, cut = 0;
  plain();
  for (uint64_t start : starts)
    for (uint64_t count : counts) {
      const uint32_t chunks = claim_chunks(count);
      for (int plant = 0; plant < 3; ++plant) {
        Job j{start, count, 0, std::vector<uint64_t>(count), std::vector<uint8_t>(count)};
        // few distinct values: ties everywhere
        for (uint64_t i = 0; i < count; ++i) j.value[i] = 1 + mix(i * 2654435761ull + plant) % 997;
        if (plant == 1) {  // equal maxima in different chunks: the last lane of the span, the first lane of a chunk
          j.value[count - 1] = 5000;
          j.value[count > C ? C : 0] = 5000;
          if (count > 2 * C) j.value[2 * C - 1] = 5000;
        }
        if (plant == 2) j.floor = 998;  // nothing reaches it
        for (uint64_t claims = 0; claims <= (uint64_t)chunks + 3; ++claims) {
          replay(j, ~0ull, claims, false, &cut);  // the whole range as one launch's span
          ++cases;
        }
      }
    }
  // spans below the range, two launches in flight: the earlier one's remainder goes in front of the later one's
  for (uint64_t start : starts)
    for (uint64_t span : {C + 65, 2 * C, 2 * C + 513}) {
      const uint64_t count = 7 * C + 65;
      Job j{start, count, 0, std::vector<uint64_t>(count), std::vector<uint8_t>(count)};
      for (uint64_t i = 0; i < count; ++i) j.value[i] = 1 + mix(i + span) % 997;
      j.value[3 * C] = j.value[C - 1] = j.value[count - 1] = 4000;
      for (uint64_t claims = 0; claims <= 4; ++claims) {
        replay(j, span, claims, true, &cut);
        replay(j, span, claims, false, &cut);
        cases += 2;
      }
    }
  CHECK(cut > 0, "no launch was cut");
  printf("ok %u cut %u\n", cases, cut);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("best_background")
    src, exe = d / "credit.cpp", d / "credit"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True, capture_output=True, text=True, timeout=300)
    return str(exe)


def test_cut_launches_credit_every_nonce_once_and_fold_to_the_argmax(program):
    p = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.fullmatch(r"ok (\d+) cut (\d+)", p.stdout.strip())
    # 2 starts x 11 spans x 3 value sets x (chunks + 4) claim counts, and the two-in-flight replays
    assert m and int(m.group(1)) >= 2 * 3 * (10 * 5 + 8) + 2 * 3 * 5 * 2 and int(m.group(2)) > 0, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_both_collectors_credit_through_the_one_helper():
    """The crediting step is HIP-free and shared: no second copy in the pool to drift."""
    txt = open(os.path.join(CSRC, "npow_credit.h")).read()
    assert "hip" not in txt.replace("HIP types", "").lower() and '#include "npow_claims.h"' in txt
    pool = open(os.path.join(CSRC, "npow_pool.cpp")).read()
    assert pool.count(" credit_launch(") == 1  # Worker::credit_entry alone; the prefix itself is the header's
    assert "= claim_prefix(" not in pool and "claim_prefix(count, claims)" in txt
    for collector in ("collect_best", "collect_sweep"):
        body = pool[pool.index(f"void Worker::{collector}("):]
        body = body[:body.index("\n}\n")]
        assert "credit_entry(sl, c, f);" in body, collector
    assert "collects() && background" in open(os.path.join(CSRC, "npow_pool.h")).read()
