"""The start map of a table that holds shared range jobs (nano-dpow_amd/csrc/npow_weights.h
pool_table_weights_claimed) and the span its claimed entries take (npow_claims.h), on the CPU.

A stand-alone C++ program with its own main includes the two headers the pool kernel and the host share, is built
with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  For grids of 128, 512 and 1,024 workgroups and
tables of 2, 3, 17 and 64 entries with one or two claimed entries (weight 1, at the table's ends) beside searches whose
weights cycle through patterns over {1, 2, 4, 8}, it deals the grid as the bounded kernels do (pool_claimed_pos, with
pool_claimed_mult's multiplier, over the cumulative weights 8 >> wsh) and checks:

* a workgroup starts on every entry;
* each claimed entry's started share is within one workgroup of grid * weight / sum of weights, with the weights as
  halved as the rule reports (*down);
* the returned modulus is the sum of the weights the shifts stand for;
* all-equal weights return 0 (g % n) with the jobs' own shifts;
* a table that also holds a dense entry returns 0 with the jobs' own shifts, not halved, whatever else it holds;
* a full launch region as a claimed entry's span has a chunk for every workgroup of the grid, and workgroups taking
  chunks from one counter until it runs past the span cover it exactly (claim_prefix).

The one-workgroup bound is why such a table has a map of its own: the searches' spread map (pool_start_pos) is up to
two workgroups off per entry.  The multiplier's properties are checked too: prime to the grid, so the places are a
permutation, and near grid / golden ratio.

No GPU here; the kernel is tests/test_gpu_range_shared.py.
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
#include <vector>
#include "npow_weights.h"
#include "npow_claims.h"
using namespace npow;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL line %d: ", __LINE__); \
  fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static const uint32_t kPatterns[][4] = {{8, 8, 8, 8}, {8, 1, 8, 1}, {1, 2, 4, 8}, {2, 2, 2, 2}, {4, 8, 4, 8},
                                        {8, 4, 2, 1}, {2, 1, 1, 1}, {4, 4, 4, 4}};
static double g_worst = 0;
static uint32_t g_misses = 0;

// The bounded kernels' deal (ls2_claimed_start): the number of entries whose inclusive prefix sum of 8 >> wsh is <= the
// position.  Every place of the grid is taken once.
static void deal(const uint32_t* wsh, uint32_t n, uint32_t grid, uint32_t wsum, std::vector<uint32_t>& started) {
  started.assign(n, 0);
  const uint32_t mult = pool_claimed_mult(grid);
  std::vector<uint8_t> place(grid, 0);
  for (uint32_t g = 0; g < grid; ++g) {
    const uint32_t p = (uint32_t)(((uint64_t)g * mult) % grid);
    CHECK(!place[p], "grid %u: place %u taken twice (mult %u)", grid, p, mult);
    place[p] = 1;
    const uint32_t r = pool_claimed_pos(g, wsum, grid, mult);
    CHECK(pool_claimed_pad_sum(pool_claimed_pad(wsum, mult)) == wsum &&
          pool_claimed_pad_mult(pool_claimed_pad(wsum, mult)) == mult, "the table's pad word holds %u and %u", wsum, mult);
    uint32_t acc = 0, k = 0;
    for (uint32_t i = 0; i < n; ++i) {
      acc += 8u >> (wsh[i] & 3u);
      if (acc <= r) ++k;
    }
    CHECK(k < n, "position %u past the map of %u", r, wsum);
    started[k]++;
  }
}

static uint32_t one_table(uint32_t grid, uint32_t n, uint32_t nclaimed, const uint32_t* pat) {
  std::vector<uint32_t> w(n), wsh(n), started;
  std::vector<uint8_t> kind(n, kTableUnbounded);
  for (uint32_t i = 0; i < n; ++i) w[i] = pat[i % 4];
  kind[n - 1] = kTableClaimed;  // the shared job, weight 1
  w[n - 1] = 1;
  if (nclaimed == 2) {
    kind[0] = kTableClaimed;
    w[0] = 1;
  }
  bool equal = true;
  for (uint32_t i = 0; i < n; ++i) equal = equal && w[i] == w[0];
  uint32_t down = 99;
  const uint32_t wsum =
      pool_table_weights_claimed(w.data(), kind.data(), n, grid, pool_claimed_mult(grid), wsh.data(), &down);
  if (equal) {
    CHECK(wsum == 0 && down == 0, "equal weights: wsum %u down %u", wsum, down);
    for (uint32_t i = 0; i < n; ++i) CHECK(wsh[i] == pool_wsh(w[i]), "equal weights: shift of %u", i);
    return 0;
  }
  if (wsum == 0) {  // halved until equal: g % n, and every entry has a workgroup since n <= grid
    for (uint32_t i = 0; i < n; ++i) CHECK(wsh[i] == wsh[0], "g %% n with unequal shifts");
    CHECK(n <= grid && down > 0, "g %% n: n %u grid %u down %u", n, grid, down);
    return 0;
  }
  uint32_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t eff = (w[i] >> down) ? (w[i] >> down) : 1u;
    CHECK(wsh[i] == pool_wsh(eff), "entry %u: shift %u for weight %u halved %u times", i, wsh[i], w[i], down);
    sum += eff;
  }
  CHECK(sum == wsum, "wsum %u, weights sum to %u", wsum, sum);
  deal(wsh.data(), n, grid, wsum, started);
  for (uint32_t i = 0; i < n; ++i) CHECK(started[i] > 0, "grid %u n %u: no workgroup starts on entry %u", grid, n, i);
  for (uint32_t i = 0; i < n; ++i) {
    if (kind[i] != kTableClaimed) continue;
    const double share = (double)grid * 1.0 / wsum;  // a claimed entry weighs 1 at every halving
    const double off = started[i] > share ? started[i] - share : share - started[i];
    if (off > g_worst) g_worst = off;
    if (off > 1.0) {  // (every figure is printed; the Python side asserts that there is none)
      ++g_misses;
      printf("miss grid %u n %u claimed entry %u: %u workgroups start there, its share is %.3f (wsum %u, down %u)\n",
             grid, n, i, started[i], share, wsum, down);
    }
  }
  return 1;
}

static void dense_table(uint32_t grid, uint32_t n, const uint32_t* pat) {
  for (uint32_t at = 0; at < n; at += (n > 8 ? 7 : 1)) {
    std::vector<uint32_t> w(n), wsh(n, 77);
    std::vector<uint8_t> kind(n, kTableUnbounded);
    for (uint32_t i = 0; i < n; ++i) w[i] = pat[i % 4];
    kind[n - 1] = kTableClaimed;
    w[n - 1] = 1;
    kind[at] = kTableDense;
    w[at] = 1;
    uint32_t down = 99;
    CHECK(pool_table_weights_claimed(w.data(), kind.data(), n, grid, pool_claimed_mult(grid), wsh.data(), &down) == 0,
          "a dense entry: g %% n");
    CHECK(down == 0, "a dense entry: nothing halved");
    for (uint32_t i = 0; i < n; ++i) CHECK(wsh[i] == pool_wsh(w[i]), "a dense entry: own shift of %u", i);
  }
}

// A claimed entry's span of a full launch region (grid workgroups x 8 waves x iters x 64 nonces): a chunk for every
// workgroup, and a counter handed round until it runs past the span covers it exactly.
static void span(uint32_t grid, uint32_t iters, uint32_t started) {
  const uint64_t full = (uint64_t)grid * kClaimRowBlocks * iters * 64;
  const uint32_t chunks = claim_chunks(full);
  CHECK(chunks >= grid, "grid %u iters %u: %u chunks", grid, iters, chunks);
  uint64_t counter = 0, covered = 0;
  for (bool any = true; any;) {
    any = false;
    for (uint32_t wg = 0; wg < started; ++wg) {
      const uint64_t k = counter++;
      if (k >= chunks) continue;
      covered += claim_chunk_nonces(full, (uint32_t)k);
      any = true;
    }
  }
  CHECK(covered == full && claim_prefix(full, counter) == full, "grid %u: covered %llu of %llu", grid,
        (unsigned long long)covered, (unsigned long long)full);
  CHECK(claim_prefix(full, started) == (started < chunks ? started * kClaimChunkNonces : full), "a cut launch's prefix");
}

// Workgroups are dispatched in index order and the earliest on a CU run fastest, so each quarter of the grid must hold
// each entry's share too, and each XCD shard (g mod 8): within 2 workgroups (and 1/4) of the part's share, the
// tolerance tests/test_weights_cpu.py gives the searches' spread map for the same statement.
static void spread(uint32_t grid) {
  const std::vector<std::vector<uint32_t>> tables = {{8, 1}, {1, 4}, {1, 1, 1, 1, 1, 1, 1, 1, 8}, {2, 1}, {8, 8, 8, 1}};
  const uint32_t mult = pool_claimed_mult(grid);
  for (const auto& eff : tables) {
    uint32_t sum = 0;
    for (uint32_t e : eff) sum += e;
    for (uint32_t part = 0; part < 12; ++part) {  // four quarters, eight shards
      std::vector<uint32_t> got(eff.size(), 0);
      uint32_t members = 0;
      for (uint32_t g = 0; g < grid; ++g) {
        if (part < 4 ? g * 4 / grid != part : g % 8 != part - 4) continue;
        const uint32_t r = pool_claimed_pos(g, sum, grid, mult);
        uint32_t acc = 0, k = 0;
        for (uint32_t e : eff) {
          acc += e;
          if (acc <= r) ++k;
        }
        got[k]++;
        ++members;
      }
      for (size_t i = 0; i < eff.size(); ++i) {
        const double want = (double)members * eff[i] / sum, off = got[i] > want ? got[i] - want : want - got[i];
        CHECK(off <= (want / 4 > 2.0 ? want / 4 : 2.0), "grid %u part %u entry %zu: %u workgroups, share %.2f", grid,
              part, i, got[i], want);
      }
    }
  }
}

int main() {
  const uint32_t grids[] = {128, 512, 1024}, sizes[] = {2, 3, 17, 64};
  uint32_t tables = 0, mapped = 0;
  for (uint32_t grid : grids)
    for (uint32_t n : sizes)
      for (const auto& pat : kPatterns) {
        for (uint32_t nclaimed = 1; nclaimed <= 2; ++nclaimed) {
          mapped += one_table(grid, n, nclaimed, pat);
          ++tables;
        }
        dense_table(grid, n, pat);
      }
  for (uint32_t grid : {128u, 512u, 1024u, 1216u, 320u, 96u, 3u}) {  // (304- and 80-CU devices, odd ends)
    const uint32_t mult = pool_claimed_mult(grid);
    const double off = (double)mult / grid - 0.6180339887;
    CHECK(mult >= 1 && mult < grid && (off < 0 ? -off : off) <= 0.125 + 2.0 / grid, "grid %u: mult %u", grid, mult);
    if (grid >= 96) spread(grid);
    std::vector<uint32_t> wsh1 = {0, 3}, started;  // weights (8, 1): every place once (deal checks), shares to one
    deal(wsh1.data(), 2, grid, 9, started);
    const double share = grid / 9.0, d1 = started[1] > share ? started[1] - share : share - started[1];
    CHECK(d1 <= 1.0, "grid %u: %u workgroups where the share is %.3f", grid, started[1], share);
  }
  for (uint32_t grid : grids) {
    span(grid, 4096, grid / 9 + 1);
    span(grid, 16, grid);
  }
  printf("ok %u tables %u mapped %u misses worst %.3f\n", tables, mapped, g_misses, g_worst);
  return 0;
}
"""


@pytest.fixture(scope="module")
def shared_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("range_shared")
    src, exe = d / "range_shared.cpp", d / "range_shared"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True, capture_output=True, text=True, timeout=300)
    return str(exe)


def test_start_map_of_all_claimed_tables_under_the_sanitizers(shared_program):
    p = subprocess.run([shared_program], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    m = re.fullmatch(r"ok (\d+) tables (\d+) mapped (\d+) misses worst ([0-9.]+)", p.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) == 3 * 4 * 8 * 2 and int(m.group(2)) >= 100, p.stdout
    # every claimed entry's started share within one workgroup of grid * weight / sum of weights
    assert int(m.group(3)) == 0 and float(m.group(4)) <= 1.0, p.stdout


def test_the_host_builds_its_tables_through_the_rule():
    """One rule for the host and the stand-alone program: the table builder calls it, and the kernel's claim loop and
    the host's crediting share the chunk geometry."""
    weights = open(os.path.join(CSRC, "npow_weights.h")).read()
    assert "pool_table_weights_claimed" in weights and "hip_runtime" not in weights
    pool = open(os.path.join(CSRC, "npow_pool.cpp")).read()
    assert "pool_table_weights_claimed(" in pool
    kernel = open(os.path.join(CSRC, "npow_kernel.hip")).read()
    assert "ls2_move_claimed(" in kernel and "claim_chunks(" in kernel
