"""The dense geometry of bounded pool entries (nano-dpow_amd/csrc/npow_dense.h) on the CPU.

A stand-alone C++ program with its own main includes the header the pool kernel and the host share, is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  It walks a bounded entry exactly as the kernel
does -- every own workgroup g (g % n == e), its 8 waves, iterations it < it_end, block it * K + 8 * rank + wave, nonce
base + 64 * block + lane, the lanes past the ragged end masked -- for every G in {64, 100, 128, 256, 1024, 1216},
every n in 1..64, every e < n, iters in {1, 2, 3} and ragged counts up to the entry's own share, and checks:

* the unmasked lanes cover [0, count) exactly once and no nonce outside it, from bases that cross 2^32 and 2^64;
* the workgroups' `done` sums to count;
* it_end <= iters for every workgroup whenever count <= own(e, n, iters), the host's bound;
* it_end is the same for all 8 waves of a workgroup (the loop ends in a workgroup barrier: a wave with one iteration
  fewer would hang the launch);
* the entries' own shares sum to the launch's full span;
* the header agrees, value for value, with a line-for-line transcription of pool_load_ls and of the kernel's lane
  mask as they stood before the header (the lane mask is still written out in the kernel: see
  test_header_is_host_and_device_and_shared);
* a job of several launches' worth, replayed over launches whose (n, e, iters) change at random, each taking
  min(remaining, own) from the front, has every nonce hashed exactly once.

No GPU here; the kernel itself is tests/test_gpu_crowded_tables.py.
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
#include "npow_dense.h"
using namespace npow;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
  fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
typedef unsigned long long ull;

// pool_load_ls's bounded branch and the hash loop's lane mask, transcribed line for line from npow_kernel.hip as they
// stood before npow_dense.h (kLsWaves = 8).
static const uint32_t kLsWaves = 8;
struct Cursor { uint32_t K, j, it_end, last_b, tail; };
static Cursor kernel_cursor(uint64_t count, uint32_t g, uint32_t wv, uint32_t G, uint32_t n, uint32_t e) {
  Cursor c;
  const uint32_t cnt = G / n + (e < G % n ? 1u : 0u);
  const uint32_t j0 = (g / n) * kLsWaves;
  c.K = kLsWaves * cnt;
  c.j = j0 + wv;
  const uint32_t blocks = (uint32_t)((count + 63) / 64);
  c.it_end = blocks > j0 ? (blocks - j0 + c.K - 1) / c.K : 0u;
  c.last_b = blocks - 1u;
  c.tail = (uint32_t)(count - (uint64_t)(blocks - 1u) * 64);
  return c;
}
static uint32_t kernel_in_lanes(uint32_t b, const Cursor& c) {
  const uint32_t in_lanes = b < c.last_b ? 64u : (b == c.last_b ? c.tail : 0u);
  return in_lanes;
}
// The same cursor from the header.
static Cursor header_cursor(uint64_t count, uint32_t g, uint32_t wv, uint32_t G, uint32_t n, uint32_t e) {
  Cursor c;
  const uint32_t j0 = dense_first_slot(g, n);
  c.K = dense_stride(G, n, e);
  c.j = j0 + wv;
  const uint32_t blocks = dense_blocks(count);
  c.it_end = dense_it_end(blocks, j0, c.K);
  c.last_b = dense_last_b(blocks);
  c.tail = dense_tail(count, c.last_b);
  return c;
}

static uint64_t g_walks, g_blocks, g_lanes;

// The kernel's walk of entry e of n in a launch of G workgroups: the entry's span is (base, count), `origin` the nonce
// of cover[0].  Every lane it does not mask adds one to cover[nonce - origin] (lanes = true), or every block adds its
// lanes in range to blk[b] and one to seen[b] (lanes = false: the lanes of a block are 0 .. in_lanes - 1, so a block
// seen once with the right number of lanes is its nonces once each; its first and last nonce are still range-checked).
// Returns the sum of the waves' `done`; *it_max the largest it_end of a workgroup.
static uint64_t walk_entry(uint64_t base, uint64_t count, uint32_t G, uint32_t n, uint32_t e, uint64_t origin,
                           uint64_t span, bool lanes, std::vector<uint8_t>& cover, std::vector<uint8_t>& seen,
                           std::vector<uint8_t>& blk, uint32_t* it_max) {
  uint64_t done = 0;
  uint32_t groups = 0;
  *it_max = 0;
  for (uint32_t g = 0; g < G; ++g) {
    if (dense_entry(g, n) != e) continue;  // own workgroups only
    CHECK(dense_rank(g, n) == groups, "rank of workgroup %u", g);
    ++groups;
    const Cursor c0 = header_cursor(count, g, 0, G, n, e);
    if (c0.it_end > *it_max) *it_max = c0.it_end;
    for (uint32_t wv = 0; wv < kDenseWaves; ++wv) {
      const Cursor c = header_cursor(count, g, wv, G, n, e), k = kernel_cursor(count, g, wv, G, n, e);
      CHECK(c.K == k.K && c.j == k.j && c.it_end == k.it_end && c.last_b == k.last_b && c.tail == k.tail,
            "header and kernel differ: G %u n %u e %u g %u wave %u count %llu", G, n, e, g, wv, (ull)count);
      // every wave of a workgroup runs the same number of iterations (each ends in a workgroup barrier)
      CHECK(c.it_end == c0.it_end, "G %u n %u e %u g %u: wave %u runs %u iterations, wave 0 %u", G, n, e, g, wv,
            c.it_end, c0.it_end);
      CHECK(c.tail >= 1 && c.tail <= 64, "tail %u", c.tail);
      CHECK((uint64_t)c.it_end * c.K + c.j < (1ull << 32), "block index overflows");
      for (uint32_t it = 0; it < c.it_end; ++it) {
        const uint32_t b = it * c.K + c.j;
        const uint32_t in_lanes = dense_block_lanes(b, c.last_b, c.tail);
        CHECK(in_lanes == kernel_in_lanes(b, k), "lane mask of block %u", b);
        done += in_lanes;
        ++g_blocks;
        if (!in_lanes) continue;
        const uint64_t first = base + ((uint64_t)b << 6);  // wraps mod 2^64
        CHECK(first - origin < span && first + (in_lanes - 1) - origin < span, "nonce %llx outside the range", (ull)first);
        if (lanes) {
          for (uint32_t lane = 0; lane < in_lanes; ++lane) {
            const uint64_t off = first + lane - origin;
            CHECK(cover[off] < 255, "overflow");
            cover[off]++;
          }
          g_lanes += in_lanes;
        } else {
          CHECK(seen[b] < 255, "overflow");
          seen[b]++;
          blk[b] = (uint8_t)in_lanes;
        }
      }
    }
  }
  CHECK(groups == dense_groups(G, n, e), "G %u n %u e %u: %u own workgroups, dense_groups %u", G, n, e, groups,
        dense_groups(G, n, e));
  ++g_walks;
  return done;
}

static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// One entry, one count: the walk covers [0, count) exactly once.
static void cover_once(uint32_t G, uint32_t n, uint32_t e, uint32_t iters, uint64_t count, uint64_t base, bool lanes) {
  static std::vector<uint8_t> cover, seen, blk;
  const uint32_t blocks = dense_blocks(count);
  if (lanes) cover.assign(count, 0); else { seen.assign(blocks, 0); blk.assign(blocks, 0); }
  uint32_t it_max;
  const uint64_t done = walk_entry(base, count, G, n, e, base, count, lanes, cover, seen, blk, &it_max);
  CHECK(done == count, "G %u n %u e %u count %llu: done %llu", G, n, e, (ull)count, (ull)done);
  CHECK(it_max <= iters, "G %u n %u e %u iters %u count %llu: a workgroup runs %u iterations", G, n, e, iters,
        (ull)count, it_max);
  if (lanes) {
    for (uint64_t i = 0; i < count; ++i)
      CHECK(cover[i] == 1, "G %u n %u e %u count %llu: offset %llu covered %u times", G, n, e, (ull)count, (ull)i, cover[i]);
  } else {
    for (uint32_t b = 0; b < blocks; ++b)
      CHECK(seen[b] == 1 && blk[b] == (b + 1 < blocks ? 64u : count - 64ull * (blocks - 1)),
            "G %u n %u e %u count %llu: block %u seen %u times with %u lanes", G, n, e, (ull)count, b, seen[b], blk[b]);
  }
}

// A job of `total` nonces from `start` over launches whose table changes every time.
static void stitch(uint32_t G, uint64_t start, uint64_t total, uint32_t seed) {
  std::vector<uint8_t> cover(total, 0), none;
  g_rng = seed;
  uint64_t at = 0, launches = 0;
  while (at < total) {
    const uint32_t n = 1 + rnd() % 64, e = rnd() % n, iters = 1 + rnd() % 3;
    const uint64_t own = dense_own(G, n, e, iters);
    if (own == 0) continue;  // (G < n: the entry has no workgroup in this launch; the host gives it none)
    const uint64_t take = total - at < own ? total - at : own;
    uint32_t it_max;
    const uint64_t done = walk_entry(start + at, take, G, n, e, start, total, true, cover, none, none, &it_max);
    CHECK(done == take && it_max <= iters, "stitch G %u n %u e %u: done %llu of %llu, %u iterations of %u", G, n, e,
          (ull)done, (ull)take, it_max, iters);
    at += take;
    ++launches;
  }
  for (uint64_t i = 0; i < total; ++i)
    CHECK(cover[i] == 1, "stitch G %u seed %u: offset %llu hashed %u times", G, seed, (ull)i, cover[i]);
  CHECK(launches >= 3, "stitch G %u: %llu launches", G, (ull)launches);
}

int main() {
  const uint32_t Gs[] = {64, 100, 128, 256, 1024, 1216};
  const uint64_t fixed[] = {1, 63, 64, 65, 511, 512, 513};
  unsigned long long cases = 0;
  for (uint32_t G : Gs) {
    const uint64_t walks0 = g_walks;
    uint64_t count_max = 0;
    for (uint32_t n = 1; n <= 64; ++n) {
      for (uint32_t iters = 1; iters <= 3; ++iters) {
        uint64_t sum = 0;
        for (uint32_t e = 0; e < n; ++e) sum += dense_own(G, n, e, iters);
        CHECK(sum == dense_full(G, iters), "G %u n %u iters %u: the own shares sum to %llu of %llu", G, n, iters,
              (ull)sum, (ull)dense_full(G, iters));
      }
      for (uint32_t e = 0; e < n; ++e) {
        CHECK(dense_groups(G, n, e) >= 1, "an entry without a workgroup");
        for (uint32_t iters = 1; iters <= 3; ++iters) {
          const uint64_t own = dense_own(G, n, e, iters);
          CHECK(own == (uint64_t)dense_stride(G, n, e) * iters * 64, "own and K");
          uint64_t counts[16];
          unsigned nc = 0;
          for (uint64_t c : fixed) if (c <= own) counts[nc++] = c;
          counts[nc++] = own - 1;
          counts[nc++] = own;
          for (int r = 0; r < 3; ++r) counts[nc++] = 1 + (((uint64_t)rnd() << 16) ^ rnd()) % own;
          for (unsigned i = 0; i < nc; ++i) {
            const uint64_t count = counts[i];
            // bases that make the span cross 2^32 and 2^64 (odd, so no block is aligned), and one far from both
            const uint64_t half = count / 2;
            const uint64_t bases[3] = {(1ull << 32) - half - (half & 1 ? 0 : 1), 0ull - half - (half & 1 ? 0 : 1),
                                       0x0123456789abcdefull};
            const uint64_t base = bases[(cases + i) % 3];
            // lane by lane on the small grids and for every small count; block by block beyond
            cover_once(G, n, e, iters, count, base, G <= 128 || count <= 4096);
            if (count > count_max) count_max = count;
            ++cases;
          }
        }
      }
    }
    printf("G %u n 1..64 entries %u iters 1..3 walks %llu largest count %llu\n", G, 64 * 65 / 2,
           (ull)(g_walks - walks0), (ull)count_max);
  }
  // stitching: (n, e, iters) change from launch to launch
  unsigned stitched = 0;
  for (uint32_t seed = 1; seed <= 4; ++seed) {
    stitch(64, 0ull - 54321, 4 * dense_own(64, 1, 0, 3) + 4097, seed);
    stitch(100, (1ull << 32) - 99999, 3 * dense_own(100, 1, 0, 3) + 65, seed + 10);
    stitch(128, 0x0123456789abcdefull, 3 * dense_own(128, 1, 0, 3) + 513, seed + 20);
    stitch(1024, 0ull - 1, 2 * dense_own(1024, 1, 0, 3) + 63, seed + 30);
    stitched += 4;
  }
  printf("stitched %u jobs\n", stitched);
  printf("ok cases %llu walks %llu blocks %llu lanes %llu\n", cases, (ull)g_walks, (ull)g_blocks, (ull)g_lanes);
  return 0;
}
"""


@pytest.fixture(scope="module")
def dense_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    src, exe = d / "dense.cpp", d / "dense"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True, capture_output=True, text=True, timeout=300)
    return str(exe)


def test_dense_walks_and_stitching_under_the_sanitizers(dense_program):
    p = subprocess.run([dense_program], capture_output=True, text=True, timeout=600)
    print(p.stdout)  # the coverage table: G, n and the counts walked
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    table = [re.fullmatch(r"G (\d+) n 1\.\.64 entries 2080 iters 1\.\.3 walks (\d+) largest count (\d+)", ln)
             for ln in lines[:6]]
    assert all(table), p.stdout
    assert [int(m.group(1)) for m in table] == [64, 100, 128, 256, 1024, 1216]
    for m in table:  # every (n, e, iters) with at least own - 1, own and three random counts; the largest is own at n = 1
        assert int(m.group(2)) >= 2080 * 3 * 5 and int(m.group(3)) == int(m.group(1)) * 8 * 3 * 64
    assert lines[6] == "stitched 16 jobs"
    m = re.fullmatch(r"ok cases (\d+) walks (\d+) blocks (\d+) lanes (\d+)", lines[7])
    assert m and int(m.group(1)) >= 6 * 2080 * 3 * 5 and int(m.group(2)) > int(m.group(1)), p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_header_is_host_and_device_and_shared():
    """One header for both sides: pool_load_ls and PoolShape call it, and the G / n + (e < G % n) rule stands nowhere
    else.  The hash loop's lane mask is the one expression still written out in the kernel (through the inline
    function the compiler swaps the operands of one s_and_b64, and the kernels' text is kept): its text is pinned
    here, and the program above checks dense_block_lanes against its transcription."""
    txt = open(os.path.join(CSRC, "npow_dense.h")).read()
    assert "__host__ __device__" in txt and "hip_runtime" not in txt
    internal = open(os.path.join(CSRC, "npow_internal.h")).read()
    kernel = open(os.path.join(CSRC, "npow_kernel.hip")).read()
    assert '#include "npow_dense.h"' in internal
    assert "kDenseWaves == (uint32_t)kLsWaves" in internal
    assert "return dense_own(units(), n, e, iters);" in internal and "dense_full(units(), iters)" in internal
    load = kernel[kernel.index("void pool_load_ls("):kernel.index("void lds_drain()")]
    for call in ("dense_groups(G, n, e)", "dense_first_slot(g, n)", "dense_blocks(pe->count)", "dense_it_end(blocks, j0, c.K)",
                 "dense_last_b(blocks)", "dense_tail(pe->count, c.last_b)"):
        assert call in load, call
    for name in ("npow_internal.h", "npow_kernel.hip", "npow_pool.cpp", "npow_pool_jobs.cpp", "npow_host.h"):
        src = open(os.path.join(CSRC, name)).read()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert not re.search(r"<\s*\w+\s*%\s*n\b", code), f"{name}: a second copy of the e < G % n rule"
    assert "const uint32_t in_lanes = b < c.last_b ? 64u : (b == c.last_b ? c.tail : 0u);" in kernel
    assert "return b < last_b ? 64u : (b == last_b ? tail : 0u);" in txt
