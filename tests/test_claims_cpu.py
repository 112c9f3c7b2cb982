"""The chunk geometry of background sweep jobs (nano-dpow_amd/csrc/npow_claims.h) on the CPU.

A stand-alone C++ program with its own main includes the header the pool kernel and the host share, is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  It walks a claimed entry's span exactly as the
kernel does -- chunk c, rows [cR, (c+1)R), block row * 8 + wave, nonce base + 64 * block + lane, lanes past the ragged
end masked -- and checks against what the host credits:

* for every stop point k in 0..chunks, the union of the first k chunks' nonces is exactly the prefix
  claim_prefix(count, k), each nonce once, and prefix and remainder partition the span;
* a job replayed through launches that are cut at arbitrary points, the remainder going back to the front of its
  queue of ranges, has every nonce hashed exactly once.

No GPU here; the kernel itself is tests/test_gpu_sweep_background.py.
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
#include "npow_claims.h"
using namespace npow;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
  fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// The kernel's walk of chunk c of the span (base, count): every lane it does not mask adds one to cover[nonce - origin].
// Returns the lanes it counted (the workgroup's `done`).
static uint64_t walk_chunk(uint64_t base, uint64_t count, uint32_t c, uint64_t origin, std::vector<uint8_t>& cover) {
  const uint32_t rows = claim_rows(count);
  uint64_t done = 0;
  for (uint32_t row = claim_row_first(c); row < claim_row_end(rows, c); ++row)
    for (uint32_t wave = 0; wave < kClaimRowBlocks; ++wave) {
      const uint64_t b = (uint64_t)row * kClaimRowBlocks + wave;
      const uint32_t lanes = claim_block_lanes(count, b);
      for (uint32_t lane = 0; lane < lanes; ++lane) {
        const uint64_t nonce = base + 64 * b + lane;  // wraps mod 2^64
        const uint64_t off = nonce - origin;
        CHECK(off < cover.size(), "nonce %llx outside the range", (unsigned long long)nonce);
        CHECK(cover[off] < 255, "overflow");
        cover[off]++;
      }
      done += lanes;
    }
  return done;
}

static void prefixes(uint64_t base, uint64_t count) {
  const uint32_t chunks = claim_chunks(count);
  CHECK(chunks == (claim_rows(count) + kClaimRows - 1) / kClaimRows, "chunks of %llu", (unsigned long long)count);
  CHECK(claim_chunk_nonces(count, chunks) == 0, "a chunk past the end holds nonces");
  for (uint32_t k = 0; k <= chunks; ++k) {
    std::vector<uint8_t> cover(count, 0);
    uint64_t done = 0, by_size = 0;
    for (uint32_t c = 0; c < k; ++c) {
      const uint64_t d = walk_chunk(base, count, c, base, cover);
      CHECK(d == claim_chunk_nonces(count, c), "chunk %u of %llu: %llu lanes", c, (unsigned long long)count,
            (unsigned long long)d);
      CHECK(claim_chunk_first(c) == (uint64_t)c * kClaimChunkNonces, "first of chunk %u", c);
      done += d;
      by_size += claim_chunk_nonces(count, c);
    }
    const uint64_t prefix = claim_prefix(count, k);
    CHECK(prefix <= count && done == prefix && by_size == prefix, "count %llu k %u: prefix %llu, walked %llu",
          (unsigned long long)count, k, (unsigned long long)prefix, (unsigned long long)done);
    for (uint64_t i = 0; i < count; ++i)  // the prefix once, the remainder not at all: they partition the span
      CHECK(cover[i] == (i < prefix ? 1 : 0), "count %llu k %u: offset %llu covered %u times",
            (unsigned long long)count, k, (unsigned long long)i, cover[i]);
    CHECK((k == chunks) == (prefix == count), "count %llu k %u: full cover", (unsigned long long)count, k);
  }
  // the counter runs past the span's chunks, once per workgroup that found it used up
  CHECK(claim_prefix(count, (uint64_t)chunks + 1) == count && claim_prefix(count, (uint64_t)chunks + 1024) == count,
        "a counter past the chunks");
}

struct Range { uint64_t base, count; };

// The host's side of a job over (start, total): launches take up to `span` nonces from the front of the queue, the
// kernel covers the first k chunks (k from the generator: any stop point, the full span at times), the remainder goes
// back to the front.  A second launch in flight takes its span before the first one's remainder returns.
static void replay(uint64_t start, uint64_t total, uint64_t span, uint32_t seed) {
  std::vector<uint8_t> cover(total, 0);
  std::deque<Range> todo{{start, total}};
  uint64_t credited = 0, launches = 0, cut = 0;
  uint32_t x = seed;
  auto rnd = [&x] { x = x * 1664525u + 1013904223u; return x >> 8; };
  auto take = [&](Range& out) {
    if (todo.empty()) return false;
    Range& r = todo.front();
    out = {r.base, r.count < span ? r.count : span};
    r.base += out.count;
    r.count -= out.count;
    if (r.count == 0) todo.pop_front();
    return true;
  };
  auto retire = [&](const Range& s) {
    const uint32_t chunks = claim_chunks(s.count);
    const uint32_t mode = rnd() % 4;
    const uint64_t claims = mode == 0 ? chunks + rnd() % 64 : (mode == 1 ? 0 : rnd() % (chunks + 1));
    const uint32_t k = claims < chunks ? (uint32_t)claims : chunks;
    uint64_t done = 0;
    for (uint32_t c = 0; c < k; ++c) done += walk_chunk(s.base, s.count, c, start, cover);
    const uint64_t prefix = claim_prefix(s.count, claims);
    CHECK(done == prefix, "launch: hashed %llu, credited %llu", (unsigned long long)done, (unsigned long long)prefix);
    credited += prefix;
    ++launches;
    if (prefix < s.count) {
      ++cut;
      todo.push_front({s.base + prefix, s.count - prefix});
    }
  };
  uint32_t idle = 0;
  while (!todo.empty()) {
    Range a, b;
    take(a);
    const bool two = rnd() % 2 && take(b);  // two launches in flight
    const uint64_t before = credited;
    retire(a);
    if (two) retire(b);
    idle = credited == before ? idle + 1 : 0;
    CHECK(idle < 10000, "no progress");
  }
  CHECK(credited == total, "credited %llu of %llu", (unsigned long long)credited, (unsigned long long)total);
  for (uint64_t i = 0; i < total; ++i)
    CHECK(cover[i] == 1, "offset %llu hashed %u times (span %llu, seed %u)", (unsigned long long)i, cover[i],
          (unsigned long long)span, seed);
  CHECK(total <= span || launches > 1, "launches");
  (void)cut;
}

int main() {
  static_assert(kClaimRowNonces == 512 && kClaimChunkNonces == kClaimRows * 512, "rows of 8 blocks of 64");
  const uint64_t C = kClaimChunkNonces;
  const uint64_t counts[] = {1, 63, 64, 65, 511, 512, 513, C - 1, C, C + 1, 3 * C + 65};
  const uint64_t bases[] = {0, 0x0123456789abcdefull};
  unsigned cases = 0;
  for (uint64_t base : bases)
    for (uint64_t count : counts) {
      prefixes(base, count);
      ++cases;
    }
  // spans that end at, and run across, the wrap-around at 2^64, from odd bases
  prefixes(0ull - (3 * C + 65), 3 * C + 65);
  prefixes(0ull - 12345, 3 * C + 65);
  prefixes(0ull - 1, C + 1);
  cases += 3;
  // whole jobs through cut launches: spans of one chunk and less, several chunks, ragged ones
  const uint64_t spans[] = {1, 64, 513, C - 1, C, 2 * C + 65, 7 * C};
  for (uint64_t span : spans)
    for (uint32_t seed = 1; seed <= 6; ++seed) {
      replay(0x0123456789abcdefull, span < 64 ? 700 : 9 * C + 4097, span, seed);
      replay(0ull - 12345, 5 * C + 65, span < 64 ? 4096 : span, seed + 100);
      cases += 2;
    }
  printf("ok %u R %u\n", cases, kClaimRows);
  return 0;
}
"""


@pytest.fixture(scope="module")
def claims_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims")
    src, exe = d / "claims.cpp", d / "claims"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True, capture_output=True, text=True, timeout=300)
    return str(exe)


def test_prefixes_and_replays_under_the_sanitizers(claims_program):
    p = subprocess.run([claims_program], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.fullmatch(r"ok (\d+) R (\d+)", p.stdout.strip())
    assert m and int(m.group(1)) >= 25 + 2 * 7 * 6, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_header_is_host_and_device_and_shared():
    """One header for both sides: the kernel and the host include the same geometry (no second copy to drift)."""
    txt = open(os.path.join(CSRC, "npow_claims.h")).read()
    assert "__host__ __device__" in txt and "hip_runtime" not in txt
    assert '#include "npow_claims.h"' in open(os.path.join(CSRC, "npow_internal.h")).read()
    kernel = open(os.path.join(CSRC, "npow_kernel.hip")).read()
    pool = open(os.path.join(CSRC, "npow_pool.cpp")).read()
    assert "claim_chunks(" in kernel and "claim_row_end(" in kernel
    assert "claim_prefix(" in pool
    m = re.search(r"constexpr uint32_t kClaimRows = (\d+);", txt)
    assert m and int(m.group(1)) == 16
