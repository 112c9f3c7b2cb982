"""tests/reserve_records.py without a GPU: the conditions the tests of tests/test_gpu_reserve_exact.py lean on hold for
the fixture and for the grids they run on, and the key that orders a slot's reserve candidates
(nano-dpow_amd/csrc/npow_reserve_key.h pool_reserve_key) orders them as their values do.

The key is checked where it is defined: a stand-alone C++ program with its own main includes the header the pool
kernel and the host share, is built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly, with the
fixture's 126 values as its arguments.  Nothing of the key is restated in Python.
"""
import os
import subprocess

import pytest

import reserve_records as rr
import search_positions as sp
from conftest import ROOT

CSRC = os.path.join(ROOT, "nano-dpow_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
GRIDS = [1024, 512, 128]  # the whole MI355X, one of two CU partitions, a 32-CU partition


def test_the_fixture_facts_the_gpu_tests_quote():
    root, hits = rr.fixture()
    F = sp.full(1024)
    assert F == 1 << 23
    r33, r34 = rr.records(F, rr.Z33), rr.records(F, rr.Z34)
    assert [f"{h:x}" for h in r33] == ["152692f99", "3a307f8fb", "6de52ed29", "760a48842", "8302498d0", "a927c68ff",
                                       "b356c0992"]
    assert [f"{h:x}" for h in r34] == ["6de52ed29", "a927c68ff"]
    assert sum(1 for h in r33 if hits[h] >> 32 == rr.LO) == 6
    run = rr.running_records(rr.SOLO_S, rr.SOLO_N)
    assert len(rr.hits_in(rr.SOLO_S, rr.SOLO_S + rr.SOLO_N)) == 26 and len(run) == 7
    assert run[0] == 0x8d93d76ac and run[-1] == 0xa927c68ff and hits[run[-1]] == 0xffffffffee3ad8ec
    assert [hits[n] for n in run] == sorted(hits[n] for n in run)
    # the closest pair of hits is 2^21.98 nonces apart: no wave ever holds two candidates of this fixture
    s = sorted(hits)
    assert min(b - a for a, b in zip(s, s[1:])) == 4136019 > 64


@pytest.mark.parametrize("grid", GRIDS)
def test_records_hold_the_conditions(grid):
    root, hits = rr.fixture()
    F = sp.full(grid)
    recs = rr.records(F, rr.Z33)
    assert len(recs) >= 3
    assert any(rr.low_word_decides(hits[h]) for h in recs)
    assert set(rr.records(F, rr.Z34)) <= set(recs)
    for h in recs:
        v = hits[h]
        assert v == rr.value(root, h)
        # the definition, by int comparison over the whole fixture
        assert all(x <= v for n, x in hits.items() if h - F <= n <= h + rr.Z33) and h - F >= 0 and h + rr.Z33 <= rr.END
        # every position of the grid keeps [S, S + Z) inside the fixture's range, and h the best of the first window
        sh = sp.SoleHit(grid, "fixture", None, root, None, h, v, F, None, None)
        ps = sp.positions(sh)
        assert len(ps) == 86
        for pos in ps:
            S = sp.start_of(sh, pos)
            assert 0 <= S <= h < S + F and S + rr.Z33 <= rr.END
            w = rr.window_hits(S, F)
            assert w[h] == v == max(w.values())
        rungs = rr.ladder(h)
        assert len(rungs) == 7 and [r.candidate for r in rungs] == [True] * 6 + [False]
        assert {(r.T, r.R) for r in rungs} == {(T, R) for T in (rr.M64, v + 1) for R in (v, v - 1, rr.OLD)} | \
            {(rr.M64, v + 1)}
        # (no record of this fixture shares a window with a lower hit: the R = OLD rungs still allow for one)
        print(f"grid {grid}: record {h:x} value {v:016x}, lower hits within F: "
              f"{[f'{n:x}' for n in rr.lower_in_window(h, F)]}")


def test_the_key_buckets_are_distinct():
    _, hits = rr.fixture()
    assert len({rr.key_bucket(v) for v in hits.values()}) == 126


def test_running_records_are_prefix_maxima():
    _, hits = rr.fixture()
    S, n = rr.SOLO_S, rr.SOLO_N
    run = rr.running_records(S, n)
    window = rr.hits_in(S, S + n)
    assert run == [x for i, x in enumerate(window) if all(hits[y] < hits[x] for y in window[:i])]
    assert rr.running_records(0, rr.END)[-1] == max(hits, key=hits.get)


PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include "nanopow.h"
#include "npow_reserve_key.h"
using namespace npow;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
  fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
typedef unsigned long long ull;

int main(int argc, char** argv) {
  const uint64_t kMin = NPOW_RESERVE_MIN, kMax = ~0ull;
  const uint64_t gens[] = {0, 1, 2, 12345, (1ull << 32) - 1, 1ull << 32, (1ull << 40) - 2};
  // monotone in the value at bucket granularity: one key per 2^20 values, each bucket one above the last, over the
  // whole of [NPOW_RESERVE_MIN, 2^64)
  ull buckets = 0;
  for (uint64_t g : {gens[0], gens[3], gens[6]}) {
    uint64_t lo = kMin;
    ull prev = 0;
    buckets = 0;
    for (;;) {
      const uint64_t hi = lo | 0xfffffull;
      const ull k = pool_reserve_key(g, lo);
      CHECK(k == pool_reserve_key(g, hi) && k == pool_reserve_key(g, lo + (hi - lo) / 3), "bucket of %llx", (ull)lo);
      CHECK(buckets == 0 || k == prev + 1, "key of %llx is %llx after %llx", (ull)lo, k, prev);
      prev = k;
      ++buckets;
      if (hi == kMax) break;
      lo = hi + 1;
    }
    CHECK(buckets == 1ull << 24, "%llu buckets", buckets);
  }
  printf("buckets %llu\n", buckets);
  // a higher generation beats any value, and a key never leaves 64 bits
  for (uint64_t g : gens) {
    CHECK(pool_reserve_key(g + 1, kMin) > pool_reserve_key(g, kMax), "generation %llu", (ull)g);
    CHECK(pool_reserve_key(g, kMax) >> 24 == g && pool_reserve_key(g, kMin) >> 24 == g, "generation %llu", (ull)g);
  }
  printf("generations %zu\n", sizeof(gens) / sizeof(gens[0]));
  // the fixture's values order by key as by value
  std::vector<uint64_t> v;
  for (int i = 1; i < argc; ++i) v.push_back(strtoull(argv[i], nullptr, 16));
  for (uint64_t x : v) CHECK(x >= kMin, "%llx is below NPOW_RESERVE_MIN", (ull)x);
  std::vector<uint64_t> by_value(v), by_key(v);
  std::sort(by_value.begin(), by_value.end());
  std::stable_sort(by_key.begin(), by_key.end(),
                   [](uint64_t a, uint64_t b) { return pool_reserve_key(7, a) < pool_reserve_key(7, b); });
  CHECK(by_value == by_key, "the orders differ");
  for (size_t i = 1; i < by_value.size(); ++i)
    CHECK(pool_reserve_key(7, by_value[i - 1]) < pool_reserve_key(7, by_value[i]), "a tie at %llx", (ull)by_value[i]);
  printf("values %zu\nok\n", v.size());
  return 0;
}
"""


@pytest.fixture(scope="module")
def key_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("reserve_key")
    src, exe = d / "reserve_key.cpp", d / "reserve_key"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-I", INCLUDE, "-o", str(exe), str(src)], check=True, capture_output=True, text=True,
                   timeout=300)
    return str(exe)


def test_reserve_key_under_the_sanitizers(key_program):
    _, hits = rr.fixture()
    p = subprocess.run([key_program] + [f"{v:016x}" for v in hits.values()], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.split() == ["buckets", str(1 << 24), "generations", "7", "values", "126", "ok"], p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_the_key_has_one_definition():
    """One header for both sides, as npow_dense.h: npow_internal.h includes it, the kernel and the host call it, and
    the rule stands nowhere else."""
    txt = open(os.path.join(CSRC, "npow_reserve_key.h")).read()
    assert "__host__ __device__" in txt and "hip_runtime" not in txt
    assert '#include "npow_reserve_key.h"' in open(os.path.join(CSRC, "npow_internal.h")).read()
    assert "pool_reserve_key(gen, rv)" in open(os.path.join(CSRC, "npow_kernel.hip")).read()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip", ".cpp")) and name != "npow_reserve_key.h":
            assert "inline unsigned long long pool_reserve_key" not in open(os.path.join(CSRC, name)).read(), name
