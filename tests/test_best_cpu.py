"""The fold of a best job's records (nano-dpow_amd/csrc/npow_best.h) on the CPU.

A stand-alone C++ program with its own main includes the header the pool's host side folds with, is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly:

* equal values resolve to the smallest nonce - start, also for a range that runs across the wrap at 2^64;
* a record below the floor is ignored, one at the floor is a candidate (floor 0 included);
* the order the records come in is irrelevant: every permutation of a record set folds to the same best;
* the watch the next entry carries is the floor before any record and the best value after.

No GPU here; the kernel side is tests/test_gpu_best.py.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nano-dpow_amd", "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "npow_best.h"
using namespace npow;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
  fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Rec { uint64_t nonce, value; };

static BestFold fold(const std::vector<Rec>& r, uint64_t start, uint64_t floor) {
  BestFold b;
  for (const Rec& x : r) best_fold(b, start, floor, x.nonce, x.value);
  return b;
}

// The definition, by brute force: the highest value at or above the floor; among equals the smallest nonce - start.
static BestFold brute(const std::vector<Rec>& r, uint64_t start, uint64_t floor) {
  BestFold b;
  for (const Rec& x : r) {
    if (x.value < floor) continue;
    if (!b.found || x.value > b.value || (x.value == b.value && x.nonce - start < b.nonce - start)) {
      b.nonce = x.nonce;
      b.value = x.value;
      b.found = true;
    }
  }
  return b;
}

static unsigned permutations(std::vector<Rec> r, uint64_t start, uint64_t floor) {
  const BestFold want = brute(r, start, floor);
  std::vector<size_t> idx(r.size());
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
  unsigned n = 0;
  do {
    std::vector<Rec> p;
    for (size_t i : idx) p.push_back(r[i]);
    const BestFold got = fold(p, start, floor);
    CHECK(got.found == want.found, "found %d want %d", (int)got.found, (int)want.found);
    if (want.found)
      CHECK(got.nonce == want.nonce && got.value == want.value, "permutation %u: %llx/%llx want %llx/%llx", n,
            (unsigned long long)got.nonce, (unsigned long long)got.value, (unsigned long long)want.nonce,
            (unsigned long long)want.value);
    ++n;
  } while (std::next_permutation(idx.begin(), idx.end()));
  return n;
}

int main() {
  unsigned cases = 0;
  // equal values: the smallest offset from the start wins, whatever the order
  {
    const uint64_t start = 1000;
    BestFold b = fold({{1500, 77}, {1200, 77}, {1900, 77}}, start, 0);
    CHECK(b.found && b.nonce == 1200 && b.value == 77, "tie: %llu", (unsigned long long)b.nonce);
    b = fold({{1200, 77}, {1500, 77}}, start, 0);
    CHECK(b.nonce == 1200, "tie, first kept");
    ++cases;
  }
  // ... across the wrap: the range starts 16 below 2^64, so nonce 3 (offset 19) lies after nonce 2^64 - 5 (offset 11)
  {
    const uint64_t start = 0ull - 16;
    BestFold b = fold({{3, 900}, {0ull - 5, 900}}, start, 0);
    CHECK(b.nonce == 0ull - 5, "wrap tie: %llx", (unsigned long long)b.nonce);
    b = fold({{0ull - 5, 900}, {3, 900}, {0ull - 16, 900}}, start, 0);
    CHECK(b.nonce == 0ull - 16, "wrap tie at the start: %llx", (unsigned long long)b.nonce);
    b = fold({{0ull - 5, 900}, {3, 901}}, start, 0);
    CHECK(b.nonce == 3 && b.value == 901, "the higher value beats the nearer nonce");
    ++cases;
  }
  // the floor: below it no candidate, at it one; floor 0 takes value 0
  {
    BestFold b = fold({{5, 99}, {6, 50}}, 0, 100);
    CHECK(!b.found, "below the floor");
    CHECK(best_watch(b, 100) == 100, "watch before any record");
    b = fold({{5, 99}, {6, 100}, {7, 98}}, 0, 100);
    CHECK(b.found && b.nonce == 6 && b.value == 100, "at the floor");
    CHECK(best_watch(b, 100) == 100, "watch at the floor");
    b = fold({{9, 0}}, 0, 0);
    CHECK(b.found && b.nonce == 9 && b.value == 0, "floor 0 takes value 0");
    b = fold({{5, 99}, {6, 150}}, 0, 100);
    CHECK(best_watch(b, 100) == 150, "watch follows the best");
    CHECK(!best_fold(b, 0, 100, 7, 120) && b.nonce == 6, "a lesser record changes nothing");
    CHECK(best_fold(b, 0, 100, 2, 150) && b.nonce == 2, "an equal record nearer the start replaces");
    CHECK(!best_fold(b, 0, 100, 2, 150), "the same record again is no news");
    ++cases;
  }
  // order: every permutation of sets with ties, values below the floor, and nonces on both sides of the wrap
  unsigned perms = 0;
  {
    const std::vector<Rec> a = {{10, 5}, {11, 9}, {12, 9}, {13, 2}, {14, 9}, {15, 7}};
    perms += permutations(a, 0, 0);
    perms += permutations(a, 12, 0);   // nonce 12 now has offset 0, nonce 11 the largest
    perms += permutations(a, 0, 8);
    perms += permutations(a, 0, 10);   // nothing reaches the floor
    const std::vector<Rec> w = {{0ull - 3, 40}, {0ull - 1, 41}, {0, 41}, {2, 41}, {5, 40}, {0ull - 7, 3}};
    perms += permutations(w, 0ull - 8, 0);
    perms += permutations(w, 0ull - 8, 41);
    perms += permutations(w, 1, 0);    // the range starts after the wrap: nonce 2 is nearest
    cases += 7;
  }
  printf("ok %u perms %u\n", cases, perms);
  return 0;
}
"""


@pytest.fixture(scope="module")
def best_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("best")
    src, exe = d / "best.cpp", d / "best"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True, capture_output=True, text=True, timeout=300)
    return str(exe)


def test_fold_ties_floor_and_order_under_the_sanitizers(best_program):
    p = subprocess.run([best_program], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.fullmatch(r"ok (\d+) perms (\d+)", p.stdout.strip())
    assert m and int(m.group(1)) == 10 and int(m.group(2)) == 7 * 720, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_header_needs_no_hip_and_the_pool_folds_with_it():
    txt = open(os.path.join(CSRC, "npow_best.h")).read()
    assert "hip_runtime" not in txt and "__device__" not in txt
    pool = open(os.path.join(CSRC, "npow_pool.cpp")).read()
    assert '#include "npow_best.h"' in open(os.path.join(CSRC, "npow_pool.h")).read()
    assert "best_fold(" in pool and "best_watch(" in pool
