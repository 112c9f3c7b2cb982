"""Promotion (npow_promote) on the CPU side: the declaration and the export, the stats field, and the helpers of
nano-dpow_amd/csrc/npow_weights.h that the host and the kernel share -- the pinned boost word, its device-memory
mirror, the effective shift of an entry and the balancing rule with a promoted side.  No GPU here; the shares are
measured in tests/test_gpu_promote.py."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")
CSRC = os.path.join(ROOT, "nano-dpow_amd", "csrc")


def test_header_declares_npow_promote_within_abi_7():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+npow_promote\s*\(([^)]*)\)", txt)
    assert m, "include/nanopow.h does not declare npow_promote"
    assert [a.strip() for a in m.group(1).split(",")] == ["uint64_t ticket", "uint32_t weight"]
    assert re.search(r"#define NPOW_ABI_VERSION (\d+)", txt).group(1) == "7"
    assert _lib.NPOW_ABI_VERSION == 7
    # the revision comment names the addition
    rev = raw[raw.index("ABI revision"):raw.index("#define NPOW_ABI_VERSION")]
    assert "npow_promote" in rev and "promotions" in rev


def test_library_exports_npow_promote():
    lib = _lib.load()
    assert hasattr(lib, "npow_promote")
    assert "npow_promote" in _lib.EXPORTED_SYMBOLS
    assert lib.npow_abi_version() == 7
    assert callable(getattr(_lib.Ticket, "promote", None))


def test_device_stats_has_promotions_last():
    names = [f[0] for f in _lib.DeviceStats._fields_]
    assert names[-1] == "promotions" and names[-2] == "stale_gpu_delay_us"
    assert _lib.DeviceStats.promotions.size == 8
    assert _lib.DeviceStats.promotions.offset == ctypes.sizeof(_lib.DeviceStats) - 8


def test_promote_before_init_is_an_error_with_a_message():
    """In a process of its own: the engine there was never initialised."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from nanopow import _lib\n"
            "lib = _lib.load()\n"
            "rc = lib.npow_promote(1, 8)\n"
            "print(rc, (lib.npow_last_error() or b'').decode())\n" % os.path.join(ROOT, "nano-dpow_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60, check=True).stdout
    rc, _, msg = out.strip().partition(" ")
    assert int(rc) == _lib.NPOW_ERR_NOT_INITIALISED and msg.strip(), out


def test_ticket_promote_needs_the_symbol():
    class OldLib:
        pass

    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = OldLib()
    t = _lib.Ticket(eng, 0, None)  # (ticket 0: nothing for __del__ to collect)
    with pytest.raises(_lib.NanoPowError) as e:
        t.promote(8)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    """The promotion helpers of npow_weights.h compiled into a small program: one line of numbers per query."""
    d = tmp_path_factory.mktemp("pw")
    src = d / "pw.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "npow_weights.h"
using namespace npow;
int main(int argc, char** argv) {
  if (!strcmp(argv[1], "word")) {  // gen wsh -> word gen wsh mirror
    const uint64_t gen = strtoull(argv[2], 0, 0);
    const uint32_t wsh = (uint32_t)atoi(argv[3]);
    const uint64_t w = pool_boost_word(gen, wsh);
    printf("%llu %llu %u %llu\n", (unsigned long long)w, (unsigned long long)pool_boost_gen(w), pool_boost_wsh(w),
           (unsigned long long)pool_boost_mirror(w));
  } else if (!strcmp(argv[1], "eff")) {  // word_gen word_wsh entry_gen own_wsh wdown -> effective shift
    const uint64_t m = pool_boost_mirror(pool_boost_word(strtoull(argv[2], 0, 0), (uint32_t)atoi(argv[3])));
    printf("%u\n", pool_eff_wsh(m, strtoull(argv[4], 0, 0), (uint32_t)atoi(argv[5]), (uint32_t)atoi(argv[6])));
  } else if (!strcmp(argv[1], "table")) {  // every (weight, wdown): wsh of the weight, promoted shift, table's shift
    for (uint32_t w = 1; w <= 8; w <<= 1)
      for (uint32_t k = 0; k <= 3; ++k)
        printf("%u %u %u %u %u\n", w, k, pool_wsh(w), pool_promoted_wsh(pool_wsh(w), k),
               pool_wsh((w >> k) ? (w >> k) : 1u));
  } else if (!strcmp(argv[1], "pingpong")) {  // sa sb: pairs (a, b) of counts 0..64 where a move and its reverse
    const uint32_t sa = (uint32_t)atoi(argv[2]), sb = (uint32_t)atoi(argv[3]);  // both qualify (none, one hopes)
    unsigned both = 0, moves = 0;
    for (unsigned long long a = 0; a <= 64; ++a)
      for (unsigned long long b = 0; b <= 64; ++b) {
        // a workgroup of B (b > 0) moves to A; then the reverse move from A (a + 1) to B (b - 1) must not qualify
        if (b > 0 && pool_should_move(a, sa, b, sb)) {
          ++moves;
          if (pool_should_move(b - 1, sb, a + 1, sa)) ++both;
        }
      }
    printf("%u %u\n", both, moves);
  }
  return 0;
}
''')
    exe = d / "pw"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
        return [[int(x) for x in ln.split()] for ln in out.splitlines()]
    return run


@pytest.mark.parametrize("gen", [1, 2, 12345, (1 << 40) + 7, (1 << 61) + 3])
@pytest.mark.parametrize("wsh", [0, 1, 2, 3])
def test_boost_word_round_trips(helpers, gen, wsh):
    (word, g, s, mirror), = helpers("word", gen, wsh)
    assert (g, s) == (gen, wsh) and word == (gen << 2) | wsh
    assert mirror == (gen << 2) | (3 - wsh)


def test_boost_mirror_grows_with_generation_and_weight(helpers):
    """The mirror is raised with an atomic max: a later generation, or a heavier weight of the same one, must
    compare greater."""
    def mirror(gen, wsh):
        return helpers("word", gen, wsh)[0][3]
    for gen in (1, 77):
        assert mirror(gen, 3) < mirror(gen, 2) < mirror(gen, 1) < mirror(gen, 0) < mirror(gen + 1, 3)


@pytest.mark.parametrize("own", [0, 1, 2, 3])
def test_effective_shift_falls_back_on_another_generation(helpers, own):
    for word_wsh in range(4):
        assert helpers("eff", 41, word_wsh, 42, own, 0) == [[own]]  # a word of the slot's previous job
        assert helpers("eff", 43, word_wsh, 42, own, 0) == [[own]]  # ... or of a later one
        assert helpers("eff", 0, word_wsh, 42, own, 0) == [[own]]   # ... or none yet (a zeroed mirror reads level 3!)
        assert helpers("eff", 42, word_wsh, 42, own, 0) == [[word_wsh]]


def test_promoted_shift_is_the_tables_for_every_weight_and_halving(helpers):
    rows = helpers("table")
    assert len(rows) == 16
    for w, k, wsh, promoted, table in rows:
        assert wsh == 3 - (w.bit_length() - 1)
        assert promoted == min(3, wsh + k)
        assert promoted == table  # what pool_table_weights / dyn_add give a job submitted at that weight
        assert helpers("eff", 9, wsh, 9, 3, k) == [[promoted]]


@pytest.mark.parametrize("sa,sb", list(itertools.product(range(4), repeat=2)))
def test_balancing_rule_never_trades_a_workgroup_back(helpers, sa, sb):
    """Every pair of (possibly promoted) shifts, counts 0..64: after a qualifying move the reverse does not qualify."""
    (both, moves), = helpers("pingpong", sa, sb)
    assert moves > 0 and both == 0
