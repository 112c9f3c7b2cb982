"""Shared range jobs (npow_submit_sweep_shared / npow_submit_best_shared / npow_ticket_share): the C ABI surface,
without a GPU.

The header declares the three calls and the struct within ABI 7, the library exports them, the ctypes wrapper binds
them and mirrors the struct byte for byte (a compiled C snippet tells its size and offsets), the existing structs keep
their sizes, before npow_init the calls fail as their siblings do, and the wrapper refuses `shared=True` beside
`background=True` and on a library without the symbols.  The GPU behaviour is tests/test_gpu_range_shared.py.
"""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")
SYMBOLS = ("npow_submit_sweep_shared", "npow_submit_best_shared", "npow_ticket_share")
SHARE_FIELDS = ["size", "klass", "launches", "launches_cut", "held_us", "moves"]


def _declarations():
    txt = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _args(code, name):
    return [a.split()[-1].strip("*") for a in re.search(rf"int {name}\s*\(([^)]*)\)", code).group(1).split(",")]


def test_header_declares_the_calls_and_the_struct():
    code = _declarations()
    for s in SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", code), s
    assert re.search(r"#define NPOW_ABI_VERSION 7\b", code)  # added within ABI 7: callers probe for the symbols
    assert _args(code, "npow_submit_sweep_shared") == _args(code, "npow_submit_sweep")
    assert _args(code, "npow_submit_sweep") == ["root[32]", "threshold", "start", "count", "device_mask", "cancel",
                                                "ticket"]
    assert _args(code, "npow_submit_best_shared") == _args(code, "npow_submit_best")
    look = re.search(r"int npow_ticket_share\s*\(([^)]*)\)", code).group(1)
    assert re.sub(r"\s+", " ", look).strip() == "uint64_t ticket, npow_range_share_info* out"
    body = re.search(r"typedef struct npow_range_share_info \{(.*?)\} npow_range_share_info;", code,
                     flags=re.S).group(1)
    fields = [f for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for f in re.split(r",\s*", decl)]
    assert fields == SHARE_FIELDS


SIZES = r"""
#include <stddef.h>
#include <stdio.h>
#include "nanopow.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(npow_range_share_info),
         offsetof(npow_range_share_info, size), offsetof(npow_range_share_info, klass),
         offsetof(npow_range_share_info, launches), offsetof(npow_range_share_info, launches_cut),
         offsetof(npow_range_share_info, held_us), offsetof(npow_range_share_info, moves),
         sizeof(npow_sweep_info), sizeof(npow_best_info), sizeof(npow_best_hold_info));
  return 0;
}
"""


def test_wrapper_struct_matches_the_compiled_header(tmp_path):
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text(SIZES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True, capture_output=True, text=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib._RangeShareStruct
    assert [f[0] for f in S._fields_] == SHARE_FIELDS
    assert got[0] == ctypes.sizeof(S) == 40
    assert got[1:7] == [getattr(S, f).offset for f in SHARE_FIELDS] == [0, 4, 8, 16, 24, 32]
    # no existing struct changed size
    assert got[7] == ctypes.sizeof(_lib._SweepInfoStruct) == 64
    assert got[8] == ctypes.sizeof(_lib._BestInfoStruct) == 72
    assert got[9] == ctypes.sizeof(_lib._BestHoldStruct) == 24
    for f in SHARE_FIELDS[1:]:
        assert f in _lib.RangeShare.__dataclass_fields__, f
    assert (_lib.RANGE_PLAIN, _lib.RANGE_BACKGROUND, _lib.RANGE_SHARED) == (0, 1, 2)


def test_library_exports_and_wrapper_binds_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (npow_\w+)$", out, flags=re.M))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in exported, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        f = getattr(lib, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(lib.npow_submit_sweep_shared.argtypes) == 7
    assert len(lib.npow_submit_best_shared.argtypes) == 7
    assert len(lib.npow_ticket_share.argtypes) == 2
    assert hasattr(_lib.SweepTicket, "share") and hasattr(_lib.BestTicket, "share")
    for call in (_lib.Engine.submit_sweep, _lib.Engine.submit_best):
        assert inspect.signature(call).parameters["shared"].default is False  # without the keyword: unchanged


UNINITIALISED = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from nanopow import _lib
lib = _lib.load()
t = ctypes.c_uint64(0)
want = lib.npow_submit_sweep(b"\x00" * 32, 0, 0, 64, 0, None, ctypes.byref(t))
assert want == _lib.NPOW_ERR_NOT_INITIALISED
for call in (lib.npow_submit_sweep_shared, lib.npow_submit_best_shared):
    for count in (64, 0):  # count == 0 is no way round it
        rc = call(b"\x00" * 32, 0, 0, count, 0, None, ctypes.byref(t))
        assert rc == want and t.value == 0, rc
        assert lib.npow_last_error()
s = _lib._RangeShareStruct()
s.size = ctypes.sizeof(s)
assert lib.npow_ticket_share(1, ctypes.byref(s)) == want
assert lib.npow_last_error()
assert (s.klass, s.launches, s.launches_cut, s.held_us, s.moves) == (0, 0, 0, 0, 0)
print("ok")
"""


def test_uninitialised_calls_fail_as_their_siblings_do():
    """Before npow_init the calls return a negative status with npow_last_error() set.  In a process of its own:
    npow_init is process-wide, and other tests of this run may have called it."""
    p = subprocess.run([sys.executable, "-c", UNINITIALISED, os.path.join(ROOT, "nano-dpow_amd")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


class _OldLib:
    """A library from before these calls: it has the plain and the background submits and nothing newer."""

    def _never(self, *a):  # pragma: no cover - must not be reached
        raise AssertionError("another class's call was used for a shared job")

    npow_submit_sweep = npow_submit_best = npow_submit_sweep_background = npow_submit_best_background = _never

    def npow_last_error(self):
        return b""


def test_shared_with_background_and_on_a_library_without_the_symbol_raises():
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = _OldLib()
    with pytest.raises(ValueError):
        eng.submit_sweep(b"\x00" * 32, 0, 0, 64, shared=True, background=True)
    with pytest.raises(ValueError):
        eng.submit_best(b"\x00" * 32, 0, 64, shared=True, background=True)
    with pytest.raises(_lib.NanoPowError) as e:
        eng.submit_sweep(b"\x00" * 32, 0, 0, 64, shared=True)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    with pytest.raises(_lib.NanoPowError) as e:
        eng.submit_best(b"\x00" * 32, 0, 64, shared=True)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    for t in (_lib.BestTicket(eng, 7, None), _lib.SweepTicket(eng, 8, None, 16)):
        with pytest.raises(_lib.NanoPowError) as e:
            t.share()
        assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
        t.ticket = 0  # (nothing to cancel at its deletion)
