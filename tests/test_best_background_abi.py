"""Background best jobs (npow_submit_best_background / npow_ticket_best_hold): the C ABI surface, without a GPU.

The header declares both calls and the struct within ABI 7, the library exports them, the ctypes wrapper binds them
and mirrors the struct byte for byte (a compiled C snippet tells its size and offsets), before npow_init both fail as
their siblings do, and the wrapper refuses `background=True` on a library without the symbol.  The GPU behaviour is
tests/test_gpu_best_background.py.
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
SYMBOLS = ("npow_submit_best_background", "npow_ticket_best_hold")
HOLD_FIELDS = ["size", "background", "launches_cut", "held_us"]


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
    # the same arguments as npow_submit_best
    assert _args(code, "npow_submit_best_background") == _args(code, "npow_submit_best")
    assert _args(code, "npow_submit_best") == ["root[32]", "floor", "start", "count", "device_mask", "cancel", "ticket"]
    look = re.search(r"int npow_ticket_best_hold\s*\(([^)]*)\)", code).group(1)
    assert re.sub(r"\s+", " ", look).strip() == "uint64_t ticket, npow_best_hold_info* out"
    body = re.search(r"typedef struct npow_best_hold_info \{(.*?)\} npow_best_hold_info;", code, flags=re.S).group(1)
    fields = [f for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for f in re.split(r",\s*", decl)]
    assert fields == HOLD_FIELDS
    # the header says what the class means, for best jobs too
    txt = open(HEADER).read()
    at = txt.index("Background best jobs")
    assert re.search(r"starves", txt[at:txt.index("int npow_submit_best_background", at)], flags=re.I)


SIZES = r"""
#include <stddef.h>
#include <stdio.h>
#include "nanopow.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(npow_best_hold_info), offsetof(npow_best_hold_info, size),
         offsetof(npow_best_hold_info, background), offsetof(npow_best_hold_info, launches_cut),
         offsetof(npow_best_hold_info, held_us), sizeof(npow_best_info));
  return 0;
}
"""


def test_wrapper_struct_matches_the_compiled_header(tmp_path):
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text(SIZES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True, capture_output=True, text=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib._BestHoldStruct
    assert [f[0] for f in S._fields_] == HOLD_FIELDS
    assert got[0] == ctypes.sizeof(S) == 24
    assert got[1:5] == [getattr(S, f).offset for f in HOLD_FIELDS] == [0, 4, 8, 16]
    assert got[5] == ctypes.sizeof(_lib._BestInfoStruct) == 72  # npow_best_info did not grow
    for f in ("background", "launches_cut", "held_us"):
        assert f in _lib.BestHold.__dataclass_fields__, f
    assert tuple(_lib.BestHold(1, 2, 3)) == (1, 2, 3)


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
    assert len(lib.npow_submit_best_background.argtypes) == 7
    assert len(lib.npow_ticket_best_hold.argtypes) == 2
    assert hasattr(_lib.BestTicket, "hold")
    p = inspect.signature(_lib.Engine.submit_best).parameters["background"]
    assert p.default is False  # without the keyword: unchanged


UNINITIALISED = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from nanopow import _lib
lib = _lib.load()
t = ctypes.c_uint64(0)
# what the siblings return (npow_submit_best, npow_ticket_best) ...
want_submit = lib.npow_submit_best(b"\x00" * 32, 0, 0, 64, 0, None, ctypes.byref(t))
info = _lib._BestInfoStruct()
info.size = ctypes.sizeof(info)
want_look = lib.npow_ticket_best(1, ctypes.byref(info))
assert want_submit == want_look == _lib.NPOW_ERR_NOT_INITIALISED
# ... is what these return
rc = lib.npow_submit_best_background(b"\x00" * 32, 0, 0, 64, 0, None, ctypes.byref(t))
assert rc == want_submit and t.value == 0, rc
assert lib.npow_last_error()
h = _lib._BestHoldStruct()
h.size = ctypes.sizeof(h)
rc = lib.npow_ticket_best_hold(1, ctypes.byref(h))
assert rc == want_look, rc
assert lib.npow_last_error()
assert (h.background, h.launches_cut, h.held_us) == (0, 0, 0)
# count == 0 is no way round it
assert lib.npow_submit_best_background(b"\x00" * 32, 0, 0, 0, 0, None, ctypes.byref(t)) == want_submit
print("ok")
"""


def test_uninitialised_calls_fail_as_their_siblings_do():
    """Before npow_init both calls return a negative status with npow_last_error() set.  In a process of its own:
    npow_init is process-wide, and other tests of this run may have called it."""
    p = subprocess.run([sys.executable, "-c", UNINITIALISED, os.path.join(ROOT, "nano-dpow_amd")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


class _OldLib:
    """A library from before these calls: it has npow_submit_best and nothing newer."""

    def npow_submit_best(self, *a):  # pragma: no cover - must not be reached
        raise AssertionError("the plain call was used for a background job")

    def npow_last_error(self):
        return b""


def test_background_on_a_library_without_the_symbol_raises():
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = _OldLib()
    with pytest.raises(_lib.NanoPowError) as e:
        eng.submit_best(b"\x00" * 32, 0, 64, background=True)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    t = _lib.BestTicket(eng, 7, None)
    with pytest.raises(_lib.NanoPowError) as e:
        t.hold()
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    t.ticket = 0  # (nothing to cancel at its deletion)
