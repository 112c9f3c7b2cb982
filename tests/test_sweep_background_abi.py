"""Background sweep jobs (npow_submit_sweep_background / npow_ticket_sweep): the C ABI surface, without a GPU.

The header declares both calls and the struct, the library exports them, the ctypes wrapper binds them, before
npow_init both fail cleanly, and the wrapper refuses `background=True` on a library without the symbol.  The GPU
behaviour is tests/test_gpu_sweep_background.py.
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")
SYMBOLS = ("npow_submit_sweep_background", "npow_ticket_sweep")
INFO_FIELDS = ["size", "background", "count", "nonces_done", "hits", "launches", "launches_cut", "held_us",
               "finished", "pad"]


def _declarations():
    txt = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls_and_the_struct():
    code = _declarations()
    for s in SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", code), s
    sub = re.search(r"int npow_submit_sweep_background\s*\(([^)]*)\)", code).group(1)
    plain = re.search(r"int npow_submit_sweep\s*\(([^)]*)\)", code).group(1)
    names = [a.split()[-1].strip("*") for a in sub.split(",")]
    assert names == ["root[32]", "threshold", "start", "count", "device_mask", "cancel", "ticket"]
    assert names == [a.split()[-1].strip("*") for a in plain.split(",")]  # the same arguments as npow_submit_sweep
    look = re.search(r"int npow_ticket_sweep\s*\(([^)]*)\)", code).group(1)
    assert re.sub(r"\s+", " ", look).strip() == "uint64_t ticket, npow_sweep_info* out"
    body = re.search(r"typedef struct npow_sweep_info \{(.*?)\} npow_sweep_info;", code, flags=re.S).group(1)
    fields = [f for decl in body.split(";") if decl.strip()
              for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert fields == INFO_FIELDS
    assert fields[0] == "size"  # written up to the caller's size
    # the header says what the class means
    assert re.search(r"starves", open(HEADER).read(), flags=re.I)


def test_wrapper_struct_matches_the_header():
    assert [f[0] for f in _lib._SweepInfoStruct._fields_] == INFO_FIELDS
    assert ctypes.sizeof(_lib._SweepInfoStruct) == 64
    for f in ("background", "nonces_done", "hits", "launches", "launches_cut", "held_us"):
        assert f in _lib.SweepInfo.__dataclass_fields__, f


def test_library_exports_and_wrapper_binds_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (npow_\w+)$", out, flags=re.M))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in exported, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        f = getattr(lib, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(lib.npow_submit_sweep_background.argtypes) == 7
    assert len(lib.npow_ticket_sweep.argtypes) == 2
    assert hasattr(_lib.SweepTicket, "info")
    import inspect
    p = inspect.signature(_lib.Engine.submit_sweep).parameters["background"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY  # without the keyword: unchanged


UNINITIALISED = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from nanopow import _lib
lib = _lib.load()
t = ctypes.c_uint64(0)
rc = lib.npow_submit_sweep_background(b"\x00" * 32, 0, 0, 64, 0, None, ctypes.byref(t))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED and t.value == 0, rc
assert lib.npow_last_error()
i = _lib._SweepInfoStruct()
i.size = ctypes.sizeof(i)
rc = lib.npow_ticket_sweep(1, ctypes.byref(i))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED, rc
assert lib.npow_last_error()
assert (i.background, i.nonces_done, i.hits, i.launches, i.launches_cut, i.held_us) == (0, 0, 0, 0, 0, 0)
# count == 0 is no way round it
rc = lib.npow_submit_sweep_background(b"\x00" * 32, 0, 0, 0, 0, None, ctypes.byref(t))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED, rc
print("ok")
"""


def test_uninitialised_calls_fail_cleanly():
    """Before npow_init both calls return a negative status with npow_last_error() set.  In a process of its own:
    npow_init is process-wide, and other tests of this run may have called it."""
    p = subprocess.run([sys.executable, "-c", UNINITIALISED, os.path.join(ROOT, "nano-dpow_amd")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


class _OldLib:
    """A library from before this call: it has npow_submit_sweep and nothing newer."""

    def npow_submit_sweep(self, *a):  # pragma: no cover - must not be reached
        raise AssertionError("the plain call was used for a background job")

    def npow_last_error(self):
        return b""


def test_background_on_a_library_without_the_symbol_raises():
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = _OldLib()
    with pytest.raises(_lib.NanoPowError) as e:
        eng.submit_sweep(b"\x00" * 32, 0, 0, 64, background=True)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    t = _lib.SweepTicket(eng, 7, None, 16)
    with pytest.raises(_lib.NanoPowError) as e:
        t.info()
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    t.ticket = 0  # (nothing to cancel at its deletion)
