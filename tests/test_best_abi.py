"""Best jobs (npow_submit_best / npow_wait_best / npow_ticket_best): the C ABI surface, without a GPU.

The header declares the calls with the documented arguments, the library exports them, the ctypes wrapper binds
them, and before npow_init each fails cleanly (never a CPU fallback).  The refusals between ticket kinds need live
tickets, so they are in tests/test_gpu_best.py.
"""
import ctypes
import os
import re
import subprocess
import sys

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")
SYMBOLS = ("npow_submit_best", "npow_wait_best", "npow_ticket_best")


def _declarations():
    txt = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _args(code, name):
    return [a.split()[-1].strip("*") for a in re.search(rf"int {name}\s*\(([^)]*)\)", code).group(1).split(",")]


def test_header_declares_the_calls():
    code = _declarations()
    for s in SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", code), s
    assert _args(code, "npow_submit_best") == ["root[32]", "floor", "start", "count", "device_mask", "cancel", "ticket"]
    assert _args(code, "npow_wait_best") == ["ticket", "timeout_us", "nonce_out", "value_out", "nonces_done"]
    assert _args(code, "npow_ticket_best") == ["ticket", "out"]
    assert re.search(r"#define NPOW_ABI_VERSION 7\b", code)  # added within ABI 7: callers probe for the symbols
    # the info struct the wrapper mirrors, field for field
    body = re.search(r"typedef struct npow_best_info \{(.*?)\} npow_best_info;", code, flags=re.S).group(1)
    fields = [f for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for f in re.split(r",\s*", decl)]
    assert fields == [n for n, _ in _lib._BestInfoStruct._fields_]
    assert ctypes.sizeof(_lib._BestInfoStruct) == 8 + 8 * 8


def test_library_exports_and_wrapper_binds_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (npow_\w+)$", out, flags=re.M))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in exported, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        f = getattr(lib, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(lib.npow_submit_best.argtypes) == 7
    assert len(lib.npow_wait_best.argtypes) == 5
    assert hasattr(_lib.Engine, "submit_best")
    for m in ("wait", "cancel", "info", "__del__"):
        assert hasattr(_lib.BestTicket, m), m
    # wait() gives status, nonce, value, nonces_done
    assert tuple(_lib.BestResult(_lib.NPOW_OK, 5, 7, 9)) == (_lib.NPOW_OK, 5, 7, 9)


UNINITIALISED = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from nanopow import _lib
lib = _lib.load()
t = ctypes.c_uint64(0)
rc = lib.npow_submit_best(b"\x00" * 32, 0, 0, 64, 0, None, ctypes.byref(t))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED and t.value == 0, rc
assert lib.npow_last_error()
nonce, value, done = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
rc = lib.npow_wait_best(1, 0, ctypes.byref(nonce), ctypes.byref(value), ctypes.byref(done))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED and (nonce.value, value.value, done.value) == (0, 0, 0), rc
assert lib.npow_last_error()
info = _lib._BestInfoStruct()
info.size = ctypes.sizeof(info)
assert lib.npow_ticket_best(1, ctypes.byref(info)) == _lib.NPOW_ERR_NOT_INITIALISED
# count == 0 is no way round it
assert lib.npow_submit_best(b"\x00" * 32, 0, 0, 0, 0, None, ctypes.byref(t)) == _lib.NPOW_ERR_NOT_INITIALISED
print("ok")
"""


def test_uninitialised_calls_fail_cleanly():
    """Before npow_init every call returns a negative status with npow_last_error() set and hashes nothing on the
    CPU.  In a process of its own: npow_init is process-wide, and other tests of this run may have called it."""
    p = subprocess.run([sys.executable, "-c", UNINITIALISED, os.path.join(ROOT, "nano-dpow_amd")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
