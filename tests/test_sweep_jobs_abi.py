"""Sweep jobs (npow_submit_sweep / npow_wait_sweep): the C ABI surface, without a GPU.

The header declares both calls and the per-device hit capacity, the library exports them, the ctypes
wrapper binds them, and before npow_init both fail cleanly (never a CPU fallback).  The GPU behaviour
is tests/test_gpu_sweep_jobs.py.
"""
import ctypes
import os
import re
import subprocess
import sys

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")
SYMBOLS = ("npow_submit_sweep", "npow_wait_sweep")


def _declarations():
    txt = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls_and_the_capacity():
    code = _declarations()
    for s in SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", code), s
    m = re.search(r"#define NPOW_SWEEP_JOB_HITS (\d+)", code)
    assert m, "NPOW_SWEEP_JOB_HITS"
    cap = int(m.group(1))
    assert cap >= 1 << 20  # npow_sweep's device buffer
    assert cap == _lib.NPOW_SWEEP_JOB_HITS
    # the documented signatures, argument for argument
    sub = re.search(r"int npow_submit_sweep\s*\(([^)]*)\)", code).group(1)
    assert [a.split()[-1].strip("*") for a in sub.split(",")] == [
        "root[32]", "threshold", "start", "count", "device_mask", "cancel", "ticket"]
    wait = re.search(r"int npow_wait_sweep\s*\(([^)]*)\)", code).group(1)
    assert [a.split()[-1].strip("*") for a in wait.split(",")] == [
        "ticket", "timeout_us", "out", "cap", "n_out", "nonces_done"]


def test_library_exports_and_wrapper_binds_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (npow_\w+)$", out, flags=re.M))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in exported, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        f = getattr(lib, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(lib.npow_submit_sweep.argtypes) == 7
    assert len(lib.npow_wait_sweep.argtypes) == 6
    assert hasattr(_lib.Engine, "submit_sweep") and hasattr(_lib.SweepTicket, "wait")
    assert hasattr(_lib.SweepTicket, "cancel") and hasattr(_lib.SweepTicket, "__del__")


UNINITIALISED = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from nanopow import _lib
lib = _lib.load()
t = ctypes.c_uint64(0)
rc = lib.npow_submit_sweep(b"\x00" * 32, 0, 0, 64, 0, None, ctypes.byref(t))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED and t.value == 0, rc
assert lib.npow_last_error()
out = (ctypes.c_uint64 * 64)()
n, done = ctypes.c_uint64(0), ctypes.c_uint64(0)
rc = lib.npow_wait_sweep(1, 0, ctypes.addressof(out), 64, ctypes.byref(n), ctypes.byref(done))
assert rc == _lib.NPOW_ERR_NOT_INITIALISED and n.value == 0 and done.value == 0, rc
assert lib.npow_last_error()
# count == 0 is no way round it
assert lib.npow_submit_sweep(b"\x00" * 32, 0, 0, 0, 0, None, ctypes.byref(t)) == _lib.NPOW_ERR_NOT_INITIALISED
print("ok")
"""


def test_uninitialised_calls_fail_cleanly():
    """Before npow_init both calls return a negative status with npow_last_error() set and hash nothing on the
    CPU.  In a process of its own: npow_init is process-wide, and other tests of this run may have called it."""
    p = subprocess.run([sys.executable, "-c", UNINITIALISED, os.path.join(ROOT, "nano-dpow_amd")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
