"""Retargeting (npow_retarget) on the CPU side: the declaration, the status code and the export, the three fields
npow_search_info gains and their mirror in nanopow._lib, and the call before npow_init.  No GPU here; the search
itself is exercised in tests/test_gpu_retarget.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")


def test_header_declares_npow_retarget_within_abi_7():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+npow_retarget\s*\(([^)]*)\)", txt)
    assert m, "include/nanopow.h does not declare npow_retarget"
    assert [a.strip() for a in m.group(1).split(",")] == ["uint64_t ticket", "uint64_t threshold"]
    assert re.search(r"#define\s+NPOW_TOO_LATE\s+(\S+)", txt).group(1) == "4"
    assert _lib.NPOW_TOO_LATE == 4
    assert re.search(r"#define NPOW_ABI_VERSION (\d+)", txt).group(1) == "7"
    assert _lib.NPOW_ABI_VERSION == 7
    # the revision comment names the addition
    rev = raw[raw.index("ABI revision"):raw.index("#define NPOW_ABI_VERSION")]
    assert "npow_retarget" in rev and "stale_hits" in rev


def test_too_late_is_no_other_status():
    codes = [_lib.NPOW_OK, _lib.NPOW_CANCELLED, _lib.NPOW_EXHAUSTED, _lib.NPOW_PENDING, _lib.NPOW_TOO_LATE]
    assert len(set(codes)) == len(codes) and all(c >= 0 for c in codes)


def test_library_exports_npow_retarget():
    lib = _lib.load()
    assert hasattr(lib, "npow_retarget")
    assert "npow_retarget" in _lib.EXPORTED_SYMBOLS
    assert lib.npow_abi_version() == 7
    assert callable(getattr(_lib.Ticket, "retarget", None))


def test_search_info_ends_with_the_retarget_fields():
    names = [f[0] for f in _lib.SearchInfo._fields_]
    assert names[-4:] == ["win_seen_us", "retargets", "stale_hits", "stale_wins"]
    for n in names[-3:]:
        assert getattr(_lib.SearchInfo, n).size == 8
    assert _lib.SearchInfo.stale_wins.offset == ctypes.sizeof(_lib.SearchInfo) - 8


def test_search_info_matches_the_header(tmp_path):
    """Size and every field's offset, from a C compiler's view of include/nanopow.h."""
    names = [f[0] for f in _lib.SearchInfo._fields_]
    src = tmp_path / "si.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"nanopow.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(npow_search_info));\n" +
                   "".join(f"  printf(\"{n} %zu\\n\", offsetof(npow_search_info, {n}));\n" for n in names) +
                   "  return 0;\n}\n")
    exe = tmp_path / "si"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert int(out[0]) == ctypes.sizeof(_lib.SearchInfo)
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out[1:]}
    assert got == {n: getattr(_lib.SearchInfo, n).offset for n in names}


def test_retarget_before_init_is_an_error_with_a_message():
    """In a process of its own: the engine there was never initialised."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from nanopow import _lib\n"
            "lib = _lib.load()\n"
            "rc = lib.npow_retarget(1, 0xfffffff800000000)\n"
            "print(rc, (lib.npow_last_error() or b'').decode())\n" % os.path.join(ROOT, "nano-dpow_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60, check=True).stdout
    rc, _, msg = out.strip().partition(" ")
    assert int(rc) == _lib.NPOW_ERR_NOT_INITIALISED and msg.strip(), out


def _ticket(lib):
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = lib
    return _lib.Ticket(eng, 0, None)  # (ticket 0: nothing for __del__ to collect)


def test_ticket_retarget_needs_the_symbol():
    class OldLib:
        pass

    with pytest.raises(_lib.NanoPowError) as e:
        _ticket(OldLib()).retarget(1 << 63)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


def test_ticket_retarget_maps_the_status_to_a_bool():
    class Lib:
        def __init__(self, rc):
            self.rc, self.calls = rc, []

        def npow_retarget(self, ticket, threshold):
            self.calls.append((ticket, threshold))
            return self.rc

        def npow_last_error(self):
            return b"unknown ticket"

    ok, late, bad = Lib(_lib.NPOW_OK), Lib(_lib.NPOW_TOO_LATE), Lib(_lib.NPOW_ERR_BAD_ARGUMENT)
    assert _ticket(ok).retarget(0xfffffffe00000000) is True and ok.calls == [(0, 0xfffffffe00000000)]
    assert _ticket(late).retarget(5) is False
    with pytest.raises(_lib.NanoPowError) as e:
        _ticket(bad).retarget(5)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    for wrong in (-1, 1 << 64, 1.5, True, "ff"):
        with pytest.raises(_lib.NanoPowError):
            _ticket(ok).retarget(wrong)
    assert len(ok.calls) == 1
    t = _ticket(ok)
    t.result = _lib.SearchResult(_lib.NPOW_CANCELLED, None, None, 0)  # collected
    with pytest.raises(_lib.NanoPowError):
        t.retarget(5)
