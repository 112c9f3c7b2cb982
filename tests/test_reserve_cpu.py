"""Reserve hits (npow_submit_reserve, npow_ticket_reserve, npow_relax) on the CPU side: the declarations within ABI 7,
the export, npow_reserve_info and its mirror in nanopow._lib, the calls before npow_init, and the Python wrappers'
mapping of the statuses.  No GPU here; the search itself is exercised in tests/test_gpu_reserve.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from nanopow import _lib

HEADER = os.path.join(ROOT, "include", "nanopow.h")
NEW = ("npow_submit_reserve", "npow_ticket_reserve", "npow_relax")


def _decl(txt, name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, f"include/nanopow.h does not declare {name}"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_the_reserve_calls_within_abi_7():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert _decl(txt, "npow_submit_reserve") == [
        "const uint8_t root[32]", "uint64_t threshold", "uint64_t reserve", "uint64_t start", "uint64_t device_mask",
        "const volatile uint32_t* cancel", "uint32_t weight", "uint32_t background", "uint64_t* ticket"]
    assert _decl(txt, "npow_ticket_reserve") == ["uint64_t ticket", "npow_reserve_info* out"]
    assert _decl(txt, "npow_relax") == ["uint64_t ticket", "uint64_t threshold", "uint32_t* answered"]
    assert re.search(r"#define\s+NPOW_RESERVE_MIN\s+(\S+)", txt).group(1) == "0xfffff00000000000ull"
    assert _lib.NPOW_RESERVE_MIN == 0xfffff00000000000
    assert re.search(r"#define NPOW_ABI_VERSION (\d+)", txt).group(1) == "7"
    assert _lib.NPOW_ABI_VERSION == 7
    rev = raw[raw.index("ABI revision"):raw.index("#define NPOW_ABI_VERSION")]
    for name in NEW:
        assert name in rev  # the revision comment names the additions


def test_library_exports_the_reserve_calls():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    assert lib.npow_abi_version() == 7
    for meth in ("reserve", "reserve_info", "relax"):
        assert callable(getattr(_lib.Ticket, meth, None))


def test_reserve_info_matches_the_header(tmp_path):
    """Size and every field's offset, from a C compiler's view of include/nanopow.h."""
    names = [f[0] for f in _lib.ReserveInfo._fields_]
    assert names == ["size", "armed", "reserve_threshold", "threshold", "nonce", "value", "device", "answered",
                     "relaxes", "candidates"]
    src = tmp_path / "ri.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"nanopow.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(npow_reserve_info));\n" +
                   "".join(f"  printf(\"{n} %zu\\n\", offsetof(npow_reserve_info, {n}));\n" for n in names) +
                   "  return 0;\n}\n")
    exe = tmp_path / "ri"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert int(out[0]) == ctypes.sizeof(_lib.ReserveInfo) == 64
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out[1:]}
    assert got == {n: getattr(_lib.ReserveInfo, n).offset for n in names}


def test_search_info_and_device_stats_are_unchanged():
    """The new facts travel in npow_reserve_info: the two older structs keep their size and their last field."""
    assert ctypes.sizeof(_lib.SearchInfo) == 144 and _lib.SearchInfo._fields_[-1][0] == "stale_wins"
    assert ctypes.sizeof(_lib.DeviceStats) == 224 and _lib.DeviceStats._fields_[-1][0] == "promotions"


def test_reserve_calls_before_init_are_errors_with_a_message():
    """In a process of its own: the engine there was never initialised."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from nanopow import _lib\n"
            "lib = _lib.load()\n"
            "info = _lib.ReserveInfo(); info.size = ctypes.sizeof(info)\n"
            "ans, t = ctypes.c_uint32(7), ctypes.c_uint64(0)\n"
            "for rc in (lib.npow_relax(1, 0xfffffff800000000, ctypes.byref(ans)), lib.npow_relax(1, 0, None),\n"
            "           lib.npow_ticket_reserve(1, ctypes.byref(info)), lib.npow_ticket_reserve(1, None),\n"
            "           lib.npow_submit_reserve(b'\\0' * 32, 2**64 - 1, 0xfffffff800000000, 0, 0, None, 1, 0,\n"
            "                                   ctypes.byref(t))):\n"
            "    print(rc, (lib.npow_last_error() or b'').decode())\n"
            "print(info.value, t.value)\n" % os.path.join(ROOT, "nano-dpow_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60, check=True).stdout
    lines = out.strip().splitlines()
    assert len(lines) == 6, out
    for ln in lines[:5]:
        rc, _, msg = ln.partition(" ")
        assert int(rc) == _lib.NPOW_ERR_NOT_INITIALISED and msg.strip(), out
    assert lines[5] == "0 0"


def _ticket(lib):
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = lib
    return _lib.Ticket(eng, 0, None)  # (ticket 0: nothing for __del__ to collect)


def test_ticket_calls_need_the_symbols():
    class OldLib:
        pass

    for call in (lambda t: t.relax(1 << 63), lambda t: t.reserve(), lambda t: t.reserve_info()):
        with pytest.raises(_lib.NanoPowError) as e:
            call(_ticket(OldLib()))
        assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = OldLib()
    with pytest.raises(_lib.NanoPowError) as e:
        eng.submit(b"\0" * 32, (1 << 64) - 1, reserve=_lib.NPOW_RESERVE_MIN)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


class _Lib:
    def __init__(self, rc, answered=0, held=(0, 0)):
        self.rc, self.answered, self.held, self.calls = rc, answered, held, []

    def npow_relax(self, ticket, threshold, answered):
        self.calls.append((ticket, threshold))
        answered._obj.value = self.answered
        return self.rc

    def npow_ticket_reserve(self, ticket, out):
        out._obj.nonce, out._obj.value = self.held
        out._obj.armed = 1
        return self.rc

    def npow_last_error(self):
        return b"unknown ticket"


def test_ticket_relax_maps_the_status():
    yes, no = _Lib(_lib.NPOW_OK, 1), _Lib(_lib.NPOW_OK, 0)
    late, bad = _Lib(_lib.NPOW_TOO_LATE), _Lib(_lib.NPOW_ERR_BAD_ARGUMENT)
    assert _ticket(yes).relax(0xfffffe0000000000) is True and yes.calls == [(0, 0xfffffe0000000000)]
    assert _ticket(no).relax(5) is False
    assert _ticket(late).relax(5) is None
    with pytest.raises(_lib.NanoPowError) as e:
        _ticket(bad).relax(5)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    for wrong in (-1, 1 << 64, 1.5, True, "ff"):
        with pytest.raises(_lib.NanoPowError):
            _ticket(yes).relax(wrong)
    assert len(yes.calls) == 1
    t = _ticket(yes)
    t.result = _lib.SearchResult(_lib.NPOW_CANCELLED, None, None, 0)  # collected
    with pytest.raises(_lib.NanoPowError):
        t.relax(5)
    with pytest.raises(_lib.NanoPowError):
        t.reserve()


def test_ticket_reserve_is_none_until_a_value_is_held():
    assert _ticket(_Lib(_lib.NPOW_OK)).reserve() is None
    r = _ticket(_Lib(_lib.NPOW_OK, held=(0xabc, 0xfffffff900000000))).reserve()
    assert (r.status, r.nonce, r.value, r.nonces_done) == (_lib.NPOW_OK, 0xabc, 0xfffffff900000000, 0)
    with pytest.raises(_lib.NanoPowError):
        _ticket(_Lib(_lib.NPOW_ERR_BAD_ARGUMENT)).reserve()


def test_submit_passes_the_reserve_only_to_npow_submit_reserve():
    class Lib:
        def __init__(self):
            self.calls = []

        def npow_submit_reserve(self, *a):
            self.calls.append(("reserve",) + a[1:8])
            a[8]._obj.value = 0
            return _lib.NPOW_OK

        def npow_submit_weighted(self, *a):
            self.calls.append(("weighted",) + a[1:7])
            a[7]._obj.value = 0
            return _lib.NPOW_OK

    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = Lib()
    eng.submit(b"\1" * 32, 0xfffffff800000000, start=5, weight=2)
    eng.submit(b"\1" * 32, 0xfffffff800000000, start=5, weight=2, reserve=0xfffffe0000000000)
    eng.submit(b"\1" * 32, 0xfffffff800000000, background=True, reserve=0xfffffe0000000000)
    assert eng.lib.calls == [("weighted", 0xfffffff800000000, 5, 0, 0, None, 2),
                             ("reserve", 0xfffffff800000000, 0xfffffe0000000000, 5, 0, None, 2, 0),
                             ("reserve", 0xfffffff800000000, 0xfffffe0000000000, 0, 0, None, 1, 1)]
    for bad in (dict(reserve=-1), dict(reserve=1 << 64), dict(reserve=True), dict(reserve=5, max_nonces_per_device=64),
                dict(reserve=5, background=True, weight=2)):
        with pytest.raises(_lib.NanoPowError):
            eng.submit(b"\1" * 32, 0xfffffff800000000, **bad)
    assert len(eng.lib.calls) == 3
