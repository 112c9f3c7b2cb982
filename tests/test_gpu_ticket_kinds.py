"""Every ticket call on a ticket of every kind (a search, a sweep job, a best job): 13 calls x 3 kinds, each return
code and npow_last_error() message against tests/golden/ticket_kind_errors.json (recorded by
tests/golden/gen_ticket_kind_errors.py, which runs calls() below).

The wrong-kind calls come first: each is refused with NPOW_ERR_BAD_ARGUMENT and leaves the job untouched.  Then a
ticket's own calls, in an order whose answers do not depend on timing -- the looks, the calls that change nothing
(a promotion to weight 1, a retarget to the threshold the search has), the cancel once the job is over (a no-op) --
and last its own wait, whose result is checked against the oracle: the hit set, the maximum, value >= threshold.

One job of each kind on device 0, the shapes of the refusal tests in test_gpu_sweep_jobs.py and test_gpu_best.py:
the receive threshold, 65,537 nonces, floor 0.
"""
import ctypes
import time

import numpy as np
import pytest

import oracle
from conftest import load_golden
from nanopow import _lib

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RECEIVE = 0xfffffe0000000000
ROOT_A = bytes(range(3, 35))
START = 0x0123456789abcdef
N = 65537
KINDS = ("search", "sweep", "best")
CALLS = ("npow_wait", "npow_wait_info", "npow_wait_result", "npow_ticket_background", "npow_promote", "npow_retarget",
         "npow_relax", "npow_ticket_reserve", "npow_wait_sweep", "npow_ticket_sweep", "npow_wait_best",
         "npow_ticket_best", "npow_cancel")
# the calls that belong to a kind (npow_cancel to all of them); every other call on its ticket is a wrong-kind call
OWN = {"search": ("npow_ticket_background", "npow_promote", "npow_retarget", "npow_relax", "npow_ticket_reserve",
                  "npow_wait_result", "npow_cancel", "npow_wait_info", "npow_wait"),
       "sweep": ("npow_ticket_sweep", "npow_cancel", "npow_wait_sweep"),
       "best": ("npow_ticket_best", "npow_cancel", "npow_wait_best")}


class Caller:
    """The 13 calls on one ticket number, each with arguments that are valid for a ticket of the call's own kind;
    call() returns (return code, message) and keeps what the call wrote."""

    def __init__(self, lib, ticket):
        self.lib, self.ticket = lib, ticket
        self.nonce, self.value, self.done = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.n, self.u32 = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self.hits = (ctypes.c_uint64 * N)()
        self.info, self.rinfo = _lib.SearchInfo(), _lib.ReserveInfo()
        self.sinfo, self.binfo = _lib._SweepInfoStruct(), _lib._BestInfoStruct()
        for s in (self.info, self.rinfo, self.sinfo, self.binfo):
            s.size = ctypes.sizeof(s)

    def call(self, name, timeout_us=0):
        lib, t, ref = self.lib, self.ticket, ctypes.byref
        rc = {
            "npow_wait": lambda: lib.npow_wait(t, timeout_us, ref(self.nonce), ref(self.value), ref(self.done)),
            "npow_wait_info": lambda: lib.npow_wait_info(t, timeout_us, ref(self.info)),
            "npow_wait_result": lambda: lib.npow_wait_result(t, timeout_us, ref(self.nonce), ref(self.value)),
            "npow_ticket_background": lambda: lib.npow_ticket_background(t, ref(self.u32)),
            "npow_promote": lambda: lib.npow_promote(t, 1),
            "npow_retarget": lambda: lib.npow_retarget(t, RECEIVE),
            "npow_relax": lambda: lib.npow_relax(t, RECEIVE, ref(self.u32)),
            "npow_ticket_reserve": lambda: lib.npow_ticket_reserve(t, ref(self.rinfo)),
            "npow_wait_sweep": lambda: lib.npow_wait_sweep(t, timeout_us, ctypes.addressof(self.hits), N, ref(self.n),
                                                           ref(self.done)),
            "npow_ticket_sweep": lambda: lib.npow_ticket_sweep(t, ref(self.sinfo)),
            "npow_wait_best": lambda: lib.npow_wait_best(t, timeout_us, ref(self.nonce), ref(self.value),
                                                         ref(self.done)),
            "npow_ticket_best": lambda: lib.npow_ticket_best(t, ref(self.binfo)),
            "npow_cancel": lambda: lib.npow_cancel(t),
        }[name]()
        return rc, ((lib.npow_last_error() or b"").decode() if rc < 0 else "")


def _until_finished(c, look, info, timeout=30.0):
    deadline = time.time() + timeout
    while time.time() < deadline:
        rc, msg = c.call(look)
        assert rc == _lib.NPOW_OK, (look, rc, msg)
        if info.finished:
            return rc, msg
        time.sleep(0.0005)
    raise AssertionError(f"{look}: the job did not finish in {timeout} s")


def calls(engine):
    """{kind: {call: [return code, message]}} of the 13 calls on a ticket of each kind, and each job's result as its
    own wait returned it: {kind: Caller}."""
    lib = engine.lib
    tickets = {"search": engine.submit(ROOT_A, RECEIVE, start=START, device_mask=1),
               "sweep": engine.submit_sweep(ROOT_A, RECEIVE, START, N, device_mask=1, cap=N),
               "best": engine.submit_best(ROOT_A, START, N, device_mask=1)}
    callers = {k: Caller(lib, t.ticket) for k, t in tickets.items()}
    got = {k: {} for k in KINDS}
    for kind in KINDS:  # wrong-kind calls first, on every ticket
        for name in CALLS:
            if name not in OWN[kind]:
                got[kind][name] = list(callers[kind].call(name))
    for kind in KINDS:
        c = callers[kind]
        for name in OWN[kind]:
            if name == "npow_ticket_sweep":
                got[kind][name] = list(_until_finished(c, name, c.sinfo))
            elif name == "npow_ticket_best":
                got[kind][name] = list(_until_finished(c, name, c.binfo))
            elif name == "npow_wait_info":  # npow_wait collects the search: what npow_wait_info then says of the
                continue                    # released ticket, after it
            else:
                got[kind][name] = list(c.call(name, timeout_us=30_000_000))
    got["search"]["npow_wait_info"] = list(callers["search"].call("npow_wait_info"))
    for t in tickets.values():  # collected through the C ABI: nothing is left for the Python tickets to collect
        t.ticket, t.result = 0, object()
    return got, callers


@pytest.fixture(scope="module")
def outcome(gpu_engine):
    return calls(gpu_engine)


def test_all_39_calls_are_recorded(outcome):
    golden = load_golden("ticket_kind_errors.json")["kinds"]
    assert sorted(golden) == sorted(KINDS)
    for kind in KINDS:
        assert sorted(golden[kind]) == sorted(CALLS), kind
        assert sorted(outcome[0][kind]) == sorted(CALLS), kind


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_kind_calls_are_refused_with_the_recorded_message(outcome, kind):
    golden = load_golden("ticket_kind_errors.json")["kinds"][kind]
    for name in CALLS:
        if name in OWN[kind]:
            continue
        rc, msg = outcome[0][kind][name]
        print(kind, name, rc, msg)
        assert golden[name][0] == _lib.NPOW_ERR_BAD_ARGUMENT and golden[name][1], (kind, name, golden[name])
        assert [rc, msg] == golden[name], (kind, name)


@pytest.mark.parametrize("kind", KINDS)
def test_own_calls_answer_as_recorded(outcome, kind):
    golden = load_golden("ticket_kind_errors.json")["kinds"][kind]
    for name in OWN[kind]:
        rc, msg = outcome[0][kind][name]
        print(kind, name, rc, msg)
        assert [rc, msg] == golden[name], (kind, name)


def test_the_refused_jobs_finish_exact(outcome):
    got, c = outcome
    assert got["search"]["npow_wait"][0] == _lib.NPOW_OK
    s = c["search"]
    assert oracle.work_value_hashlib(ROOT_A, s.nonce.value) == s.value.value >= RECEIVE
    assert got["sweep"]["npow_wait_sweep"][0] == _lib.NPOW_OK
    w = c["sweep"]
    want = oracle.sweep(ROOT_A, RECEIVE, START, N)
    assert w.n.value == len(want) and list(w.hits[:w.n.value]) == want and w.done.value == N
    assert got["best"]["npow_wait_best"][0] == _lib.NPOW_OK
    b = c["best"]
    v = oracle.work_values_range(ROOT_A, START, N)
    k = int(np.argmax(v))
    assert (b.nonce.value, b.value.value, b.done.value) == ((START + k) & M64, int(v[k]), N)
