"""What the three ticket classes of nanopow._lib (Ticket, SweepTicket, BestTicket) share, against a fake library that
records its calls: an abandoned ticket is cancelled and collected by its own kind's wait, a collected one makes no
call, the timeout's conversion to microseconds, and the guard for a library that lacks a call.  No GPU here; the
library's side of the ticket kinds is tests/test_gpu_ticket_kinds.py."""
import gc

import pytest

from nanopow import _lib

ABANDON_US = 10_000_000


class FakeLib:
    """Every wait returns `wait_rc`; each call is recorded as (name, ticket, ...)."""

    def __init__(self, wait_rc=_lib.NPOW_CANCELLED):
        self.wait_rc, self.calls = wait_rc, []

    def npow_cancel(self, ticket):
        self.calls.append(("npow_cancel", ticket))
        return _lib.NPOW_OK

    def npow_wait(self, ticket, us, nonce, value, done):
        self.calls.append(("npow_wait", ticket, us))
        return self.wait_rc

    def npow_wait_result(self, ticket, us, nonce, value):
        self.calls.append(("npow_wait_result", ticket, us))
        return self.wait_rc

    def npow_wait_info(self, ticket, us, info):
        self.calls.append(("npow_wait_info", ticket, us))
        return self.wait_rc

    def npow_wait_sweep(self, ticket, us, out, cap, n_out, done):
        self.calls.append(("npow_wait_sweep", ticket, us, cap))
        return self.wait_rc

    def npow_wait_best(self, ticket, us, nonce, value, done):
        self.calls.append(("npow_wait_best", ticket, us))
        return self.wait_rc

    def npow_last_error(self):
        return b"fake"


def _engine(lib):
    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = lib
    return eng


def _make(kind, lib, ticket=7, cancel=None):
    if kind == "search":
        return _lib.Ticket(_engine(lib), ticket, cancel)
    if kind == "sweep":
        return _lib.SweepTicket(_engine(lib), ticket, cancel, 16)
    return _lib.BestTicket(_engine(lib), ticket, cancel)


OWN_WAIT = {"search": ("npow_wait", 7, ABANDON_US),
            "sweep": ("npow_wait_sweep", 7, ABANDON_US, 0),
            "best": ("npow_wait_best", 7, ABANDON_US)}
KINDS = sorted(OWN_WAIT)


@pytest.mark.parametrize("kind", KINDS)
def test_an_abandoned_ticket_is_cancelled_and_collected_by_its_own_wait(kind):
    lib = FakeLib()
    t = _make(kind, lib, cancel=_lib.CancelToken())
    before = len(_lib._ORPHANED_CANCEL_WORDS)
    del t
    gc.collect()
    assert lib.calls == [("npow_cancel", 7), OWN_WAIT[kind]]
    assert len(_lib._ORPHANED_CANCEL_WORDS) == before  # collected: the cancel word may go


@pytest.mark.parametrize("kind", KINDS)
def test_a_job_that_outlives_the_wait_keeps_its_cancel_word(kind):
    lib = FakeLib(_lib.NPOW_PENDING)
    token = _lib.CancelToken()
    t = _make(kind, lib, cancel=token)
    del t
    gc.collect()
    assert lib.calls == [("npow_cancel", 7), OWN_WAIT[kind]]
    assert _lib._ORPHANED_CANCEL_WORDS[-1] is token
    _lib._ORPHANED_CANCEL_WORDS.pop()


@pytest.mark.parametrize("kind", KINDS)
def test_a_collected_ticket_makes_no_call_when_dropped(kind):
    lib = FakeLib()
    t = _make(kind, lib, cancel=_lib.CancelToken())
    r = t.wait()
    assert r is not None and r.status == _lib.NPOW_CANCELLED and t.cancel_token is None
    assert t.wait() is r  # the result is kept
    t.cancel()            # ... and nothing is left to cancel
    n = len(lib.calls)
    assert n == 1
    del t
    gc.collect()
    assert len(lib.calls) == n
    # ticket 0 (nothing was submitted): no call either
    t = _make(kind, lib, ticket=0)
    del t
    gc.collect()
    assert len(lib.calls) == n


def test_only_a_search_keeps_its_ticket_number_once_collected():
    got = {}
    for kind in KINDS:
        t = _make(kind, FakeLib())
        t.wait()
        got[kind] = t.ticket
    assert got == {"search": 7, "sweep": 0, "best": 0}


@pytest.mark.parametrize("kind", KINDS)
def test_cancel_of_a_live_ticket_calls_npow_cancel(kind):
    lib = FakeLib(_lib.NPOW_PENDING)
    t = _make(kind, lib)
    t.cancel()
    assert lib.calls == [("npow_cancel", 7)]
    t.result = object()  # (collected: __del__ has nothing to do)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("timeout,us", [(None, -1), (0.5, 500000), (-3.0, 0), (0, 0)])
def test_the_timeout_in_microseconds(kind, timeout, us):
    lib = FakeLib(_lib.NPOW_PENDING)
    t = _make(kind, lib)
    assert t.wait(timeout) is None
    assert lib.calls[-1][0] == OWN_WAIT[kind][0] and lib.calls[-1][2] == us
    if kind == "search":
        assert t.wait_result(timeout) is None and lib.calls[-1] == ("npow_wait_result", 7, us)
        assert t.wait_info(timeout) is None and lib.calls[-1] == ("npow_wait_info", 7, us)
    if kind == "sweep":
        assert lib.calls[-1][3] == 16  # the ticket's cap
    t.result = object()


@pytest.mark.parametrize("call,args", [("promote", (2,)), ("retarget", (1 << 63,)), ("relax", (1 << 63,)),
                                       ("reserve_info", ())])
def test_a_library_without_the_call_is_a_bad_argument(call, args):
    name = {"promote": "npow_promote", "retarget": "npow_retarget", "relax": "npow_relax",
            "reserve_info": "npow_ticket_reserve"}[call]
    lib = FakeLib()
    t = _make("search", lib)
    with pytest.raises(_lib.NanoPowError) as e:
        getattr(t, call)(*args)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    assert e.value.message == f"the loaded libnanopow has no {name}"
    assert lib.calls == []
    t.result = object()


def test_a_library_without_npow_ticket_sweep_is_a_bad_argument():
    lib = FakeLib()
    t = _make("sweep", lib)
    with pytest.raises(_lib.NanoPowError) as e:
        t.info()
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
    assert e.value.message == "the loaded libnanopow has no npow_ticket_sweep"
    assert lib.calls == []
    t.result = object()


def test_the_messages_of_a_collected_ticket_and_a_bad_number():
    class Lib(FakeLib):
        def npow_promote(self, ticket, weight):
            return _lib.NPOW_OK

        npow_retarget = npow_promote

        def npow_relax(self, ticket, threshold, answered):
            return _lib.NPOW_OK

        def npow_ticket_reserve(self, ticket, info):
            return _lib.NPOW_OK

        def npow_ticket_sweep(self, ticket, info):
            return _lib.NPOW_OK

        def npow_ticket_best(self, ticket, info):
            return _lib.NPOW_OK

    def message(f, *a):
        with pytest.raises(_lib.NanoPowError) as e:
            f(*a)
        assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT
        return e.value.message

    t = _make("search", Lib())
    for wrong in (-1, 1 << 64, 1.5, True, "ff"):
        assert message(t.retarget, wrong) == "threshold must be an integer in [0, 2^64)"
        assert message(t.relax, wrong) == "threshold must be an integer in [0, 2^64)"
    for wrong in (-1, 1 << 32, 1.5, True, "2"):
        assert message(t.promote, wrong) == "weight must be 1, 2, 4 or 8"
    t.wait()
    for f, a in ((t.promote, (2,)), (t.retarget, (5,)), (t.relax, (5,)), (t.reserve_info, ())):
        assert message(f, *a) == "the ticket's result was already collected"
    with pytest.raises(RuntimeError, match="the ticket's result was already collected"):
        t.wait_info()
    s, b = _make("sweep", Lib()), _make("best", Lib())
    s.wait(), b.wait()
    assert message(s.info) == "the sweep ticket is collected"
    assert message(b.info) == "the best ticket is collected"


def test_public_attributes():
    t, s, b = (_make(k, FakeLib(), ticket=0) for k in ("search", "sweep", "best"))
    assert t.submitted_background is False and s.cap == 16
    for x in (t, s, b):
        assert x.ticket == 0 and x.cancel_token is None and x.result is None and x.engine.lib is not None
