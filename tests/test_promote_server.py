"""Promotion through the work server and the DPoW work handler: a heavier duplicate or a ``work_promote`` raises a
job that is already in the engine (Ticket.promote), a queued one is re-ordered, and the handler turns a
``work/ondemand`` message for a hash whose precache search is ongoing into one ``work_promote``.  No GPU: the
engine here is a fake whose tickets record their promote calls."""
import asyncio
import random
import threading
import time

import pytest

from nanopow import _lib, dpow
from nanopow import work as W
from nanopow.server import WorkServer

LOW = "ff00000000000000"
A, B, C = "AA" * 32, "BB" * 32, "CC" * 32


class _Ticket:
    def __init__(self, eng, root, threshold):
        self.eng, self.root, self.threshold = eng, root, threshold
        self.promoted = []

    def wait(self, timeout=None):
        if not self.eng.gate.wait(timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, 0x1234, self.threshold, 1)

    def promote(self, weight):
        self.promoted.append(weight)


class _OldTicket:
    """A ticket of an engine without promotion."""

    def __init__(self, eng, root, threshold):
        self.eng, self.root, self.threshold = eng, root, threshold

    def wait(self, timeout=None):
        if not self.eng.gate.wait(timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, 0x1234, self.threshold, 1)


class PromoteEngine:
    def __init__(self, ticket_cls=_Ticket):
        self.gate = threading.Event()
        self.ticket_cls = ticket_cls
        self.calls = []    # (root, weight keyword or None)
        self.tickets = []

    def submit(self, root, threshold, start=0, device_mask=0, max_nonces_per_device=0, cancel=None, **kw):
        assert set(kw) <= {"weight"}, kw
        self.calls.append((root, kw.get("weight")))
        t = self.ticket_cls(self, root, threshold)
        self.tickets.append(t)
        return t

    def work_value(self, root, nonce):
        return 0


class _Asker:
    """work_generate requests on threads of their own (each blocks until the gate opens)."""

    def __init__(self, srv):
        self.srv, self.threads, self.replies = srv, [], []

    def ask(self, root_hex, **extra):
        def run():
            self.replies.append(self.srv.handle({"action": "work_generate", "hash": root_hex, "difficulty": LOW,
                                                 **extra}))
        t = threading.Thread(target=run)
        t.start()
        self.threads.append(t)

    def join(self):
        for t in self.threads:
            t.join(10)
            assert not t.is_alive()


def _until(cond):
    deadline = time.time() + 10
    while not cond():
        assert time.time() < deadline
        time.sleep(0.001)


def _waiters(srv, root_hex):
    with srv._lock:
        return sum(j.waiters for j in srv._inflight + srv._queue if j.root == bytes.fromhex(root_hex))


@pytest.fixture
def served():
    eng = PromoteEngine()
    srv = WorkServer(eng, max_active=1).start()
    asker = _Asker(srv)
    yield eng, srv, asker
    eng.gate.set()
    asker.join()
    srv.stop()


def test_heavier_duplicate_promotes_an_inflight_job_once(served):
    eng, srv, asker = served
    asker.ask(A)
    _until(lambda: len(eng.tickets) == 1)
    asker.ask(A, weight=8)
    _until(lambda: _waiters(srv, A) == 2)
    assert eng.tickets[0].promoted == [8]
    asker.ask(A, weight=8)  # the same weight again: nothing more to raise
    asker.ask(A, weight=4)  # lighter than it is by now
    asker.ask(A)
    _until(lambda: _waiters(srv, A) == 5)
    assert eng.tickets[0].promoted == [8]
    assert eng.calls == [(bytes.fromhex(A), None)]
    with srv._lock:
        assert srv._inflight[0].weight == 8
    eng.gate.set()
    asker.join()
    assert len(asker.replies) == 5 and all(r.get("work") == "0000000000001234" for r in asker.replies)


def test_lighter_or_equal_duplicate_does_not_promote(served):
    eng, srv, asker = served
    asker.ask(A, weight=4)
    _until(lambda: len(eng.tickets) == 1)
    asker.ask(A, weight=4)
    asker.ask(A, weight=2)
    asker.ask(A)
    _until(lambda: _waiters(srv, A) == 4)
    assert eng.tickets[0].promoted == [] and eng.calls == [(bytes.fromhex(A), 4)]
    with srv._lock:
        assert srv._inflight[0].weight == 4


def test_queued_job_is_reordered_by_a_heavier_duplicate_and_by_work_promote(served):
    eng, srv, asker = served
    asker.ask(A)  # runs (max_active 1); B, C and D queue in this order
    _until(lambda: len(eng.tickets) == 1)
    D = "DD" * 32
    for i, r in enumerate((B, C, D)):
        asker.ask(r)
        _until(lambda: int(srv.status()["queue_size"]) == i + 1)
    asker.ask(D, weight=2)  # a duplicate raises D in the queue
    _until(lambda: _waiters(srv, D) == 2)
    assert srv.handle({"action": "work_promote", "hash": C, "weight": 8}) == {}  # ... and the action C, above it
    assert all(t.promoted == [] for t in eng.tickets)  # nothing in the engine was touched
    eng.gate.set()
    asker.join()
    b = bytes.fromhex
    assert eng.calls == [(b(A), None), (b(C), 8), (b(D), 2), (b(B), None)]


def test_work_promote_raises_an_inflight_job_and_answers_like_work_cancel(served):
    eng, srv, asker = served
    asker.ask(A)
    _until(lambda: len(eng.tickets) == 1)
    assert srv.handle({"action": "work_promote", "hash": A, "weight": "4"}) == {}
    assert eng.tickets[0].promoted == [4]
    assert srv.handle({"action": "work_promote", "hash": A, "weight": 2}) == {}  # lighter: no call
    assert srv.handle({"action": "work_promote", "hash": A, "weight": 4}) == {}  # equal: no call
    assert srv.handle({"action": "work_promote", "hash": A}) == {}               # weight 1 when absent: no call
    assert eng.tickets[0].promoted == [4]
    assert srv.handle({"action": "work_promote", "hash": A, "weight": 8}) == {}
    assert eng.tickets[0].promoted == [4, 8]
    assert srv.handle({"action": "work_promote", "hash": B, "weight": 8}) == {}  # no such job: {} all the same
    assert srv.handle({"action": "work_cancel", "hash": B}) == {}
    assert eng.tickets[0].promoted == [4, 8] and len(eng.tickets) == 1


@pytest.mark.parametrize("weight", [3, "x", 0, 16, -1, 2.0, True, [8]])
def test_work_promote_weight_errors_are_work_generates(served, weight):
    eng, srv, asker = served
    want = srv.handle({"action": "work_generate", "hash": A, "difficulty": LOW, "weight": weight})
    assert want == {"error": "Bad weight", "hint": "Expecting 1, 2, 4 or 8"}
    assert srv.handle({"action": "work_promote", "hash": A, "weight": weight}) == want
    assert eng.calls == []


@pytest.mark.parametrize("req", [{}, {"hash": "AB"}, {"hash": "G" * 64}, {"hash": 5}])
def test_work_promote_hash_errors_are_work_generates(served, req):
    eng, srv, asker = served
    want = srv.handle({"action": "work_generate", "difficulty": LOW, **req})
    assert "error" in want
    assert srv.handle({"action": "work_promote", "weight": 8, **req}) == want
    assert eng.calls == []


def test_engine_without_promote_keeps_serving():
    eng = PromoteEngine(_OldTicket)
    srv = WorkServer(eng, max_active=1).start()
    asker = _Asker(srv)
    try:
        asker.ask(A)
        _until(lambda: len(eng.tickets) == 1)
        asker.ask(A, weight=8)
        _until(lambda: _waiters(srv, A) == 2)
        assert srv.handle({"action": "work_promote", "hash": A, "weight": 8}) == {}
        with srv._lock:
            assert srv._inflight[0].weight == 8
        eng.gate.set()
        asker.join()
    finally:
        eng.gate.set()
        srv.stop()
    assert len(asker.replies) == 2 and all(r.get("work") == "0000000000001234" for r in asker.replies)


def test_a_failing_promote_does_not_fail_the_request():
    class Raising(_Ticket):
        def promote(self, weight):
            raise _lib.NanoPowError(_lib.NPOW_ERR_BAD_ARGUMENT, "unknown ticket")

    eng = PromoteEngine(Raising)
    srv = WorkServer(eng, max_active=1).start()
    asker = _Asker(srv)
    try:
        asker.ask(A)
        _until(lambda: len(eng.tickets) == 1)
        assert srv.handle({"action": "work_promote", "hash": A, "weight": 8}) == {}
        eng.gate.set()
        asker.join()
    finally:
        eng.gate.set()
        srv.stop()
    assert asker.replies[0].get("work") == "0000000000001234"


def test_unknown_action_hint_is_unchanged(served):
    eng, srv, asker = served
    assert srv.handle({"action": "invalid"}) == {
        "error": "Unknown command",
        "hint": "Supported commands: work_generate, work_cancel, work_validate, benchmark, status"}
    assert W.SUPPORTED == "Supported commands: work_generate, work_cancel, work_validate, benchmark, status"


# ---- the DPoW work handler against a stub worker -----------------------------------------------------------------
class _StubWorker:
    """work_generate answers only once released, so a hash stays ongoing while further messages arrive."""
    uri = "stub"

    def __init__(self):
        self.bodies = []
        self.release = None  # an asyncio.Event, made inside the loop

    async def post(self, obj):
        self.bodies.append(dict(obj))
        if obj.get("action") == "work_generate":
            await self.release.wait()
            return {"work": "00000000000000ab"}
        if obj.get("action") in ("work_promote", "work_cancel"):
            return {}
        return {"error": "Unknown command"}


def _run_handler(script, **kw):
    """script(handler, worker) is awaited between start and stop; returns (worker bodies, published, stats)."""
    worker = _StubWorker()
    published = []
    out = {}

    async def main():
        worker.release = asyncio.Event()

        async def publish(topic, payload):
            published.append((topic, payload))

        h = dpow.DpowWorkHandler(worker, publish, "nano_payout", rng=random.Random(3), **kw)
        await h.start()
        try:
            await script(h, worker)
        finally:
            worker.release.set()
            await h.stop()
        out["stats"] = dict(h.stats)
    asyncio.run(main())
    return worker.bodies, published, out["stats"]


async def _settle(cond):
    for _ in range(5000):
        if cond():
            return
        await asyncio.sleep(0.001)
    raise AssertionError("timed out")


DIFF = "fffffff800000000"
WEIGHTS = {"ondemand": 8, "precache": 1}


def _ongoing_then(second_topic, second_difficulty, **kw):
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message(second_topic, f"{A},{second_difficulty}".encode())
        await h.on_message(second_topic, f"{A},{second_difficulty}".encode())  # and once more: nothing new
        assert A in h.ongoing and A not in h.queue
        worker.release.set()
        await _settle(lambda: not h.ongoing)
        await asyncio.sleep(0.01)
    return _run_handler(script, **kw)


def test_ondemand_for_an_ongoing_precache_sends_one_work_promote():
    bodies, published, stats = _ongoing_then("work/ondemand", DIFF, weights=WEIGHTS)
    assert [b for b in bodies if b["action"] == "work_promote"] == [
        {"action": "work_promote", "hash": A, "weight": 8}]
    assert [b for b in bodies if b["action"] == "work_generate"] == [
        {"action": "work_generate", "hash": A, "difficulty": DIFF}]
    assert published == [("result/ondemand", f"{A},00000000000000ab,nano_payout".encode())]
    assert stats["promoted"] == 1 and stats["ignored"] == 1 and stats["sent"] == 1


def test_ondemand_with_default_weights_is_ignored_as_in_the_reference():
    bodies, published, stats = _ongoing_then("work/ondemand", DIFF)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate"]
    assert published == [("result/precache", f"{A},00000000000000ab,nano_payout".encode())]
    assert stats["promoted"] == 0 and stats["ignored"] == 2


def test_a_lower_difficulty_still_promotes_and_a_higher_one_is_ignored():
    bodies, published, stats = _ongoing_then("work/ondemand", "fffffe0000000000", weights=WEIGHTS)
    assert sum(b["action"] == "work_promote" for b in bodies) == 1 and stats["promoted"] == 1
    bodies, published, stats = _ongoing_then("work/ondemand", "fffffffc00000000", weights=WEIGHTS)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate"]
    assert published == [("result/precache", f"{A},00000000000000ab,nano_payout".encode())]
    assert stats["promoted"] == 0 and stats["ignored"] == 2
    bodies, published, stats = _ongoing_then("work/ondemand", "not-hex", weights=WEIGHTS)
    assert stats["promoted"] == 0 and stats["ignored"] == 2


def test_a_lighter_type_for_an_ongoing_hash_is_ignored():
    async def script(h, worker):
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        worker.release.set()
        await _settle(lambda: not h.ongoing)
    bodies, published, stats = _run_handler(script, weights=WEIGHTS)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate"] and bodies[1]["weight"] == 8
    assert published[0][0] == "result/ondemand" and stats["ignored"] == 1 and stats["promoted"] == 0


def test_a_queued_hash_is_retyped():
    async def script(h, worker):
        await h.on_message("work/precache", f"{B},{DIFF}".encode())  # B becomes ongoing (concurrency 1) ...
        await _settle(lambda: B in h.ongoing)
        await h.on_message("work/precache", f"{A},{DIFF}".encode())  # ... so A waits in the queue
        assert h.queue[A] == (DIFF, "precache")
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())
        assert h.queue[A] == (DIFF, "ondemand")
        await h.on_message("work/ondemand", f"{A},fffffffc00000000".encode())  # higher difficulty: ignored
        assert h.queue[A] == (DIFF, "ondemand")
        worker.release.set()
        await _settle(lambda: not h.ongoing and not h.queue)
        await asyncio.sleep(0.01)
    bodies, published, stats = _run_handler(script, weights=WEIGHTS)
    assert all(b["action"] != "work_promote" for b in bodies)  # nothing at the work server to raise yet
    gen = {b["hash"]: b for b in bodies if b["action"] == "work_generate"}
    assert gen[A] == {"action": "work_generate", "hash": A, "difficulty": DIFF, "weight": 8}
    assert "weight" not in gen[B]
    assert sorted(t for t, _ in published) == ["result/ondemand", "result/precache"]
    assert stats["promoted"] == 1 and stats["ignored"] == 1 and stats["sent"] == 2


def test_cancel_of_a_promoted_hash_still_forgets_it():
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())
        await h.on_message("cancel/ondemand", A.encode())
        assert A not in h.ongoing
        worker.release.set()
        await asyncio.sleep(0.02)
    bodies, published, stats = _run_handler(script, weights=WEIGHTS)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate", "work_promote", "work_cancel"]
    assert published == [] and stats["cancelled"] == 1 and stats["promoted"] == 1
