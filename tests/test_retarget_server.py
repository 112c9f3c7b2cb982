"""Retargeting through the work server and the DPoW work handler: ``work_retarget`` raises the difficulty of a
queued job and of one already in the engine (Ticket.retarget), a later ``work_generate`` at that difficulty joins the
job, and the handler -- only with ``retarget=True`` -- turns a work message for a known hash at a higher difficulty
into a new queued difficulty or one ``work_retarget``, and queues a hash again whose reply came in below the
difficulty it recorded.  No GPU: the engine is tests/retarget_fake_engine.py."""
import asyncio
import random
import threading
import time

import pytest

from nanopow import dpow
from nanopow.server import WorkServer
from retarget_fake_engine import OldTicket, RetargetEngine

LOW, MID, HIGH = "ff00000000000000", "fff0000000000000", "fffffffe00000000"
A, B = "AA" * 32, "BB" * 32


class _Asker:
    """work_generate requests on threads of their own (each blocks until the gate opens)."""

    def __init__(self, srv):
        self.srv, self.threads, self.replies = srv, [], []

    def ask(self, root_hex, difficulty=LOW, **extra):
        def run():
            self.replies.append(self.srv.handle({"action": "work_generate", "hash": root_hex,
                                                 "difficulty": difficulty, **extra}))
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


def _jobs(srv, root_hex):
    with srv._lock:
        return [(j.threshold, j.waiters, j.active) for j in srv._inflight + srv._queue
                if j.root == bytes.fromhex(root_hex)]


def _serve(eng):
    srv = WorkServer(eng, max_active=1).start()
    return srv, _Asker(srv)


@pytest.fixture
def served():
    eng = RetargetEngine()
    srv, asker = _serve(eng)
    yield eng, srv, asker
    eng.gate.set()
    asker.join()
    srv.stop()


def test_work_retarget_raises_an_inflight_job_and_a_later_duplicate_joins_it(served):
    eng, srv, asker = served
    asker.ask(A)
    _until(lambda: len(eng.tickets) == 1)
    assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": HIGH}) == {}
    assert eng.tickets[0].retargeted == [int(HIGH, 16)]
    assert _jobs(srv, A) == [(int(HIGH, 16), 1, True)]
    assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": MID}) == {}   # lower: no call
    assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": HIGH}) == {}  # equal: no call
    assert eng.tickets[0].retargeted == [int(HIGH, 16)]
    asker.ask(A, HIGH)  # a duplicate at the new difficulty joins the job: no second search
    _until(lambda: _jobs(srv, A) == [(int(HIGH, 16), 2, True)])
    assert eng.submits == [(bytes.fromhex(A), int(LOW, 16))]
    eng.gate.set()
    asker.join()
    assert asker.replies == [{"work": "0000000000001234", "difficulty": HIGH,
                              "multiplier": asker.replies[0]["multiplier"]}] * 2


def test_work_retarget_raises_a_queued_job(served):
    eng, srv, asker = served
    asker.ask(A)  # runs (max_active 1); B queues
    _until(lambda: len(eng.tickets) == 1)
    asker.ask(B)
    _until(lambda: int(srv.status()["queue_size"]) == 1)
    assert srv.handle({"action": "work_retarget", "hash": B, "difficulty": MID}) == {}
    assert _jobs(srv, B) == [(int(MID, 16), 1, False)]
    assert all(t.retargeted == [] for t in eng.tickets)  # nothing in the engine was touched
    asker.ask(B, MID)  # joins it
    _until(lambda: _jobs(srv, B) == [(int(MID, 16), 2, False)])
    eng.gate.set()
    asker.join()
    assert eng.submits == [(bytes.fromhex(A), int(LOW, 16)), (bytes.fromhex(B), int(MID, 16))]
    assert sorted(r["difficulty"] for r in asker.replies) == [LOW, MID, MID]


def test_work_retarget_takes_a_multiplier_like_work_generate(served):
    eng, srv, asker = served
    asker.ask(A, LOW)
    _until(lambda: len(eng.tickets) == 1)
    assert srv.handle({"action": "work_retarget", "hash": A, "multiplier": "8.0"}) == {}
    want = srv.handle({"action": "work_validate", "hash": A, "work": "0", "multiplier": "8.0"})
    assert "valid" in want
    (thr, _, _), = _jobs(srv, A)
    assert eng.tickets[0].retargeted == [thr] and thr > int(LOW, 16)


def test_work_retarget_answers_empty_when_no_job_matches(served):
    eng, srv, asker = served
    assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": HIGH}) == {}
    asker.ask(A)
    _until(lambda: len(eng.tickets) == 1)
    assert srv.handle({"action": "work_retarget", "hash": B, "difficulty": HIGH}) == {}
    assert srv.handle({"action": "work_cancel", "hash": B}) == {}
    assert eng.tickets[0].retargeted == [] and len(eng.tickets) == 1


@pytest.mark.parametrize("req", [{}, {"hash": "AB"}, {"hash": "G" * 64}, {"hash": 5}])
def test_work_retarget_hash_errors_are_work_generates(served, req):
    eng, srv, asker = served
    want = srv.handle({"action": "work_generate", "difficulty": LOW, **req})
    assert "error" in want
    assert srv.handle({"action": "work_retarget", "difficulty": LOW, **req}) == want
    assert eng.submits == []


@pytest.mark.parametrize("extra", [{"difficulty": "xyz"}, {"difficulty": ""}, {"difficulty": 5},
                                   {"difficulty": "1" * 17}, {"multiplier": "-1"}, {"multiplier": "x"}])
def test_work_retarget_difficulty_errors_are_work_generates(served, extra):
    eng, srv, asker = served
    want = srv.handle({"action": "work_generate", "hash": A, **extra})
    assert "error" in want, want
    assert srv.handle({"action": "work_retarget", "hash": A, **extra}) == want
    assert eng.submits == []


def test_work_generate_still_matches_by_hash_and_difficulty():
    eng = RetargetEngine()
    srv = WorkServer(eng, max_active=2).start()
    asker = _Asker(srv)
    try:
        asker.ask(A, LOW)
        _until(lambda: len(eng.tickets) == 1)
        asker.ask(A, HIGH)  # no work_retarget: a second search, as before
        _until(lambda: len(eng.tickets) == 2)
        assert all(t.retargeted == [] for t in eng.tickets)
        assert eng.submits == [(bytes.fromhex(A), int(LOW, 16)), (bytes.fromhex(A), int(HIGH, 16))]
    finally:
        eng.gate.set()
        asker.join()
        srv.stop()


def test_too_late_leaves_the_jobs_difficulty():
    eng = RetargetEngine(too_late=True)
    srv, asker = _serve(eng)
    try:
        asker.ask(A)
        _until(lambda: len(eng.tickets) == 1)
        assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": HIGH}) == {}
        assert eng.tickets[0].retargeted == [int(HIGH, 16)]
        assert _jobs(srv, A) == [(int(LOW, 16), 1, True)]
        eng.gate.set()
        asker.join()
    finally:
        eng.gate.set()
        srv.stop()
    assert asker.replies[0]["difficulty"] == LOW


def test_engine_without_retarget_keeps_serving():
    eng = RetargetEngine(OldTicket)
    srv, asker = _serve(eng)
    try:
        asker.ask(A)
        _until(lambda: len(eng.tickets) == 1)
        assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": HIGH}) == {}
        assert _jobs(srv, A) == [(int(LOW, 16), 1, True)]
        eng.gate.set()
        asker.join()
    finally:
        eng.gate.set()
        srv.stop()
    assert asker.replies[0].get("work") == "0000000000001234"


def test_a_failing_retarget_does_not_fail_the_request():
    from nanopow import _lib
    from retarget_fake_engine import RetargetTicket

    class Raising(RetargetTicket):
        def retarget(self, threshold):
            raise _lib.NanoPowError(_lib.NPOW_ERR_BAD_ARGUMENT, "unknown ticket")

    eng = RetargetEngine(Raising)
    srv, asker = _serve(eng)
    try:
        asker.ask(A)
        _until(lambda: len(eng.tickets) == 1)
        assert srv.handle({"action": "work_retarget", "hash": A, "difficulty": HIGH}) == {}
        eng.gate.set()
        asker.join()
    finally:
        eng.gate.set()
        srv.stop()
    assert asker.replies[0].get("work") == "0000000000001234"


# ---- the DPoW work handler against a stub worker -----------------------------------------------------------------
DIFF, HIGHER = "fffffff800000000", "fffffffe00000000"
WEIGHTS = {"ondemand": 8, "precache": 1}


class _StubWorker:
    """work_generate answers only once released, at the difficulty it was asked for (a work server whose search was
    decided before any raise), so a hash stays ongoing while further messages arrive."""
    uri = "stub"

    def __init__(self):
        self.bodies = []
        self.release = None  # an asyncio.Event, made inside the loop

    async def post(self, obj):
        self.bodies.append(dict(obj))
        if obj.get("action") == "work_generate":
            await self.release.wait()
            return {"work": "00000000000000ab", "difficulty": obj["difficulty"]}
        if obj.get("action") in ("work_promote", "work_cancel", "work_retarget"):
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


def _ongoing_then(second_topic, second_difficulty, **kw):
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message(second_topic, f"{A},{second_difficulty}".encode())
        await h.on_message(second_topic, f"{A},{second_difficulty}".encode())  # and once more: nothing new
        assert A in h.ongoing and A not in h.queue
        worker.release.set()
        await _settle(lambda: not h.ongoing and not h.queue)
        await asyncio.sleep(0.01)
    return _run_handler(script, **kw)


def test_default_handler_still_ignores_a_higher_difficulty():
    bodies, published, stats = _ongoing_then("work/ondemand", HIGHER, weights=WEIGHTS)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate"]
    assert published == [("result/precache", f"{A},00000000000000ab,nano_payout".encode())]
    assert stats["ignored"] == 2 and stats["retargeted"] == 0 and stats["promoted"] == 0 and stats["requeued"] == 0


def test_ongoing_hash_at_a_higher_difficulty_sends_one_work_retarget_too_late_requeues():
    """The stub's pending work_generate answers at the difficulty it was asked for -- below the raised one, as a
    search decided before the raise would -- so the hash is queued again at the recorded difficulty, and that
    second reply is published."""
    bodies, published, stats = _ongoing_then("work/precache", HIGHER, retarget=True)
    assert [b for b in bodies if b["action"] != "invalid"] == [
        {"action": "work_generate", "hash": A, "difficulty": DIFF},
        {"action": "work_retarget", "hash": A, "difficulty": HIGHER},
        {"action": "work_generate", "hash": A, "difficulty": HIGHER}]
    assert published == [("result/precache", f"{A},00000000000000ab,nano_payout".encode())]
    assert stats["retargeted"] == 1 and stats["requeued"] == 1 and stats["sent"] == 1
    assert stats["ignored"] == 1 and stats["promoted"] == 0


def test_ongoing_hash_retargeted_in_time_is_published_once():
    class InTime(_StubWorker):
        """A work server that retargets: the pending work_generate answers at the raised difficulty."""
        async def post(self, obj):
            res = await super().post(obj)
            if obj.get("action") == "work_generate":
                raised = [b["difficulty"] for b in self.bodies if b["action"] == "work_retarget"]
                res["difficulty"] = max([obj["difficulty"]] + raised, key=lambda d: int(d, 16))
            return res

    worker, published, out = InTime(), [], {}

    async def main():
        worker.release = asyncio.Event()

        async def publish(topic, payload):
            published.append((topic, payload))

        h = dpow.DpowWorkHandler(worker, publish, "nano_payout", rng=random.Random(3), weights=WEIGHTS, retarget=True)
        await h.start()
        try:
            await h.on_message("work/precache", f"{A},{DIFF}".encode())
            await _settle(lambda: A in h.ongoing)
            await h.on_message("work/ondemand", f"{A},{HIGHER}".encode())  # higher and heavier
            assert h.ongoing[A] == [HIGHER, "ondemand"]
            worker.release.set()
            await _settle(lambda: not h.ongoing and not h.queue)
            await asyncio.sleep(0.01)
        finally:
            worker.release.set()
            await h.stop()
        out["stats"] = dict(h.stats)
    asyncio.run(main())
    assert [b for b in worker.bodies if b["action"] != "invalid"] == [
        {"action": "work_generate", "hash": A, "difficulty": DIFF},
        {"action": "work_retarget", "hash": A, "difficulty": HIGHER},
        {"action": "work_promote", "hash": A, "weight": 8}]
    assert published == [("result/ondemand", f"{A},00000000000000ab,nano_payout".encode())]
    st = out["stats"]
    assert st["retargeted"] == 1 and st["promoted"] == 1 and st["requeued"] == 0 and st["sent"] == 1


def test_queued_hash_takes_the_higher_difficulty():
    async def script(h, worker):
        await h.on_message("work/precache", f"{B},{DIFF}".encode())  # B becomes ongoing (concurrency 1) ...
        await _settle(lambda: B in h.ongoing)
        await h.on_message("work/precache", f"{A},{DIFF}".encode())  # ... so A waits in the queue
        assert h.queue[A] == (DIFF, "precache")
        await h.on_message("work/precache", f"{A},{HIGHER}".encode())
        assert h.queue[A] == (HIGHER, "precache")
        await h.on_message("work/precache", f"{A},{DIFF}".encode())  # lower again: ignored
        assert h.queue[A] == (HIGHER, "precache")
        worker.release.set()
        await _settle(lambda: not h.ongoing and not h.queue)
        await asyncio.sleep(0.01)
    bodies, published, stats = _run_handler(script, retarget=True)
    assert all(b["action"] != "work_retarget" for b in bodies)  # nothing at the work server to raise yet
    gen = {b["hash"]: b for b in bodies if b["action"] == "work_generate"}
    assert gen[A] == {"action": "work_generate", "hash": A, "difficulty": HIGHER}
    assert stats["retargeted"] == 1 and stats["ignored"] == 1 and stats["sent"] == 2 and stats["requeued"] == 0


def test_cancel_of_a_retargeted_hash_still_forgets_it():
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message("work/precache", f"{A},{HIGHER}".encode())
        await h.on_message("cancel/precache", A.encode())
        assert A not in h.ongoing
        worker.release.set()
        await asyncio.sleep(0.02)
    bodies, published, stats = _run_handler(script, retarget=True)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate", "work_retarget", "work_cancel"]
    assert published == [] and stats["cancelled"] == 1 and stats["retargeted"] == 1 and stats["requeued"] == 0
