"""Reserve hits through the work server and the DPoW work handler.  With the reserve difficulty configured
(``WorkServer(reserve_threshold=...)``, or a request's ``"reserve"``) a search is submitted with the ``reserve``
keyword; a ``work_generate`` for the same hash at a lower difficulty is answered at once from a qualifying reserve
while the harder job runs on, ``work_relax`` lowers a queued job's field and relaxes one in the engine
(Ticket.relax), and the handler -- only with ``relax=True`` -- turns a work message for a known hash at a lower
difficulty into a new queued difficulty or one ``work_relax``.  Without the option everything is as before.
No GPU: the engine is tests/reserve_fake_engine.py."""
import asyncio
import random
import threading
import time

import pytest

from nanopow import dpow
from nanopow import work as W
from nanopow.__main__ import parse_args
from nanopow.server import WorkServer
from reserve_fake_engine import WIN_NONCE, OldTicket, ReserveEngine

SEND, RECEIVE, BETWEEN = "fffffff800000000", "fffffe0000000000", "ffffff0000000000"
MIN = "fffff00000000000"
A, B = "AA" * 32, "BB" * 32
RES_NONCE, RES_VALUE = 0xbeef, 0xffffff8000000000  # a reserve between RECEIVE (and BETWEEN) and SEND


class _Asker:
    """work_generate requests on threads of their own (each blocks until its search ends)."""

    def __init__(self, srv):
        self.srv, self.threads, self.replies = srv, [], []

    def ask(self, root_hex, difficulty=SEND, **extra):
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


@pytest.fixture
def serve():
    made = []

    def make(eng, **kw):
        srv = WorkServer(eng, max_active=kw.pop("max_active", 4), **kw).start()
        asker = _Asker(srv)
        made.append((eng, srv, asker))
        return srv, asker
    yield make
    for eng, srv, asker in made:
        eng.gate.set()
        asker.join()
        srv.stop()


def _reply(nonce, value, srv):
    return {"work": f"{nonce:016x}", "difficulty": f"{value:016x}",
            "multiplier": W.fmt_multiplier(W.to_multiplier(value, srv.base))}


# ---- configuration ---------------------------------------------------------------------------------------------------
def test_a_reserve_difficulty_below_the_minimum_is_refused_at_start_up():
    eng = ReserveEngine()
    with pytest.raises(ValueError):
        WorkServer(eng, reserve_threshold=int(MIN, 16) - 1)
    assert WorkServer(eng, reserve_threshold=int(MIN, 16)).reserve_threshold == int(MIN, 16)
    assert WorkServer(eng).reserve_threshold is None
    assert parse_args([]).reserve_difficulty is None
    assert parse_args(["--reserve-difficulty", RECEIVE]).reserve_difficulty == RECEIVE


def test_without_the_option_an_easier_duplicate_starts_its_own_search(serve):
    eng = ReserveEngine(scripted=(RES_NONCE, RES_VALUE))
    srv, asker = serve(eng)
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1)
    asker.ask(A, RECEIVE)
    _until(lambda: len(eng.tickets) == 2)
    assert eng.submits == [(bytes.fromhex(A), int(SEND, 16), {}), (bytes.fromhex(A), int(RECEIVE, 16), {})]
    assert all(t.peeks == 0 and t.relaxed == [] for t in eng.tickets)  # no reserve keyword, no peek
    eng.gate.set()
    asker.join()
    assert sorted(r["difficulty"] for r in asker.replies) == [RECEIVE, SEND]


def test_with_the_option_the_keyword_arrives_only_above_the_reserve_difficulty(serve):
    eng = ReserveEngine()
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    asker.ask(B, RECEIVE)  # at the reserve difficulty itself: a plain search
    _until(lambda: len(eng.tickets) == 2)
    assert sorted(eng.submits) == sorted([(bytes.fromhex(A), int(SEND, 16), {"reserve": int(RECEIVE, 16)}),
                                          (bytes.fromhex(B), int(RECEIVE, 16), {})])


def test_a_request_reserve_field_overrides_the_option(serve):
    eng = ReserveEngine()
    srv, asker = serve(eng)  # the option unset
    asker.ask(A, SEND, reserve=BETWEEN)
    _until(lambda: len(eng.tickets) == 1)
    assert eng.submits == [(bytes.fromhex(A), int(SEND, 16), {"reserve": int(BETWEEN, 16)})]
    for bad in ("ffff000000000000", "xyz", "", 5, "1" * 17):
        r = srv.handle({"action": "work_generate", "hash": B, "difficulty": SEND, "reserve": bad})
        assert r["error"] == "Bad reserve", r
    assert len(eng.tickets) == 1


def test_an_easier_duplicate_is_answered_from_a_qualifying_reserve_and_the_hard_job_runs_on(serve):
    eng = ReserveEngine(scripted=(RES_NONCE, RES_VALUE))
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and _jobs(srv, A) == [(int(SEND, 16), 1, True)])
    _until(lambda: eng.tickets[0] is srv._inflight[0].ticket)
    easy = srv.handle({"action": "work_generate", "hash": A, "difficulty": RECEIVE})  # returns at once
    assert easy == _reply(RES_NONCE, RES_VALUE, srv)
    assert srv.handle({"action": "work_generate", "hash": A, "difficulty": BETWEEN}) == easy
    assert len(eng.tickets) == 1 and eng.tickets[0].relaxed == []  # no second search, and never relaxed
    assert _jobs(srv, A) == [(int(SEND, 16), 1, True)]              # still in flight, one waiter
    assert asker.replies == []
    eng.gate.set()
    asker.join()
    assert asker.replies == [_reply(WIN_NONCE, int(SEND, 16), srv)]  # its first waiter: at its own difficulty


def test_a_reserve_below_the_requested_difficulty_is_not_used(serve):
    eng = ReserveEngine(scripted=(RES_NONCE, int(RECEIVE, 16) + 5))  # meets RECEIVE, not BETWEEN
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight and srv._inflight[0].ticket is not None)
    asker.ask(A, BETWEEN)  # no qualifying reserve: served as ever, by a search of its own
    _until(lambda: len(eng.tickets) == 2)
    assert eng.tickets[0].peeks == 1 and eng.tickets[0].relaxed == []
    assert eng.submits[1] == (bytes.fromhex(A), int(BETWEEN, 16), {"reserve": int(RECEIVE, 16)})
    eng.gate.set()
    asker.join()
    assert sorted(r["difficulty"] for r in asker.replies) == [BETWEEN, SEND]


def test_a_reserve_that_does_not_validate_is_not_used(serve):
    class Lying(ReserveEngine):
        def work_value(self, root, nonce):
            return 0x1000

    eng = Lying(scripted=(RES_NONCE, RES_VALUE))
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight and srv._inflight[0].ticket is not None)
    asker.ask(A, RECEIVE)
    _until(lambda: len(eng.tickets) == 2)


def test_a_duplicate_at_the_same_difficulty_still_shares_the_job(serve):
    eng = ReserveEngine(scripted=(RES_NONCE, RES_VALUE))
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1)
    asker.ask(A, SEND)
    _until(lambda: _jobs(srv, A) == [(int(SEND, 16), 2, True)])
    assert eng.tickets[0].peeks == 0


# ---- work_relax ------------------------------------------------------------------------------------------------------
def test_work_relax_lowers_a_queued_job_and_relaxes_an_inflight_one(serve):
    eng = ReserveEngine()
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16), max_active=1)
    asker.ask(A, SEND)  # runs (max_active 1); B queues
    _until(lambda: len(eng.tickets) == 1 and srv._inflight[0].ticket is not None)
    asker.ask(B, SEND)
    _until(lambda: int(srv.status()["queue_size"]) == 1)
    assert srv.handle({"action": "work_relax", "hash": B, "difficulty": BETWEEN}) == {}
    assert _jobs(srv, B) == [(int(BETWEEN, 16), 1, False)]
    assert eng.tickets[0].relaxed == []  # nothing in the engine was touched
    assert srv.handle({"action": "work_relax", "hash": A, "difficulty": BETWEEN}) == {}
    assert eng.tickets[0].relaxed == [int(BETWEEN, 16)]
    assert _jobs(srv, A) == [(int(BETWEEN, 16), 1, True)]
    assert srv.handle({"action": "work_relax", "hash": A, "difficulty": SEND}) == {}     # higher: no call
    assert srv.handle({"action": "work_relax", "hash": A, "difficulty": BETWEEN}) == {}  # equal: no call
    assert eng.tickets[0].relaxed == [int(BETWEEN, 16)]
    assert srv.handle({"action": "work_relax", "hash": "CC" * 32, "difficulty": RECEIVE}) == {}  # no job: empty
    eng.gate.set()
    asker.join()
    assert eng.submits[1] == (bytes.fromhex(B), int(BETWEEN, 16), {"reserve": int(RECEIVE, 16)})
    assert sorted(r["difficulty"] for r in asker.replies) == [BETWEEN, BETWEEN]


def test_work_relax_answered_from_the_reserve_replies_to_the_waiter_at_once(serve):
    eng = ReserveEngine(scripted=(RES_NONCE, RES_VALUE))
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight and srv._inflight[0].ticket is not None)
    assert srv.handle({"action": "work_relax", "hash": A, "multiplier": "0.015625"}) == {}  # 1/64: RECEIVE
    asker.join()  # the gate is still shut: the reply came from the reserve
    assert asker.replies == [_reply(RES_NONCE, RES_VALUE, srv)]
    assert eng.tickets[0].relaxed == [int(RECEIVE, 16)]


def test_work_relax_is_refused_below_the_jobs_reserve(serve):
    eng = ReserveEngine()
    srv, asker = serve(eng, reserve_threshold=int(BETWEEN, 16), max_active=1)
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight[0].ticket is not None)
    asker.ask(B, SEND)
    _until(lambda: int(srv.status()["queue_size"]) == 1)
    for h in (A, B):
        r = srv.handle({"action": "work_relax", "hash": h, "difficulty": RECEIVE})
        assert r["error"] == "Bad difficulty" and "reserve" in r["hint"], r
    assert eng.tickets[0].relaxed == []
    assert _jobs(srv, A) == [(int(SEND, 16), 1, True)] and _jobs(srv, B) == [(int(SEND, 16), 1, False)]


def test_work_relax_leaves_a_job_without_a_reserve_alone(serve):
    eng = ReserveEngine()
    srv, asker = serve(eng)  # the option unset: no job has a reserve
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight and srv._inflight[0].ticket is not None)
    assert srv.handle({"action": "work_relax", "hash": A, "difficulty": RECEIVE}) == {}
    assert eng.tickets[0].relaxed == [] and _jobs(srv, A) == [(int(SEND, 16), 1, True)]


def test_work_relax_too_late_keeps_the_jobs_difficulty(serve):
    eng = ReserveEngine(too_late=True)
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight and srv._inflight[0].ticket is not None)
    assert srv.handle({"action": "work_relax", "hash": A, "difficulty": RECEIVE}) == {}
    assert eng.tickets[0].relaxed == [int(RECEIVE, 16)]
    assert _jobs(srv, A) == [(int(SEND, 16), 1, True)]


def test_an_engine_without_reserves_keeps_serving(serve):
    eng = ReserveEngine(ticket_cls=OldTicket)
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    asker.ask(A, SEND)
    _until(lambda: len(eng.tickets) == 1 and srv._inflight and srv._inflight[0].ticket is not None)
    assert srv.handle({"action": "work_relax", "hash": A, "difficulty": RECEIVE}) == {}
    asker.ask(A, RECEIVE)  # no reserve() to peek at: a search of its own
    _until(lambda: len(eng.tickets) == 2)
    eng.gate.set()
    asker.join()
    assert sorted(r["difficulty"] for r in asker.replies) == [RECEIVE, SEND]


@pytest.mark.parametrize("req", [{"difficulty": SEND}, {"hash": "AB", "difficulty": SEND},
                                 {"hash": "G" * 64, "difficulty": SEND}, {"hash": 5, "difficulty": SEND},
                                 {"hash": A, "difficulty": "xyz"}, {"hash": A, "multiplier": "-1"}])
def test_work_relax_field_errors_are_work_generates(serve, req):
    eng = ReserveEngine()
    srv, asker = serve(eng, reserve_threshold=int(RECEIVE, 16))
    want = srv.handle({"action": "work_generate", **req})
    assert "error" in want
    assert srv.handle({"action": "work_relax", **req}) == want
    assert eng.submits == []


# ---- the DPoW work handler --------------------------------------------------------------------------------------------
class _StubWorker:
    uri = "stub"

    def __init__(self):
        self.bodies = []
        self.release = None  # an asyncio.Event, made inside the loop

    async def post(self, obj):
        self.bodies.append(dict(obj))
        if obj.get("action") == "work_generate":
            await self.release.wait()
            return {"work": "00000000000000ab", "difficulty": obj["difficulty"]}
        if obj.get("action") in ("work_promote", "work_cancel", "work_retarget", "work_relax"):
            return {}
        return {"error": "Unknown command"}


def _run_handler(script, **kw):
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


def _ongoing_then_lower(topic="work/precache", **kw):
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{SEND}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message(topic, f"{A},{RECEIVE}".encode())
        await h.on_message(topic, f"{A},{RECEIVE}".encode())  # and once more: nothing new
        assert A in h.ongoing and A not in h.queue
        script.recorded = list(h.ongoing[A])
        worker.release.set()
        await _settle(lambda: not h.ongoing and not h.queue)
        await asyncio.sleep(0.01)
    out = _run_handler(script, **kw)
    return out + (script.recorded,)


def test_default_handler_does_not_relax():
    bodies, published, stats, recorded = _ongoing_then_lower()
    assert [b["action"] for b in bodies] == ["invalid", "work_generate"]
    assert recorded == [SEND, "precache"]
    assert stats["relaxed"] == 0 and stats["ignored"] == 2
    assert published == [("result/precache", f"{A},00000000000000ab,nano_payout".encode())]


def test_relax_posts_one_work_relax_for_an_ongoing_hash_and_records_the_difficulty():
    bodies, published, stats, recorded = _ongoing_then_lower(relax=True)
    assert [b for b in bodies if b["action"] != "invalid"] == [
        {"action": "work_generate", "hash": A, "difficulty": SEND},
        {"action": "work_relax", "hash": A, "difficulty": RECEIVE}]
    assert recorded == [RECEIVE, "precache"]
    assert stats["relaxed"] == 1 and stats["ignored"] == 1 and stats["promoted"] == 0
    assert published == [("result/precache", f"{A},00000000000000ab,nano_payout".encode())]


def test_relax_with_a_heavier_type_also_promotes():
    bodies, published, stats, recorded = _ongoing_then_lower("work/ondemand", relax=True,
                                                             weights={"ondemand": 8, "precache": 1})
    assert [b for b in bodies if b["action"] != "invalid"] == [
        {"action": "work_generate", "hash": A, "difficulty": SEND},
        {"action": "work_relax", "hash": A, "difficulty": RECEIVE},
        {"action": "work_promote", "hash": A, "weight": 8}]
    assert recorded == [RECEIVE, "ondemand"]
    assert published == [("result/ondemand", f"{A},00000000000000ab,nano_payout".encode())]


def test_relax_lowers_a_queued_hash():
    async def script(h, worker):
        await h.on_message("work/precache", f"{B},{SEND}".encode())  # B becomes ongoing (concurrency 1) ...
        await _settle(lambda: B in h.ongoing)
        await h.on_message("work/precache", f"{A},{SEND}".encode())  # ... so A waits in the queue
        await h.on_message("work/precache", f"{A},{RECEIVE}".encode())
        assert h.queue[A] == (RECEIVE, "precache")
        worker.release.set()
        await _settle(lambda: not h.ongoing and not h.queue)
        await asyncio.sleep(0.01)
    bodies, published, stats = _run_handler(script, relax=True)
    assert all(b["action"] != "work_relax" for b in bodies)  # nothing at the work server to lower yet
    gen = {b["hash"]: b for b in bodies if b["action"] == "work_generate"}
    assert gen[A] == {"action": "work_generate", "hash": A, "difficulty": RECEIVE}
    assert stats["relaxed"] == 1
