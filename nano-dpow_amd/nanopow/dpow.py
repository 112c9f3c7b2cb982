"""DPoW client side of the path: MQTT work/cancel messages -> work server -> result messages.

The reference's DPoW client (client/dpow_client.py) subscribes to ``work/<type>`` and
``cancel/<type>`` and feeds a WorkHandler (client/work_handler.py), which serialises the
requests to the work server over HTTP and publishes ``result/<type>``.  This module is the
same flow with the broker replaced by whatever delivers messages (a queue in the harness,
an MQTT client in deployment), so time-to-work can be measured from the message that asks
for work to the message that answers it -- the latency the DPoW server sees
(server/scripts/check_latency.py:18-39 times ``work`` -> ``result`` on the broker).

Message formats (dpow_client.py:38-39, 63-85):
  work/<type>    payload "<hash>,<difficulty>"           (hash: 64 hex chars)
  cancel/<type>  payload "<hash>"
  result/<type>  payload "<hash>,<work>,<payout account>"

WorkHandler semantics kept (work_handler.py:9-125): a request already queued or ongoing
for the same hash is ignored; the next request is picked at random from the queue
(WorkQueue._get); a cancel removes a queued hash, or, for an ongoing one, forgets it (the
result is then not published) and POSTs ``work_cancel``.  ``concurrency`` > 1 runs that many
request loops against the work server (the reference runs one).

Extension: ``weights`` maps a work type to the ``"weight"`` (1, 2, 4 or 8) its work_generate
requests carry -- the work server then serves ``ondemand`` (a user is waiting) ahead of
``precache`` (speculative).  The field is sent only when it is not 1, so a reference work
server, which does not know it, is asked exactly as before with the default weights.

Promotion, part of that extension: the hub answers a service request for a hash whose precache
is pending by publishing ``work/ondemand`` for the same hash (server/dpow_server.py:287-328).
When the new message's type has a heavier configured weight than the one the hash was taken at,
and its difficulty is not above it, a queued hash is retyped to the heavier type and an ongoing
one is raised at the work server (``work_promote``, nanopow.server) -- its running search gets
the heavier share at once -- and its result is published under the heavier type.  With the
default weights (all 1) nothing is heavier: the message is ignored as in the reference.

Retargeting, opt-in (``retarget=True``): the hub asks for on-demand work above the precache
difficulty whenever a service sends a multiplier (server/dpow_server.py:273-328), and a precache
result below it would be rejected.  A message for a known hash at a HIGHER difficulty then
replaces a queued hash's difficulty, and for an ongoing hash is passed to the work server as
``work_retarget`` (nanopow.server: the running search goes on in place at the higher difficulty),
with a ``work_promote`` beside it when the type is heavier too.  The handler records the new
difficulty; a reply whose ``difficulty`` is below it means the raise came too late, and the hash
is queued again at the recorded difficulty instead of being published.  Without the option such
a message is ignored as before.

Relaxing, opt-in (``relax=True``), the other direction: a precache search runs at the send
difficulty and the block turns out to be a receive, 64 times easier.  A message for a known hash
at a LOWER difficulty then lowers a queued hash's difficulty, and for an ongoing hash is passed to
the work server as ``work_relax`` (nanopow.server: a search with a reserve is decided at once from
the best nonce it has passed, or goes on in place at the lower difficulty); the handler records
the new difficulty.  A heavier type promotes as above.  Without the option the difficulty stays.
"""
from __future__ import annotations

import asyncio
import json
import logging
import random
import time
import http.client
import threading
import urllib.parse
from typing import Awaitable, Callable, Dict, Optional, Tuple

log = logging.getLogger("nanopow.dpow")

WORK_TYPES = ("ondemand", "precache")
DEFAULT_WEIGHTS = {"ondemand": 1, "precache": 1}


class MessageError(ValueError):
    pass


def parse_work_message(topic: str, payload: bytes) -> Tuple[str, str, str]:
    """``work/<type>`` + ``b"hash,difficulty"`` -> (work_type, hash, difficulty) (dpow_client.py:63-75)."""
    work_type = topic.split("/")[-1]
    try:
        block_hash, difficulty = payload.decode("utf-8").split(",")
    except (UnicodeDecodeError, ValueError) as e:
        raise MessageError(f"Could not parse message {topic}: {e}") from e
    if len(block_hash) != 64:
        raise MessageError(f"Invalid hash {block_hash}")
    return work_type, block_hash, difficulty


def parse_cancel_message(payload: bytes) -> str:
    """``cancel/<type>`` payload -> hash (dpow_client.py:77-85)."""
    try:
        block_hash = payload.decode("utf-8")
    except UnicodeDecodeError as e:
        raise MessageError(f"Could not parse cancel message: {e}") from e
    if len(block_hash) != 64:
        raise MessageError(f"Invalid hash {block_hash}")
    return block_hash


def result_message(work_type: str, block_hash: str, work: str, payout: str) -> Tuple[str, bytes]:
    """(topic, payload) of a result (dpow_client.py:38-39)."""
    return f"result/{work_type}", f"{block_hash},{work},{payout}".encode("utf-8")


class HttpWorker:
    """POSTs JSON actions to a work server over keep-alive HTTP/1.1 connections, as the
    WorkHandler's aiohttp session does (work_handler.py:51, :75-78, :104-108): each executor thread
    keeps one connection and reuses it; a request that finds its connection closed by the server
    is sent once more on a fresh one."""

    def __init__(self, uri: str, timeout: float = 300.0) -> None:
        self.uri = uri if uri.startswith("http") else f"http://{uri}"
        u = urllib.parse.urlsplit(self.uri)
        self.host, self.port = u.hostname or "127.0.0.1", u.port or 80
        self.path = u.path or "/"
        self.timeout = timeout
        self._local = threading.local()

    def _conn(self, fresh: bool = False) -> http.client.HTTPConnection:
        c = getattr(self._local, "conn", None)
        if c is None or fresh:
            if c is not None:
                c.close()
            c = self._local.conn = http.client.HTTPConnection(self.host, self.port, timeout=self.timeout)
        return c

    def _post(self, obj: Dict) -> Dict:
        body = json.dumps(obj)
        for attempt in (0, 1):
            c = self._conn(fresh=attempt == 1)
            try:
                c.request("POST", self.path, body, {"Content-Type": "application/json"})
                return json.loads(c.getresponse().read())
            except (http.client.RemoteDisconnected, ConnectionResetError, BrokenPipeError,
                    http.client.CannotSendRequest):
                if attempt == 1:
                    raise
        raise AssertionError("unreachable")

    async def post(self, obj: Dict) -> Dict:
        return await asyncio.get_running_loop().run_in_executor(None, self._post, obj)


PublishFn = Callable[[str, bytes], Awaitable[None]]


class _Ongoing(dict):
    """The ongoing requests, hash -> [difficulty, work_type] (the type may be raised by a promotion), with
    the set-like discard() of the reference's ``work_ongoing`` (work_handler.py:39)."""

    def discard(self, block_hash: str) -> None:
        self.pop(block_hash, None)


def _difficulty_above(new: str, old: str) -> bool:
    try:
        return int(new, 16) > int(old, 16)
    except ValueError:
        return False


def _difficulty_not_above(new: str, old: str) -> bool:
    try:
        return int(new, 16) <= int(old, 16)
    except ValueError:
        return False


class DpowWorkHandler:
    """WorkHandler-equivalent: queue of requests -> work server -> published results."""

    def __init__(self, worker: HttpWorker, publish: PublishFn, payout: str, concurrency: int = 1,
                 rng: Optional[random.Random] = None, weights: Optional[Dict[str, int]] = None,
                 retarget: bool = False, background_types: Tuple[str, ...] = (), relax: bool = False) -> None:
        # background_types (opt-in, e.g. ("precache",)): requests of these work types are sent with
        # "background": true -- they hash only on what no other search wants -- and rank below every other type, so
        # the same hash again under any other type (work/ondemand) promotes the search, queued or ongoing
        self.background_types = frozenset(background_types)
        self.weights = dict(DEFAULT_WEIGHTS if weights is None else weights)
        for t, w in self.weights.items():
            if w not in (1, 2, 4, 8):
                raise ValueError(f"weight of work type {t!r} must be 1, 2, 4 or 8, not {w!r}")
        self.retarget = retarget
        self.relax = relax
        self.worker = worker
        self.publish = publish
        self.payout = payout
        self.concurrency = concurrency
        self.rng = rng or random.Random()
        self.queue: Dict[str, Tuple[str, str]] = {}   # hash -> (difficulty, work_type)
        self.ongoing: _Ongoing = _Ongoing()
        self._ready = asyncio.Event()
        self._tasks = []
        self.stats = {"queued": 0, "ignored": 0, "sent": 0, "cancelled": 0, "errors": 0, "promoted": 0,
                      "retargeted": 0, "requeued": 0, "relaxed": 0}

    async def start(self) -> None:
        # WorkHandler.start: the probe must answer with an "error" field (work_handler.py:53)
        res = await self.worker.post({"action": "invalid"})
        if "error" not in res:
            raise RuntimeError(f"Worker not available at {self.worker.uri}")
        self._tasks = [asyncio.ensure_future(self._loop()) for _ in range(self.concurrency)]

    async def stop(self) -> None:
        for t in self._tasks:
            t.cancel()
        for t in self._tasks:
            try:
                await t
            except (asyncio.CancelledError, Exception):
                pass

    # -- message entry points (dpow_client.py handle_work / handle_cancel) --------------------
    async def on_message(self, topic: str, payload: bytes) -> None:
        try:
            if "cancel" in topic:
                await self.queue_cancel(parse_cancel_message(payload))
            elif "work" in topic:
                work_type, block_hash, difficulty = parse_work_message(topic, payload)
                await self.queue_work(work_type, block_hash, difficulty)
        except MessageError as e:
            log.warning("%s", e)

    def _rank(self, work_type: str) -> int:
        """A work type's rank: its weight, background types below every weight."""
        return 0 if work_type in self.background_types else self.weights.get(work_type, 1)

    async def queue_work(self, work_type: str, block_hash: str, difficulty: str) -> None:
        if block_hash in self.queue or block_hash in self.ongoing:
            # the same hash again under a heavier type (module docstring): promote it; else ignored as in the reference
            queued = block_hash in self.queue
            old_difficulty, old_type = self.queue[block_hash] if queued else self.ongoing[block_hash]
            weight = self.weights.get(work_type, 1)
            if self.retarget and _difficulty_above(difficulty, old_difficulty):
                await self._retarget(block_hash, queued, work_type, difficulty)
                return
            if self.relax and _difficulty_above(old_difficulty, difficulty):
                await self._relax(block_hash, queued, difficulty)
                old_difficulty = difficulty
                if self._rank(work_type) <= self._rank(old_type):
                    return  # (a heavier type also promotes, below)
            if self._rank(work_type) <= self._rank(old_type) or not _difficulty_not_above(difficulty, old_difficulty):
                self.stats["ignored"] += 1
                return
            self.stats["promoted"] += 1
            if queued:
                self.queue[block_hash] = (old_difficulty, work_type)
                return
            self.ongoing[block_hash][1] = work_type  # its result is published under the heavier type
            try:
                await self.worker.post({"action": "work_promote", "hash": block_hash, "weight": weight})
            except Exception as e:  # noqa: BLE001 -- the search goes on at its old weight
                log.error("Work handler promote error: %s", e)
            return
        self.queue[block_hash] = (difficulty, work_type)
        self.stats["queued"] += 1
        self._ready.set()

    async def _retarget(self, block_hash: str, queued: bool, work_type: str, difficulty: str) -> None:
        """The same hash again at a higher difficulty (module docstring; ``retarget=True``)."""
        old_type = (self.queue[block_hash] if queued else self.ongoing[block_hash])[1]
        weight = self.weights.get(work_type, 1)
        heavier = self._rank(work_type) > self._rank(old_type)
        self.stats["retargeted"] += 1
        if heavier:
            self.stats["promoted"] += 1
        if queued:
            self.queue[block_hash] = (difficulty, work_type if heavier else old_type)
            return
        self.ongoing[block_hash][0] = difficulty  # a reply below it is not published (_loop)
        if heavier:
            self.ongoing[block_hash][1] = work_type
        try:
            await self.worker.post({"action": "work_retarget", "hash": block_hash, "difficulty": difficulty})
            if heavier:
                await self.worker.post({"action": "work_promote", "hash": block_hash, "weight": weight})
        except Exception as e:  # noqa: BLE001 -- a reply below the recorded difficulty is queued again
            log.error("Work handler retarget error: %s", e)

    async def _relax(self, block_hash: str, queued: bool, difficulty: str) -> None:
        """The same hash again at a lower difficulty (module docstring; ``relax=True``)."""
        self.stats["relaxed"] += 1
        if queued:
            self.queue[block_hash] = (difficulty, self.queue[block_hash][1])
            return
        self.ongoing[block_hash][0] = difficulty
        try:
            await self.worker.post({"action": "work_relax", "hash": block_hash, "difficulty": difficulty})
        except Exception as e:  # noqa: BLE001 -- the search goes on at its old difficulty: its result still serves
            log.error("Work handler relax error: %s", e)

    async def queue_cancel(self, block_hash: str) -> None:
        if self.queue.pop(block_hash, None) is not None:
            self.stats["cancelled"] += 1
            return
        if block_hash in self.ongoing:
            self.ongoing.discard(block_hash)  # loop() will not publish it
            self.stats["cancelled"] += 1
            try:
                await self.worker.post({"action": "work_cancel", "hash": block_hash})
            except Exception as e:  # noqa: BLE001 -- logged like work_handler.py:79-80
                log.error("Work handler queue_cancel error: %s", e)

    async def _next(self) -> Tuple[str, str, str]:
        while not self.queue:
            self._ready.clear()
            await self._ready.wait()
        block_hash = self.rng.choice(list(self.queue))  # WorkQueue._get: random entry
        difficulty, work_type = self.queue.pop(block_hash)
        return block_hash, difficulty, work_type

    async def _loop(self) -> None:
        while True:
            block_hash, difficulty, work_type = await self._next()
            self.ongoing[block_hash] = [difficulty, work_type]
            try:
                body = {"action": "work_generate", "hash": block_hash, "difficulty": difficulty}
                weight = self.weights.get(work_type, 1)
                if work_type in self.background_types:
                    body["background"] = True
                elif weight != 1:
                    body["weight"] = weight
                res = await self.worker.post(body)
            except Exception as e:  # noqa: BLE001
                log.error("Work handler loop error: %s", e)
                self.ongoing.discard(block_hash)
                self.stats["errors"] += 1
                continue
            if block_hash not in self.ongoing:  # cancelled meanwhile
                continue
            difficulty, work_type = self.ongoing.pop(block_hash)  # (a promotion or a retarget may have raised them)
            if "work" in res and self.retarget and _difficulty_above(difficulty, str(res.get("difficulty", difficulty))):
                # the raise came too late for that search: again, at the recorded difficulty
                self.queue[block_hash] = (difficulty, work_type)
                self.stats["requeued"] += 1
                self._ready.set()
            elif "work" in res:
                await self.publish(*result_message(work_type, block_hash, res["work"], self.payout))
                self.stats["sent"] += 1
            elif res.get("error"):
                log.error("Unexpected reply from work server: %s", res["error"])


class LatencyProbe:
    """check_latency.py's bookkeeping: time from a ``work`` message to its ``result``."""

    def __init__(self) -> None:
        self.t_work: Dict[str, float] = {}
        self.latency: Dict[str, float] = {}
        self.results: Dict[str, Tuple[str, str]] = {}

    def saw_work(self, block_hash: str) -> None:
        self.t_work.setdefault(block_hash, time.perf_counter())

    def saw_result(self, topic: str, payload: bytes) -> None:
        block_hash, work, account = payload.decode("utf-8").split(",")
        if block_hash in self.t_work:
            self.latency[block_hash] = time.perf_counter() - self.t_work[block_hash]
        self.results[block_hash] = (work, account)


async def replay(handler: DpowWorkHandler, probe: LatencyProbe, schedule, drain_timeout: float = 60.0) -> float:
    """Deliver ``schedule`` = [(t_offset_s, topic, payload), ...] to ``handler`` at those times
    (the broker's role), recording work messages in ``probe``; then wait until every uncancelled
    hash has a result (or ``drain_timeout``).  Returns the wall time."""
    t0 = time.perf_counter()
    cancelled = set()
    wanted = set()
    for t_off, topic, payload in sorted(schedule, key=lambda x: x[0]):
        dt = t0 + t_off - time.perf_counter()
        if dt > 0:
            await asyncio.sleep(dt)
        try:
            if "cancel" in topic:
                cancelled.add(parse_cancel_message(payload))
            elif "work" in topic:
                h = parse_work_message(topic, payload)[1]
                probe.saw_work(h)
                wanted.add(h)
        except MessageError:
            pass  # the handler logs and drops it
        await handler.on_message(topic, payload)
    deadline = time.perf_counter() + drain_timeout
    while time.perf_counter() < deadline:
        pending = [h for h in wanted if h not in probe.results and h not in cancelled]
        if not pending and not handler.queue and not handler.ongoing:
            break
        await asyncio.sleep(0.002)
    return time.perf_counter() - t0
