"""nano-work-server-compatible JSON work server on top of libnanopow.

Drop-in for the work server the DPoW client talks to
(client/README.md:31 ``nano-work-server --gpu 0:0 -l 127.0.0.1:7000``;
client/config_parse.py:18 default ``--worker_uri 127.0.0.1:7000``).  The
client's WorkHandler (client/work_handler.py) is the contract:

* ``start()`` POSTs ``{"action": "invalid"}`` with a 2 s timeout and reads
  ``['error']`` (work_handler.py:53) -> unknown actions answer
  ``{"error": "Unknown command", "hint": "Supported commands: ..."}``.
* ``loop()`` POSTs one ``work_generate {hash, difficulty}`` at a time and
  publishes ``res['work']`` (work_handler.py:104-117) -> the reply is
  ``{"work": "%016x", "difficulty": "%016x", "multiplier": "..."}``
  (nano-work-server.exe @1673856 field names).
* ``queue_cancel()`` POSTs ``work_cancel {hash}`` on a second connection while
  the generate is pending (work_handler.py:71-78) -> the pending generate
  returns ``{"error": "Cancelled"}`` and the cancel itself gets ``{}``.

Also served: ``work_validate`` (valid / valid_all / valid_receive / difficulty /
multiplier, @1680400..1680528), ``status`` (generating / queue_size,
@1679680) and ``benchmark`` (count -> duration / average / hint, @1679992..1680344).

Requests queue FIFO (``--shuffle``: random pick, nano-work-server.exe @1681064);
a request's optional ``"weight"`` (1, 2, 4 or 8 -- this server's extension, the
reference has no such field) puts it ahead of lighter ones in that queue and gives
it that share of each GPU among the searches in flight (npow_submit_weighted).
A duplicate request with a heavier weight raises the job it joins, also when its
search is already running (npow_promote: the share changes inside the running
launch), and ``{"action": "work_promote", "hash": ..., "weight": ...}`` -- this
server's extension too, answered ``{}`` like ``work_cancel`` whether or not a job
matched -- raises every queued or running job of that hash.  Weights only rise.
``{"action": "work_retarget", "hash": ..., "difficulty": ...}`` (or ``"multiplier"``, as in
``work_generate``; this server's extension, answered ``{}`` likewise) raises the
difficulty of every queued or running job of that hash that is below it: a running
search goes on in place at the higher difficulty (npow_retarget) instead of being
cancelled and started again, and a later ``work_generate`` at that difficulty joins
it.  Difficulties only rise; ``work_generate`` itself still matches a job by hash and
difficulty and never retargets one.
A ``work_generate`` with ``"background": true`` (this server's extension; a JSON
boolean) is a background search: it queues behind every foreground request and its
search hashes only on the GPU workgroups no foreground search wants
(npow_submit_background) -- speculative work that costs the other requests nothing.
A later foreground ``work_generate`` for the same hash and difficulty, or a
``work_promote`` for the hash, lifts it to a foreground search of that weight, also
while it runs.  ``status`` reports how many searches in flight are background.
With ``--reserve-difficulty HEX`` (``WorkServer(reserve_threshold=...)``; off by default, and a request's
``"reserve": "<hex>"`` -- this server's extension -- sets it for that request) every
``work_generate`` above that difficulty is searched with it as its reserve threshold
(npow_submit_reserve): the search remembers the best nonce it passes that meets the reserve
difficulty.  A ``work_generate`` for the same hash at a lower difficulty is then answered at
once from that reserve when it qualifies, while the harder search runs on for the waiters that
asked for more (the server never lowers a shared search by itself), and
``{"action": "work_relax", "hash": ..., "difficulty": ...}`` (or ``"multiplier"``; answered
``{}`` like ``work_retarget``) lowers every queued or running search of the hash that is above
it, in place (npow_relax: decided at once from its reserve when that qualifies).
``{"action": "work_best", "hash": ..., "count": N}`` (this server's extension; optional
``"start"``, 16 hex digits, and ``"difficulty"``, a floor) hashes exactly N nonces (at most
2^40) and answers with the strongest: ``{"work", "difficulty", "multiplier", "hashes"}``
(npow_submit_best), ``{"error": "Exhausted"}`` when nothing reached the floor, and
``{"error": "Cancelled"}`` after a ``work_cancel`` of the hash.  With ``"background": true``
(a JSON boolean, as ``work_generate``'s) it is a background best job
(npow_submit_best_background): the GPUs hash it only while no foreground request wants
them, so a long one can run beside ``work_generate`` traffic -- and makes no progress
while that traffic is continuous.  With ``"shared": true`` it is a shared best job
(npow_submit_best_shared): it takes a weight-1 share of each GPU beside the searches and the
workgroups they no longer want, so it finishes under continuous traffic, and a search that
arrives waits about 0.3 ms for it, not a launch.  Both flags together are refused
(``{"error": "Bad shared", ...}``).  The reply is the same.
The reference serves one request at a time; here up to ``max_active`` queued
requests are handed to libnanopow's work pool at once (npow_submit), where
every selected GPU searches all of them in the same kernel launches, so a
burst of requests from many clients keeps the GPUs busy across request
boundaries.  ``max_active=1`` is the reference's strictly serial service.
Each connection's thread hands its own request to the engine and blocks there
for the result (no dispatcher or per-request threads).
Every reply a search produces was re-validated on the CPU inside libnanopow
before it reaches this layer.
"""
from __future__ import annotations

import json
import logging
import os
import queue
import random
import socket
import socketserver
import threading
import time
from typing import Any, Dict, List, Optional, Protocol

from . import work as W
from ._lib import (NPOW_CANCELLED, NPOW_EXHAUSTED, NPOW_OK, NPOW_RESERVE_MIN, CancelToken, NanoPowError,
                   SearchResult)

log = logging.getLogger("nanopow.server")

GENERATION_FAILED = {"error": "Work generation failed (see logs for details)"}


class SearchTicket(Protocol):
    def wait(self, timeout: Optional[float] = None) -> Optional[SearchResult]: ...


class SearchEngine(Protocol):
    """What the server needs from an engine (libnanopow's :class:`nanopow.Engine`)."""

    def submit(self, root: bytes, threshold: int, start: int = 0, device_mask: int = 0,
               max_nonces_per_device: int = 0, cancel: Optional[CancelToken] = None) -> SearchTicket: ...
    # (an engine that serves weighted requests also takes `weight: int = 1`; passed only when it is not 1 -- and one
    # that serves background requests `background: bool = False`; passed only when it is set -- and one that keeps
    # reserves `reserve: Optional[int] = None`; passed only for a request with a reserve difficulty)

    def work_value(self, root: bytes, nonce: int) -> int: ...


class Job:
    __slots__ = ("root", "threshold", "cancel", "done", "reply", "active", "t_queued", "waiters", "t_started",
                 "ticket", "dispatched", "collector", "weight", "background", "reserve")

    def __init__(self, root: bytes, threshold: int, weight: int = 1, background: bool = False,
                 reserve: Optional[int] = None) -> None:
        self.root = root
        self.threshold = threshold
        self.reserve = reserve  # its reserve threshold (below `threshold` when queued), None: a search without one
        self.weight = 1 if background else weight
        self.background = background  # until a foreground duplicate or a work_promote lifts it
        self.cancel = CancelToken()
        self.done = threading.Event()
        self.reply: Dict[str, Any] = {}
        self.active = False
        self.t_queued = time.perf_counter()
        self.t_started = 0.0
        self.waiters = 1
        self.ticket: Optional[SearchTicket] = None
        self.dispatched = threading.Event()  # ticket set, or the job already resolved
        self.collector = False               # a request thread is collecting the ticket's result

    def resolve(self, reply: Dict[str, Any]) -> None:
        if not self.done.is_set():
            self.reply = reply
            self.done.set()
        self.dispatched.set()


class WorkServer:
    """Request dispatcher: a FIFO (or shuffled) queue in front of the engine's work pool.

    No thread of its own: a request is handed to the engine (npow_submit) by the request thread
    that queued it when fewer than max_active are in flight, otherwise by the request thread whose
    search ends next; each request thread then blocks in the engine (npow_wait, GIL released)
    for its own result.  A request costs no thread hand-off on the way in or out."""

    def __init__(self, engine: SearchEngine, base_threshold: int = W.DEFAULT_BASE, shuffle: bool = False,
                 device_mask: int = 0, rng: Optional[random.Random] = None, max_active: int = 4,
                 reserve_threshold: Optional[int] = None) -> None:
        if max_active < 1:
            raise ValueError("max_active must be >= 1")
        if reserve_threshold is not None and not NPOW_RESERVE_MIN <= reserve_threshold <= W.M64:
            raise ValueError(f"reserve_threshold must be at least {NPOW_RESERVE_MIN:016x}")
        self.reserve_threshold = reserve_threshold
        self.engine = engine
        self.base = base_threshold
        self.shuffle = shuffle
        self.device_mask = device_mask
        self.max_active = max_active
        self.rng = rng or random.Random(int.from_bytes(os.urandom(8), "little"))
        self._lock = threading.Condition()
        self._queue: List[Job] = []
        self._inflight: List[Job] = []
        self._best: List[Any] = []  # work_best requests in the engine: (root, cancel token)
        self._running = False
        # tickets answered at their decision (npow_wait_result) and collected after the reply
        self._reap_q: "queue.SimpleQueue" = queue.SimpleQueue()
        self._reaper: Optional[threading.Thread] = None

    # -- lifecycle ---------------------------------------------------------------------
    def start(self) -> "WorkServer":
        with self._lock:
            self._running = True
        return self

    def stop(self) -> None:
        with self._lock:
            self._running = False
            pending = list(self._queue)
            self._queue.clear()
            for j in self._inflight:
                j.cancel.set()
            for _, c in self._best:
                c.set()
            self._lock.notify_all()
        for j in pending:
            j.resolve({"error": "Cancelled"})
        deadline = time.time() + 10
        with self._lock:
            while self._inflight and time.time() < deadline:
                self._lock.wait(0.1)
            reaper, self._reaper = self._reaper, None
        if reaper is not None:
            self._reap_q.put(None)
            reaper.join(10)

    def _reap(self, ticket) -> None:
        """Collect a ticket whose reply has gone out (its other devices may still be stopping): one
        thread, started on first use, waits for each in turn (npow_wait)."""
        with self._lock:
            if self._reaper is None:
                self._reaper = threading.Thread(target=self._reap_loop, name="nanopow-reaper", daemon=True)
                self._reaper.start()
        self._reap_q.put(ticket)

    def _reap_loop(self) -> None:
        while True:
            t = self._reap_q.get()
            if t is None:
                return
            try:
                t.wait()
            except Exception as e:  # the reply is out; only log
                log.error("collecting a finished search: %s", e)

    # -- dispatch ----------------------------------------------------------------------
    def handle_body(self, raw: bytes) -> Dict[str, Any]:
        try:
            req = json.loads(raw.decode("utf-8")) if raw else None
        except (UnicodeDecodeError, json.JSONDecodeError):
            req = None
        if req is None:
            return {"error": "Failed to deserialize JSON"}
        return self.handle(req)

    def handle(self, req: Any) -> Dict[str, Any]:
        if not isinstance(req, dict):
            return {"error": "Failed to deserialize JSON"}
        action = req.get("action")
        try:
            if action == "work_generate":
                return self.work_generate(req)
            if action == "work_cancel":
                return self.work_cancel(req)
            if action == "work_promote":
                return self.work_promote(req)
            if action == "work_retarget":
                return self.work_retarget(req)
            if action == "work_relax":
                return self.work_relax(req)
            if action == "work_validate":
                return self.work_validate(req)
            if action == "work_best" and hasattr(self.engine, "submit_best"):
                return self.work_best(req)
            if action == "status":
                return self.status()
            if action == "benchmark":
                return self.benchmark(req)
            return {"error": "Unknown command", "hint": W.SUPPORTED}
        except W.RequestError as e:
            return e.reply()

    def work_generate(self, req: Dict[str, Any]) -> Dict[str, Any]:
        root = W.parse_hash(req)
        threshold = W.requested_threshold(req, self.base)
        weight = W.parse_weight(req)
        background = W.parse_background(req)
        reserve = W.parse_reserve(req, NPOW_RESERVE_MIN)
        if reserve is None:
            reserve = self.reserve_threshold
        if reserve is not None and reserve >= threshold:  # (at or below the reserve difficulty: a plain search)
            reserve = None
        return self._result(self._enqueue(root, threshold, weight, background, reserve))

    def work_cancel(self, req: Dict[str, Any]) -> Dict[str, Any]:
        root = W.parse_hash(req)
        cancelled: List[Job] = []
        with self._lock:
            keep = []
            for j in self._queue:
                (cancelled if j.root == root else keep).append(j)
            self._queue[:] = keep
            for j in self._inflight:
                if j.root == root:
                    j.cancel.set()
            for r, c in self._best:
                if r == root:
                    c.set()
        for j in cancelled:
            j.resolve({"error": "Cancelled"})
        log.info("Cancel %s", root.hex().upper())
        return {}

    def work_promote(self, req: Dict[str, Any]) -> Dict[str, Any]:
        """Raise every queued or in-flight job of the hash to the weight (this server's extension)."""
        root = W.parse_hash(req)
        weight = W.parse_weight(req)
        with self._lock:
            raised = [j for j in self._inflight + self._queue
                      if j.root == root and not j.cancel.is_set and self._raise_locked(j, weight)]
        for j in raised:
            self._promote(j, weight)
        log.info("Promote %s to weight %d (%d jobs)", root.hex().upper(), weight, len(raised))
        return {}

    def _raise_locked(self, job: Job, weight: int) -> bool:
        """Raise the job's weight; True when its search is in the engine and must be promoted there (_promote,
        once the lock is released).  A job still waiting here is submitted with the weight, and so is one whose
        submit is under way: _submit compares the weight again once the ticket exists."""
        if job.background:  # lifted: a foreground job of this weight, whatever the weight
            job.background = False
        elif weight <= job.weight:
            return False
        job.weight = max(job.weight, weight)
        return job.active and job.ticket is not None

    def _promote(self, job: Job, weight: int) -> None:
        t = job.ticket
        if t is None or not hasattr(t, "promote"):  # an engine without promotion keeps serving
            return
        try:
            t.promote(weight)
        except Exception as e:  # (its search ended and was collected meanwhile: nothing to raise)
            log.debug("promote %s: %s", job.root.hex().upper(), e)

    def work_retarget(self, req: Dict[str, Any]) -> Dict[str, Any]:
        """Raise every queued or in-flight job of the hash that is below the difficulty to it (this server's
        extension).  A job still waiting here, or one whose submit is under way (_submit compares again once the
        ticket exists), only changes its field; one in the engine is retargeted there (_retarget, once the lock is
        released) and its field follows when the raise held."""
        root = W.parse_hash(req)
        threshold = W.requested_threshold(req, self.base)
        in_engine = []
        with self._lock:
            for j in self._inflight + self._queue:
                if j.root != root or j.cancel.is_set or j.threshold >= threshold:
                    continue
                if j.active and j.ticket is not None:
                    in_engine.append(j)
                else:
                    j.threshold = threshold
        for j in in_engine:
            self._retarget(j, threshold)
        log.info("Retarget %s to difficulty %016x", root.hex().upper(), threshold)
        return {}

    def _retarget(self, job: Job, threshold: int) -> None:
        t = job.ticket
        if t is None or not hasattr(t, "retarget"):  # an engine without retargeting keeps serving
            return
        try:
            held = t.retarget(threshold)
        except Exception as e:  # (its search ended and was collected meanwhile: nothing to raise)
            log.debug("retarget %s: %s", job.root.hex().upper(), e)
            return
        if held:  # (False: decided already -- its reply, at the old difficulty, is on its way)
            with self._lock:
                job.threshold = max(job.threshold, threshold)

    def work_relax(self, req: Dict[str, Any]) -> Dict[str, Any]:
        """Lower every queued or in-flight job of the hash that has a reserve and is above the difficulty to it (this
        server's extension; work_retarget's mirror).  A job still waiting here, or one whose submit is under way
        (_submit compares again once the ticket exists), only changes its field; one in the engine is relaxed there
        (_relax, once the lock is released: decided at once from its reserve when that qualifies) and its field
        follows.  Refused, with nothing changed, when the difficulty is below the reserve of such a job."""
        root = W.parse_hash(req)
        threshold = W.requested_threshold(req, self.base)
        in_engine = []
        with self._lock:
            jobs = [j for j in self._inflight + self._queue
                    if j.root == root and not j.cancel.is_set and j.reserve is not None and j.threshold > threshold]
            if any(threshold < j.reserve for j in jobs):
                raise W.RequestError("Bad difficulty", "Below the reserve difficulty of a search for this hash")
            for j in jobs:
                if j.active and j.ticket is not None:
                    in_engine.append(j)
                else:
                    j.threshold = threshold
        for j in in_engine:
            self._relax(j, threshold)
        log.info("Relax %s to difficulty %016x", root.hex().upper(), threshold)
        return {}

    def _relax(self, job: Job, threshold: int) -> None:
        t = job.ticket
        if t is None or not hasattr(t, "relax"):  # an engine without reserves keeps serving
            return
        try:
            answered = t.relax(threshold)
        except Exception as e:  # (its search ended and was collected meanwhile: nothing to lower)
            log.debug("relax %s: %s", job.root.hex().upper(), e)
            return
        if answered is not None:  # (None: decided already -- its reply, at the old difficulty, is on its way)
            with self._lock:
                job.threshold = min(job.threshold, threshold)

    def _from_reserve(self, job: Job, threshold: int) -> Optional[Dict[str, Any]]:
        """The reply to a request at `threshold` from the reserve of the harder in-flight job, or None: a look at
        the job's reserve (Ticket.reserve: no GPU wait), re-validated as every reply is.  The job runs on."""
        t = job.ticket
        if t is None or not hasattr(t, "reserve"):
            return None
        try:
            res = t.reserve()
            if res is None or res.nonce is None:
                return None
            value = self.engine.work_value(job.root, res.nonce)
        except Exception as e:  # (collected meanwhile, or an engine error: serve the request as ever)
            log.debug("reserve of %s: %s", job.root.hex().upper(), e)
            return None
        if value < threshold:
            return None
        log.info("Answered %s from a reserve for difficulty %016x", job.root.hex().upper(), threshold)
        return {"work": W.fmt_u64(res.nonce), "difficulty": W.fmt_u64(value),
                "multiplier": W.fmt_multiplier(W.to_multiplier(value, self.base))}

    def work_best(self, req: Dict[str, Any]) -> Dict[str, Any]:
        """The strongest work among exactly `count` nonces of the hash (this server's extension; the engine's best
        job, npow_submit_best): best-effort work at a cost fixed in advance.  ``"start"`` (16 hex digits; random
        when absent) is the range's first nonce and ``"difficulty"`` a floor below which nothing is returned
        (``{"error": "Exhausted"}``).  The job queues in the engine like a bounded search; it is not shared with
        other requests, and a work_cancel of the hash cancels it.  ``"background": true`` (a JSON boolean) makes it a
        background best job (npow_submit_best_background): hashed only while no foreground job wants the GPUs;
        ``"shared": true`` a shared one (npow_submit_best_shared): a weight-1 share of each GPU beside the searches,
        never held out.  Both together are refused.  Either keyword is passed to the engine only when it is set, as
        work_generate's is."""
        root = W.parse_hash(req)
        count = W.parse_best_count(req)
        start = W.parse_start(req)
        background = W.parse_background(req)
        shared = W.parse_shared(req)
        floor = W.parse_threshold(req["difficulty"]) if req.get("difficulty") is not None else 0
        if start is None:
            start = self.rng.getrandbits(64)
        cancel = CancelToken()
        entry = (root, cancel)
        with self._lock:
            if not self._running:
                return dict(GENERATION_FAILED)
            self._best.append(entry)
        try:
            t0 = time.perf_counter()
            extra = {"background": True} if background else {"shared": True} if shared else {}
            ticket = self.engine.submit_best(root, start, count, floor=floor, device_mask=self.device_mask,
                                             cancel=cancel, **extra)
            status, nonce, value, done = ticket.wait()
            if status == NPOW_CANCELLED:
                return {"error": "Cancelled"}
            if status == NPOW_EXHAUSTED:
                return {"error": "Exhausted"}
            if status != NPOW_OK or self.engine.work_value(root, nonce) != value:
                return dict(GENERATION_FAILED)
            log.info("Best of %d nonces for %s in %.0fms: difficulty %016x", count, root.hex().upper(),
                     (time.perf_counter() - t0) * 1000.0, value)
            return {"work": W.fmt_u64(nonce), "difficulty": W.fmt_u64(value),
                    "multiplier": W.fmt_multiplier(W.to_multiplier(value, self.base)), "hashes": str(done)}
        except Exception as e:  # never leave a client waiting
            log.error("Error computing work: %s", e)
            return dict(GENERATION_FAILED)
        finally:
            with self._lock:
                self._best.remove(entry)

    def work_validate(self, req: Dict[str, Any]) -> Dict[str, Any]:
        root = W.parse_hash(req)
        nonce = W.parse_work(req)
        value = self.engine.work_value(root, nonce)
        out: Dict[str, Any] = {}
        if req.get("difficulty") is not None or req.get("multiplier") is not None:
            thr = W.requested_threshold(req, self.base)
            out["valid"] = "1" if value >= thr else "0"
        out["valid_all"] = "1" if value >= W.SEND_THRESHOLD else "0"
        out["valid_receive"] = "1" if value >= W.RECEIVE_THRESHOLD else "0"
        out["difficulty"] = W.fmt_u64(value)
        out["multiplier"] = W.fmt_multiplier(W.to_multiplier(value, self.base))
        return out

    def status(self) -> Dict[str, Any]:
        with self._lock:
            out = {"generating": "1" if self._inflight else "0", "queue_size": str(len(self._queue))}
            n_bg = sum(1 for j in self._inflight if j.background)
            if n_bg:  # (this server's extension: how many of the searches in flight are background; absent at 0)
                out["background"] = str(n_bg)
            return out

    def benchmark(self, req: Dict[str, Any]) -> Dict[str, Any]:
        count = W.parse_count(req)
        threshold = W.requested_threshold(req, self.base)
        log.info("Benchmarking %d samples at difficulty %016x (x%s)", count, threshold,
                 W.fmt_multiplier(W.to_multiplier(threshold, self.base)))
        t0 = time.perf_counter()
        for _ in range(count):
            reply = self._result(self._enqueue(self.rng.getrandbits(256).to_bytes(32, "little"), threshold))
            if "work" not in reply:
                return {"error": "Benchmark failed", "hint": "Work generation failure"}
        ms = (time.perf_counter() - t0) * 1000.0
        return {"count": str(count), "difficulty": W.fmt_u64(threshold),
                "multiplier": W.fmt_multiplier(W.to_multiplier(threshold, self.base)),
                "duration": str(int(round(ms))), "average": str(int(round(ms / count))),
                "hint": "Times in milliseconds"}

    # -- queue -------------------------------------------------------------------------
    def _enqueue(self, root: bytes, threshold: int, weight: int = 1, background: bool = False,
                 reserve: Optional[int] = None) -> Job:
        # An easier duplicate: the hash has a harder job in the engine that keeps a reserve.  A qualifying reserve
        # answers this request at once; the harder job is left as it is -- its waiters asked for more and must not
        # be handed less, so a shared job is never relaxed here.  No qualifying reserve: served as ever, below.
        harder: List[Job] = []
        with self._lock:
            same = [j for j in self._inflight + self._queue if j.root == root and not j.cancel.is_set]
            # (a job at this very difficulty is shared, as ever)
            if self._running and not any(j.threshold == threshold for j in same):
                harder = [j for j in same if j.reserve is not None and j.threshold > threshold
                          and j.ticket is not None and not j.done.is_set()]
        for h in harder:
            reply = self._from_reserve(h, threshold)
            if reply is not None:
                j = Job(root, threshold)
                j.resolve(reply)
                return j
        with self._lock:
            if not self._running:
                j = Job(root, threshold)
                j.resolve(dict(GENERATION_FAILED))
                return j
            # the same root at the same threshold queued or running: share its result
            for j in self._inflight + self._queue:
                if j.root == root and j.threshold == threshold and not j.cancel.is_set:
                    j.waiters += 1
                    # a heavier duplicate raises a job that still waits here (its place in the queue and the
                    # weight it is submitted with), and promotes one already in the engine (npow_promote)
                    # (a foreground duplicate lifts a background job; a background duplicate only shares the result)
                    dup, promote = j, (not background and self._raise_locked(j, weight))
                    break
            else:
                dup, promote = None, False
                job = Job(root, threshold, weight, background, reserve)
                self._queue.append(job)
                ready = self._pump_locked()
        if dup is not None:
            if promote:
                self._promote(dup, weight)
            return dup
        self._submit(ready)
        return job

    def _pump_locked(self) -> List[Job]:
        """Move queued jobs in flight while fewer than max_active are (the heaviest first; within a
        weight FIFO, or a random one with --shuffle); the caller submits them once the lock is released.
        Background jobs go behind every foreground one, and only while fewer than max_active jobs are in flight in
        all; a foreground job goes while fewer than max_active foreground ones are, so it never waits behind
        background jobs (the engine admits by the same rule)."""
        ready = []
        rank = lambda j: 0 if j.background else j.weight  # noqa: E731
        while self._running and self._queue:
            top = max(rank(j) for j in self._queue)
            busy = len(self._inflight) if top == 0 else sum(1 for j in self._inflight if not j.background)
            if busy >= self.max_active:
                break
            heaviest = [i for i, j in enumerate(self._queue) if rank(j) == top]
            idx = self.rng.choice(heaviest) if self.shuffle else heaviest[0]
            job = self._queue.pop(idx)
            job.active = True
            job.t_started = time.perf_counter()
            self._inflight.append(job)
            ready.append(job)
        return ready

    def _submit(self, jobs: List[Job]) -> None:
        for job in jobs:
            try:
                # (the keyword only for a weighted request: engines without it keep serving the others)
                sent, sent_threshold, sent_bg = job.weight, job.threshold, job.background
                extra = {"weight": sent} if sent != 1 else {}
                if sent_bg:  # (likewise only when asked for)
                    extra["background"] = True
                if job.reserve is not None and job.reserve < sent_threshold:  # (likewise)
                    extra["reserve"] = job.reserve
                ticket = self.engine.submit(job.root, sent_threshold, start=self.rng.getrandbits(64),
                                            device_mask=self.device_mask, cancel=job.cancel, **extra)
                with self._lock:  # (a heavier duplicate, a work_retarget or a work_relax may have come while the submit was under way)
                    job.ticket = ticket
                    now, now_threshold, now_bg = job.weight, job.threshold, job.background
                if now > sent or (sent_bg and not now_bg):
                    self._promote(job, now)
                if now_threshold > sent_threshold:
                    self._retarget(job, now_threshold)
                elif now_threshold < sent_threshold:  # (a work_relax came meanwhile)
                    self._relax(job, now_threshold)
            except Exception as e:  # never leave a client waiting
                log.error("Error computing work: %s", e)
                self._complete(job, dict(GENERATION_FAILED))
                continue
            job.dispatched.set()

    def _result(self, job: Job) -> Dict[str, Any]:
        """Block until the job's reply exists; the first request thread to get here after the
        job is in flight collects it from the engine, any other (a duplicate request) waits."""
        job.dispatched.wait()
        with self._lock:
            mine = not job.done.is_set() and job.ticket is not None and not job.collector
            if mine:
                job.collector = True
        if mine:
            self._complete(job, self._collect(job))
        job.done.wait()
        return dict(job.reply)

    def _collect(self, job: Job) -> Dict[str, Any]:
        try:
            t = job.ticket
            early = hasattr(t, "wait_result")
            # the reply as soon as the outcome is known (the reference answers when its result validates,
            # nano-work-server.exe @1669040), before a split search's other devices have stopped; the
            # ticket is collected after the reply (_reap)
            try:
                res = t.wait_result() if early else t.wait()
            finally:
                if early:  # collected even when the outcome is an error (else the engine keeps the job)
                    self._reap(t)
            if res is not None and res.status == NPOW_OK:
                log.info("Generated for %s in %.0fms for difficulty %016x", job.root.hex().upper(),
                         (time.perf_counter() - job.t_started) * 1000.0, job.threshold)
                return {"work": W.fmt_u64(res.nonce), "difficulty": W.fmt_u64(res.value),
                        "multiplier": W.fmt_multiplier(W.to_multiplier(res.value, self.base))}
            if res is not None and res.status == NPOW_CANCELLED:
                return {"error": "Cancelled"}
            return dict(GENERATION_FAILED)
        except NanoPowError as e:
            log.error("Error computing work: %s", e)
        except Exception as e:  # never leave a client waiting
            log.exception("work loop failure: %s", e)
        return dict(GENERATION_FAILED)

    def _complete(self, job: Job, reply: Dict[str, Any]) -> None:
        job.resolve(reply)
        with self._lock:
            if job in self._inflight:
                self._inflight.remove(job)
            ready = self._pump_locked()
            self._lock.notify_all()
        self._submit(ready)


# ---------------------------------------------------------------------------------------
_REASON = {200: "OK", 400: "Bad Request", 405: "Method Not Allowed", 413: "Payload Too Large"}
_MAX_LINE = 65536
_MAX_BODY = 1 << 20


class _Connection(socketserver.StreamRequestHandler):
    """One HTTP/1.1 client connection (keep-alive; the DPoW client's aiohttp session reuses it for
    every work_generate, client/work_handler.py:98-108): request line, headers, a JSON body ->
    one JSON reply written with ONE send (status line, headers and body together; TCP_NODELAY).
    A minimal parser: no email.parser header objects, no per-request allocation beyond the body."""
    disable_nagle_algorithm = True
    work_server: WorkServer  # set on the subclass

    def handle(self) -> None:
        rfile = self.rfile
        while True:
            line = rfile.readline(_MAX_LINE + 1)
            if not line:
                return
            if line in (b"\r\n", b"\n"):
                continue  # stray blank lines between requests (RFC 9112 2.2)
            parts = line.split()
            if len(parts) != 3 or not parts[2].startswith(b"HTTP/1."):
                self._send(400, {"error": "Bad request line"}, True)
                return
            method, version = parts[0], parts[2]
            close = version == b"HTTP/1.0"
            length, chunked = 0, False
            while True:
                h = rfile.readline(_MAX_LINE + 1)
                if h in (b"\r\n", b"\n", b""):
                    break
                name, _, value = h.partition(b":")
                name = name.strip().lower()
                if name == b"content-length":
                    try:
                        length = int(value.strip())
                    except ValueError:
                        length = -1
                elif name == b"connection":
                    v = value.strip().lower()
                    close = v == b"close" or (version == b"HTTP/1.0" and v != b"keep-alive")
                elif name == b"transfer-encoding":
                    chunked = b"chunked" in value.lower()
                elif name == b"expect" and value.strip().lower() == b"100-continue":
                    self.wfile.write(b"HTTP/1.1 100 Continue\r\n\r\n")
            if length < 0 or length > _MAX_BODY:
                self._send(413 if length > 0 else 400, {"error": "Bad Content-Length"}, True)
                return
            body = self._read_chunked() if chunked else (rfile.read(length) if length else b"")
            if body is None:
                self._send(400, {"error": "Bad chunked body"}, True)
                return
            if method == b"POST":
                self._send(200, self.work_server.handle_body(body), close)
            else:
                self._send(405, {"error": "Can only POST requests"}, close)
            if close:
                return

    def _read_chunked(self) -> Optional[bytes]:
        out = []
        total = 0
        while True:
            size_line = self.rfile.readline(_MAX_LINE + 1)
            try:
                n = int(size_line.split(b";")[0].strip(), 16)
            except ValueError:
                return None
            if n == 0:
                while self.rfile.readline(_MAX_LINE + 1) not in (b"\r\n", b"\n", b""):
                    pass  # trailers
                return b"".join(out)
            total += n
            if total > _MAX_BODY:
                return None
            out.append(self.rfile.read(n))
            self.rfile.readline(_MAX_LINE + 1)  # the chunk's CRLF

    def _send(self, code: int, obj: Dict[str, Any], close: bool) -> None:
        data = json.dumps(obj).encode()
        head = (f"HTTP/1.1 {code} {_REASON.get(code, 'OK')}\r\nContent-Type: application/json\r\n"
                f"Content-Length: {len(data)}\r\n{'Connection: close' + chr(13) + chr(10) if close else ''}\r\n")
        try:
            self.wfile.write(head.encode() + data)
        except OSError:
            pass  # the client went away; its request was answered as far as the server is concerned


class _Listener(socketserver.TCPServer):
    """Accepts connections and hands each to a connection thread (one per open connection: a DPoW
    client's keep-alive session holds its thread).  Threads that finish a connection wait for the
    next one (up to _MAX_IDLE of them) instead of exiting: a request on a new connection then costs
    a queue hand-off, not a thread start (round 5: ~0.3 ms per request on the MI355X box's host with
    a thread per connection, profiles/r05as_http_new_connection.json)."""
    # socketserver's default listen backlog is 5: a burst of concurrent work_generate
    # connections (many clients, or one client's precache wave) would overflow it and wait
    # out TCP's 1-s SYN retry, or be reset.  4,096 connections at once (BASELINE configs[3])
    # overflowed 1,024 with resets; the kernel caps this at net.core.somaxconn.
    request_queue_size = 8192
    allow_reuse_address = True
    _MAX_IDLE = 64

    def __init__(self, address, handler) -> None:
        super().__init__(address, handler)
        self._conns: "queue.SimpleQueue" = queue.SimpleQueue()
        self._pool_lock = threading.Lock()
        self._idle = 0       # connection threads waiting for a connection, not yet promised one
        self._closed = False

    def process_request(self, request, client_address) -> None:
        with self._pool_lock:
            spawn = self._idle == 0
            if not spawn:
                self._idle -= 1  # that thread takes this connection
        self._conns.put((request, client_address))
        if spawn:
            threading.Thread(target=self._connection_thread, name="nanopow-conn", daemon=True).start()

    def _connection_thread(self) -> None:
        while True:
            item = self._conns.get()
            if item is None:
                return
            request, client_address = item
            try:
                self.finish_request(request, client_address)
            except Exception:
                self.handle_error(request, client_address)
            finally:
                self.shutdown_request(request)
            with self._pool_lock:
                if self._closed or self._idle >= self._MAX_IDLE:
                    return
                self._idle += 1

    def server_close(self) -> None:
        super().server_close()
        with self._pool_lock:
            self._closed = True
            idle, self._idle = self._idle, 0
        for _ in range(idle):
            self._conns.put(None)


class HttpWorkServer:
    """WorkServer behind a threaded HTTP/1.1 listener (one thread per connection)."""

    def __init__(self, work_server: WorkServer, host: str = "127.0.0.1", port: int = 7000) -> None:
        handler = type("Connection", (_Connection,), {"work_server": work_server})
        self.work_server = work_server
        self.httpd = _Listener((host, port), handler)
        self._thread: Optional[threading.Thread] = None

    @property
    def address(self) -> str:
        h, p = self.httpd.server_address[:2]
        return f"{h}:{p}"

    def start(self) -> "HttpWorkServer":
        self.work_server.start()
        self._thread = threading.Thread(target=self.httpd.serve_forever, name="nanopow-http", daemon=True)
        self._thread.start()
        return self

    def serve_forever(self) -> None:
        self.work_server.start()
        self.httpd.serve_forever()

    def stop(self) -> None:
        self.work_server.stop()
        self.httpd.shutdown()
        self.httpd.server_close()
