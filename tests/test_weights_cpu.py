"""Job weights on the CPU side: the ABI revision and the npow_submit_weighted declaration, the work server's
``"weight"`` field and queue order, and the DPoW work handler's per-type weights.  No GPU here; the shares
themselves are measured in tests/test_gpu_weights.py."""
import asyncio
import os
import random
import re
import threading
import time

import pytest

from conftest import ROOT
from fake_engine import OracleEngine
from nanopow import __main__ as cli
from nanopow import _lib, dpow
from nanopow.server import Job, WorkServer

HEADER = os.path.join(ROOT, "include", "nanopow.h")
LOW = "ff00000000000000"  # a threshold the oracle engine meets within a few hundred nonces


def test_abi_7_declares_the_weighted_submit():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+npow_submit_weighted\s*\(([^)]*)\)", txt)
    assert m, "include/nanopow.h does not declare npow_submit_weighted"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[6] == "uint32_t weight" and args[7] == "uint64_t* ticket", args
    assert re.search(r"#define NPOW_ABI_VERSION (\d+)", txt).group(1) == "7"
    assert _lib.NPOW_ABI_VERSION == 7
    assert _lib.load().npow_abi_version() == 7
    assert "npow_submit_weighted" in _lib.EXPORTED_SYMBOLS


class _GatedTicket:
    def __init__(self, gate, threshold):
        self.gate, self.threshold = gate, threshold

    def wait(self, timeout=None):
        if not self.gate.wait(timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, 0x1234, self.threshold, 1)


class WeightEngine:
    """Records each submit's keywords; its searches end when the gate opens (open from the start by default)."""

    def __init__(self, gated=False):
        self.gate = threading.Event()
        if not gated:
            self.gate.set()
        self.calls = []  # (root, weight keyword or None)

    def submit(self, root, threshold, start=0, device_mask=0, max_nonces_per_device=0, cancel=None, **kw):
        assert set(kw) <= {"weight"}, kw
        self.calls.append((root, kw.get("weight")))
        return _GatedTicket(self.gate, threshold)

    def work_value(self, root, nonce):
        return 0


def _generate(srv, root_hex, **extra):
    return srv.handle({"action": "work_generate", "hash": root_hex, "difficulty": LOW, **extra})


@pytest.mark.parametrize("weight", [4, "4"])
def test_work_generate_passes_a_weight_to_the_engine(weight):
    eng = WeightEngine()
    srv = WorkServer(eng, max_active=2).start()
    try:
        reply = _generate(srv, "AB" * 32, weight=weight)
    finally:
        srv.stop()
    assert reply["work"] == "0000000000001234" and reply["difficulty"] == LOW
    assert eng.calls == [(bytes.fromhex("AB" * 32), 4)]


@pytest.mark.parametrize("weight", [3, "x", 0, "3", 16, -1, 2.0, True, "", " 4", [4]])
def test_work_generate_refuses_other_weights(weight):
    eng = WeightEngine()
    srv = WorkServer(eng, max_active=2).start()
    try:
        reply = _generate(srv, "AB" * 32, weight=weight)
    finally:
        srv.stop()
    assert reply == {"error": "Bad weight", "hint": "Expecting 1, 2, 4 or 8"}
    assert eng.calls == []


@pytest.mark.parametrize("extra", [{}, {"weight": 1}, {"weight": "1"}, {"weight": None}])
def test_unweighted_requests_reach_an_engine_without_the_keyword(extra):
    """tests/fake_engine.py's engine has no `weight` keyword: requests of weight 1 must not pass one."""
    eng = OracleEngine(chunk=1 << 12)
    srv = WorkServer(eng, max_active=2).start()
    try:
        reply = _generate(srv, "CD" * 32, **extra)
    finally:
        srv.stop()
    assert "work" in reply, reply
    assert eng.work_value(bytes.fromhex("CD" * 32), int(reply["work"], 16)) >= int(LOW, 16)
    eng2 = WeightEngine()
    srv = WorkServer(eng2, max_active=2).start()
    try:
        _generate(srv, "CD" * 32, **extra)
    finally:
        srv.stop()
    assert eng2.calls == [(bytes.fromhex("CD" * 32), None)]


def test_queue_pump_takes_the_heaviest_first():
    """max_active 1: behind a running request, queued weights [1, 8, 1, 4] reach the engine as 8, 4, 1, 1 (FIFO
    within a weight)."""
    eng = WeightEngine(gated=True)
    srv = WorkServer(eng, max_active=1).start()
    roots = [f"{i:02X}" * 32 for i in range(5)]
    weights = [1, 1, 8, 1, 4]  # the first one runs, the others queue in this order
    replies = {}

    def ask(i):
        extra = {"weight": weights[i]} if weights[i] != 1 else {}
        replies[i] = _generate(srv, roots[i], **extra)

    threads = []
    try:
        for i in range(5):
            t = threading.Thread(target=ask, args=(i,))
            t.start()
            threads.append(t)
            deadline = time.time() + 10
            while (len(eng.calls) if i == 0 else int(srv.status()["queue_size"])) != (1 if i == 0 else i):
                assert time.time() < deadline
                time.sleep(0.001)
        eng.gate.set()
        for t in threads:
            t.join(10)
    finally:
        eng.gate.set()
        srv.stop()
    assert all("work" in replies[i] for i in range(5)), replies
    b = [bytes.fromhex(r) for r in roots]
    assert eng.calls == [(b[0], None), (b[2], 8), (b[4], 4), (b[1], None), (b[3], None)]


def test_shuffle_stays_within_the_heaviest_weight():
    eng = WeightEngine(gated=True)
    srv = WorkServer(eng, max_active=1, shuffle=True, rng=random.Random(5)).start()
    try:
        with srv._lock:
            srv._inflight.append(Job(b"\xff" * 32, 0))  # something runs: requests queue
        jobs = [srv._enqueue(bytes([i]) * 32, 1, w) for i, w in enumerate([1, 2, 8, 1, 8, 2])]
        with srv._lock:
            srv._inflight.clear()
            order = []
            while srv._queue:
                ready = srv._pump_locked()
                order += [j.weight for j in ready]
                srv._inflight.clear()
        assert order == [8, 8, 2, 2, 1, 1] and len(jobs) == 6
    finally:
        eng.gate.set()
        with srv._lock:
            srv._inflight.clear()
        srv.stop()


class _Worker:
    uri = "fake"

    def __init__(self):
        self.bodies = []

    async def post(self, obj):
        self.bodies.append(dict(obj))
        if obj.get("action") == "work_generate":
            return {"work": "0000000000000001"}
        return {"error": "Unknown command"}


def _handle(messages, **kw):
    worker = _Worker()
    published = []

    async def main():
        async def publish(topic, payload):
            published.append((topic, payload))

        h = dpow.DpowWorkHandler(worker, publish, "nano_payout", rng=random.Random(3), **kw)
        await h.start()
        for topic, payload in messages:
            await h.on_message(topic, payload)
        for _ in range(2000):
            if len(published) == len(messages):
                break
            await asyncio.sleep(0.001)
        await h.stop()
    asyncio.run(main())
    assert len(published) == len(messages)
    return {b["hash"]: b for b in worker.bodies if b.get("action") == "work_generate"}


def test_dpow_handler_weights_by_work_type():
    on, pre = "AA" * 32, "BB" * 32
    msgs = [("work/ondemand", f"{on},fffffff800000000".encode()), ("work/precache", f"{pre},fffffff800000000".encode())]
    bodies = _handle(msgs, weights={"ondemand": 8, "precache": 1})
    assert bodies[on] == {"action": "work_generate", "hash": on, "difficulty": "fffffff800000000", "weight": 8}
    assert bodies[pre] == {"action": "work_generate", "hash": pre, "difficulty": "fffffff800000000"}
    bodies = _handle(msgs)  # the default weights: no body carries the field
    assert all("weight" not in b for b in bodies.values()) and set(bodies) == {on, pre}
    with pytest.raises(ValueError):
        dpow.DpowWorkHandler(_Worker(), None, "nano_payout", weights={"ondemand": 3})


def test_cli_ondemand_weight():
    assert cli.dpow_weights(cli.parse_args([])) == {"ondemand": 1, "precache": 1}
    assert cli.dpow_weights(cli.parse_args(["--ondemand-weight", "8"])) == {"ondemand": 8, "precache": 1}
    with pytest.raises(SystemExit):
        cli.parse_args(["--ondemand-weight", "3"])


def test_engine_submit_needs_abi_7_for_a_weight():
    """Engine.submit against a library without npow_submit_weighted: weight 1 goes through npow_submit, any other
    weight raises."""
    calls = []

    class OldLib:
        def npow_submit(self, *a):
            calls.append(a)
            return _lib.NPOW_OK

        def npow_last_error(self):
            return b""

    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = OldLib()
    t = eng.submit(bytes(32), 1, weight=1)
    t.result = _lib.SearchResult(_lib.NPOW_CANCELLED, None, None, 0)  # nothing to collect from the stand-in
    assert len(calls) == 1
    with pytest.raises(_lib.NanoPowError):
        eng.submit(bytes(32), 1, weight=8)
    assert len(calls) == 1


TABLE_CASES = [
    # (weights, grid): whole GPU 1024 workgroups, a 32-CU partition 128, smaller parts
    ([1, 4], 1024), ([1] * 8 + [8], 1024), ([8] * 20, 128), ([1] * 16, 128), ([8] * 64, 1024), ([8] * 17 + [1], 128),
    ([8] * 20 + [1, 2, 4, 8] * 4, 128), ([8] * 63 + [1], 128), ([8] * 63 + [1], 1024), ([8, 4] * 32, 128),
    ([8] * 40 + [2] * 24, 64), ([8, 1], 4), ([4, 2, 1], 32), ([2, 2, 2], 16), ([8], 128), ([], 128),
]


@pytest.fixture(scope="module")
def table_weights(tmp_path_factory):
    """pool_table_weights (nano-dpow_amd/csrc/npow_weights.h), the rule Worker::build_table builds a table's weights and
    start map with, compiled into a small program: weights and the grid in, wsum, the halvings and each wsh out."""
    import subprocess
    d = tmp_path_factory.mktemp("tw")
    src = d / "tw.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "npow_weights.h"\n'
                   "int main(int argc, char** argv) {\n"
                   "  uint32_t w[64], wsh[64], down = 0, grid = (uint32_t)atoi(argv[1]), n = (uint32_t)(argc - 2);\n"
                   "  for (uint32_t i = 0; i < n; ++i) w[i] = (uint32_t)atoi(argv[2 + i]);\n"
                   "  const uint32_t wsum = npow::pool_table_weights(w, n, grid, wsh, &down);\n"
                   '  printf("%u %u", wsum, down);\n'
                   '  for (uint32_t i = 0; i < n; ++i) printf(" %u", wsh[i]);\n'
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = d / "tw"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "nano-dpow_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)

    def run(weights, grid):
        out = subprocess.run([str(exe), str(grid)] + [str(x) for x in weights], capture_output=True, text=True,
                             check=True).stdout.split()
        return int(out[0]), int(out[1]), [int(x) for x in out[2:]]
    return run


def _start_counts(eff, grid):
    """The kernel's start (ls2_pick with pool_start_pos): how many of the grid's workgroups start on each entry."""
    wsum, n = sum(eff), len(eff)
    prefix = [sum(eff[:i + 1]) for i in range(n)]
    started = [0] * n
    for g in range(grid):
        r = (((g * 0x9E3779B9) & 0xffffffff) * wsum) >> 32
        started[min(n - 1, sum(1 for p in prefix if p <= r))] += 1
    return started


@pytest.mark.parametrize("weights,grid", TABLE_CASES)
def test_table_builder_gives_every_entry_a_workgroup(table_weights, weights, grid):
    """Whatever the jobs' weights and the device's grid: a workgroup starts on every entry of a mapped table (as
    g % n gives every entry one); equal weights take no map; the table's weights are the jobs' halved alike, floor
    1, and no further than an empty entry made necessary; the workgroups are dealt in proportion to the weights."""
    wsum, down, wsh = table_weights(weights, grid)
    eff = [max(1, w >> down) for w in weights]
    assert wsh == [3 - (e.bit_length() - 1) for e in eff]
    if len(set(weights)) <= 1:
        assert (wsum, down) == (0, 0)  # equal weights: g % n, the jobs' own wsh
        return
    for k in range(down):  # every lighter halving left an entry without a workgroup
        assert min(_start_counts([max(1, w >> k) for w in weights], grid)) == 0
    if wsum == 0:
        assert len(set(eff)) == 1 and down > 0  # halved until equal: g % n
        return
    assert wsum == sum(eff)
    started = _start_counts(eff, grid)
    assert min(started) >= 1, started
    # shares: within 2 workgroups (and 1/4) of grid x weight / wsum -- the spread map's discrepancy
    for e, c in zip(eff, started):
        want = grid * e / wsum
        assert abs(c - want) <= max(2.0, want / 4), (e, c, want)


def test_start_map_spreads_every_stretch_of_workgroups():
    """Workgroups are dispatched in index order and the earliest on a CU run fastest, so each quarter of the grid
    (one workgroup per CU) must hold each entry's share too, not only the grid as a whole: weights (1, 4) and eight
    light jobs beside a heavy one on a whole GPU, quarter by quarter within 2 workgroups (and 1/4) of the share;
    and every XCD shard (g mod 8) likewise."""
    for eff in ([1, 4], [1] * 8 + [8]):
        wsum, n = sum(eff), len(eff)
        prefix = [sum(eff[:i + 1]) for i in range(n)]
        entry = [sum(1 for p in prefix if p <= ((((g * 0x9E3779B9) & 0xffffffff) * wsum) >> 32)) for g in range(1024)]
        parts = [range(q * 256, (q + 1) * 256) for q in range(4)] + [range(x, 1024, 8) for x in range(8)]
        for part in parts:
            for i, e in enumerate(eff):
                c, want = sum(1 for g in part if entry[g] == i), len(part) * e / wsum
                assert abs(c - want) <= max(2.0, want / 4), (eff, part, i, c, want)


def test_table_builder_keeps_whole_gpu_weights(table_weights):
    """On a whole GPU (1,024 workgroups) the tests' tables are dealt at their jobs' own weights."""
    assert table_weights([1, 4], 1024) == (5, 0, [3, 1])
    assert table_weights([1] * 8 + [8], 1024) == (16, 0, [3] * 8 + [0])
    wsum, down, _ = table_weights([8] * 20 + [1], 128)  # a CU partition: 161 over 128 workgroups leaves entries empty
    assert down >= 1 and 0 < wsum <= 81


def test_heavier_duplicate_raises_a_queued_request():
    """The same root and threshold asked again with a larger weight while the first request still waits in the
    server's queue: the queued job takes the larger weight (a job already in the engine keeps its own)."""
    eng = WeightEngine(gated=True)
    srv = WorkServer(eng, max_active=1).start()
    try:
        with srv._lock:
            srv._inflight.append(Job(b"\xff" * 32, 0))
        a = srv._enqueue(b"\x01" * 32, 1, 1)
        b = srv._enqueue(b"\x02" * 32, 1, 2)
        assert srv._enqueue(b"\x01" * 32, 1, 8) is a and a.weight == 8 and a.waiters == 2
        assert srv._enqueue(b"\x02" * 32, 1, 1) is b and b.weight == 2
        with srv._lock:
            srv._inflight.clear()
            first = srv._pump_locked()
        assert first == [a]
        assert srv._enqueue(b"\x01" * 32, 1, 4) is a and a.weight == 8  # in flight now
    finally:
        eng.gate.set()
        with srv._lock:
            srv._inflight.clear()
            srv._queue.clear()
        srv.stop()
