"""Background searches (npow_submit_background) on the CPU side: the rules of nano-dpow_amd/csrc/npow_weights.h that
the host and the kernel share -- effective class, pick order, move rule, the start map with classes -- checked
exhaustively from a small compiled program; the declaration and the export; and the JSON server and the DPoW work
handler against a fake engine.  No GPU here; the shares are measured in tests/test_gpu_background.py."""
import asyncio
import os
import random
import re
import subprocess
import threading
import time

import pytest

from conftest import ROOT
from nanopow import _lib, dpow
from nanopow.server import WorkServer

HEADER = os.path.join(ROOT, "include", "nanopow.h")
CSRC = os.path.join(ROOT, "nano-dpow_amd", "csrc")


# ---- the rules ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("bg")
    src = d / "bg.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "npow_weights.h"
using namespace npow;

// The start of workgroup g as the kernel computes it (ls2_pick): a lane's weight is 0 for a flagged entry, else
// 8 >> wsh; the entry is the number of inclusive prefix sums <= pool_start_pos(g, wsum).
static uint32_t kernel_start(uint32_t g, uint32_t n, uint32_t wsum, const uint32_t* wsh, const uint8_t* bg) {
  if (!wsum) return g % n;
  const uint32_t r = pool_start_pos(g, wsum);
  uint32_t acc = 0, k = 0;
  for (uint32_t i = 0; i < n; ++i) {
    acc += bg[i] ? 0u : 8u >> (wsh[i] & 3u);
    if (acc <= r) ++k;
  }
  return k < n ? k : n - 1;
}

// One table: nf foreground weights f[] and nb background entries, laid out by `layout` (0: background entries spread
// between the foreground ones, 1: all first, 2: all last).  Returns the number of violated properties.
static unsigned check_table(const uint32_t* f, uint32_t nf, uint32_t nb, uint32_t grid, int layout) {
  uint32_t w[64], wsh[64], down = 99;
  uint8_t bg[64], bg0[64];
  uint32_t n = 0, fi = 0, bi = 0;
  while (fi < nf || bi < nb) {
    bool put_bg;
    if (layout == 1) put_bg = bi < nb;
    else if (layout == 2) put_bg = fi >= nf;
    else put_bg = bi < nb && (fi >= nf || (uint64_t)bi * nf <= (uint64_t)fi * nb);
    if (put_bg) { w[n] = 1; bg[n] = 1; ++bi; } else { w[n] = f[fi++]; bg[n] = 0; }
    bg0[n] = bg[n];
    ++n;
  }
  const uint32_t wsum = pool_table_weights_bg(w, bg, n, grid, wsh, &down);
  unsigned bad = 0;
  if (memcmp(bg, bg0, n)) return 1000;  // the flags were cleared: not at these grids
  if (nf == 0) {  // background only: dealt g % n, every shift that of weight 1
    if (wsum != 0 || down != 0) ++bad;
    for (uint32_t i = 0; i < n; ++i) bad += wsh[i] != kWshOne;
    return bad;
  }
  if (nb == 0) return bad;  // (pool_table_weights itself: tests/test_weights_cpu.py)
  if (wsum == 0) ++bad;  // non-zero also when the foreground weights are all equal
  uint32_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (bg[i]) { bad += wsh[i] != kWshOne; continue; }
    const uint32_t eff = (w[i] >> down) ? (w[i] >> down) : 1u;
    bad += wsh[i] != pool_wsh(eff);
    sum += eff;
  }
  if (sum != wsum) ++bad;  // the sum of the foreground weights
  uint64_t started = 0, want = 0;
  for (uint32_t g = 0; g < grid; ++g) started |= 1ull << kernel_start(g, n, wsum, wsh, bg);
  for (uint32_t i = 0; i < n; ++i) if (!bg[i]) want |= 1ull << i;
  if (started & ~want) ++bad;   // a workgroup starts on a background entry
  if (want & ~started) ++bad;   // a foreground entry starts with none
  return bad;
}

int main(int argc, char** argv) {
  if (!strcmp(argv[1], "class")) {  // flag mirror_gen mirror_level entry_gen -> background?
    const uint64_t mirror = (strtoull(argv[3], 0, 0) << 2) | (uint64_t)atoi(argv[4]);
    printf("%d\n", pool_eff_background((uint32_t)atoi(argv[2]), mirror, strtoull(argv[5], 0, 0)) ? 1 : 0);
  } else if (!strcmp(argv[1], "order")) {
    // every pair of (class, shift, count 0..64): violations of the pick order and of the move rule, and pairs that
    // admit a move in both directions
    unsigned order = 0, move = 0, both = 0, cross = 0, within = 0;
    for (int ca = 0; ca < 2; ++ca) for (int cb = 0; cb < 2; ++cb)
      for (uint32_t sa = 0; sa < 4; ++sa) for (uint32_t sb = 0; sb < 4; ++sb)
        for (unsigned long long a = 0; a <= 64; ++a) for (unsigned long long b = 0; b <= 64; ++b) {
          const uint32_t ka = pool_pick_key(ca, a, sa), kb = pool_pick_key(cb, b, sb);
          if (ca != cb) {
            if ((ka < kb) != (ca < cb)) ++order;  // foreground (class 0) first, whatever the counts
          } else if (ca == 0) {
            if ((ka < kb) != ((a << sa) < (b << sb)) || (ka == kb) != ((a << sa) == (b << sb))) ++order;
          } else {
            if ((ka < kb) != (a < b) || (ka == kb) != (a == b)) ++order;  // weight 1 among themselves
          }
          // a workgroup of B (b of them; b > 0) looks at A
          if (b == 0) continue;
          const bool m = pool_should_move_class(ca, a, sa, cb, b, sb);
          bool want;
          if (ca != cb) { want = cb == 1; ++cross; }
          else if (ca == 0) { want = pool_should_move(a, sa, b, sb); ++within; }
          else { want = pool_should_move(a, kWshOne, b, kWshOne); ++within; }
          if (m != want) ++move;
          if (m && pool_should_move_class(cb, b - 1, sb, ca, a + 1, sa)) ++both;  // ... and back again
        }
    printf("%u %u %u %u %u\n", order, move, both, cross, within);
  } else if (!strcmp(argv[1], "startmap")) {  // grid layout -> tables checked, violations
    const uint32_t grid = (uint32_t)atoi(argv[2]);
    const int layout = atoi(argv[3]);
    unsigned long long tables = 0, bad = 0;
    // every multiset of up to 20 foreground weights (n1 ones, n2 twos, n4 fours, n8 eights; heaviest first and
    // lightest first), with 1..16 background entries
    for (uint32_t n8 = 0; n8 <= 20; ++n8) for (uint32_t n4 = 0; n8 + n4 <= 20; ++n4)
      for (uint32_t n2 = 0; n8 + n4 + n2 <= 20; ++n2) for (uint32_t n1 = 0; n8 + n4 + n2 + n1 <= 20; ++n1) {
        const uint32_t nf = n8 + n4 + n2 + n1;
        uint32_t f[20], r[20];
        uint32_t k = 0;
        for (uint32_t i = 0; i < n8; ++i) f[k++] = 8;
        for (uint32_t i = 0; i < n4; ++i) f[k++] = 4;
        for (uint32_t i = 0; i < n2; ++i) f[k++] = 2;
        for (uint32_t i = 0; i < n1; ++i) f[k++] = 1;
        for (uint32_t i = 0; i < nf; ++i) r[i] = f[nf - 1 - i];
        for (uint32_t nb = 1; nb <= 16; ++nb) {
          bad += check_table(f, nf, nb, grid, layout);
          if (nf > 1 && (nb & 3) == 1) bad += check_table(r, nf, nb, grid, layout), ++tables;
          ++tables;
        }
      }
    printf("%llu %llu\n", tables, bad);
  } else if (!strcmp(argv[1], "plain")) {  // no background entry: exactly pool_table_weights
    unsigned bad = 0;
    const uint32_t sets[4][5] = {{1, 1, 1, 1, 1}, {8, 1, 1, 2, 4}, {8, 8, 8, 8, 8}, {4, 1, 8, 1, 2}};
    for (auto& s : sets) for (uint32_t grid : {128u, 1024u}) {
      uint32_t a[5], b[5], da = 0, db = 0;
      uint8_t bg[5] = {0, 0, 0, 0, 0};
      const uint32_t wa = pool_table_weights(s, 5, grid, a, &da), wb = pool_table_weights_bg(s, bg, 5, grid, b, &db);
      bad += wa != wb || da != db || memcmp(a, b, sizeof(a)) != 0;
    }
    printf("%u\n", bad);
  }
  return 0;
}
''')
    exe = d / "bg"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
        return [[int(x) for x in ln.split()] for ln in out.splitlines()]
    return run


def test_pick_order_and_move_rule_over_both_classes(rules):
    """Exhaustive: both classes, all shifts, counts 0..64.  Foreground sorts first; within a class the key is the
    count << shift (background: the plain count); moves across the classes go from background to foreground only;
    and no pair of entries admits a move in both directions."""
    (order, move, both, cross, within), = rules("order")
    assert cross > 0 and within > 0
    assert order == 0 and move == 0
    assert both == 0


@pytest.mark.parametrize("grid,layout", [(128, 0), (128, 1), (128, 2), (1024, 0)])
def test_start_map_with_classes(rules, grid, layout):
    """Every mix of up to 20 foreground weights and 1..16 background entries (spread, all first, all last): no
    workgroup starts on a background entry, every foreground entry gets one, wsum > 0 also when the foreground weights
    are all equal, and a background-only table gives wsum == 0."""
    (tables, bad), = rules("startmap", grid, layout)
    assert tables > 10626 * 16
    assert bad == 0


def test_a_table_without_background_entries_is_built_as_before(rules):
    assert rules("plain") == [[0]]


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_effective_class_follows_the_mirror(rules, level):
    gen = (1 << 40) + 7
    assert rules("class", 1, gen, level, gen) == [[0]]      # the mirror carries the entry's generation: lifted
    assert rules("class", 1, gen - 1, level, gen) == [[1]]  # the slot's previous job was promoted: not this one
    assert rules("class", 1, gen + 1, level, gen) == [[1]]  # ... nor a later one
    assert rules("class", 1, 0, level, gen) == [[1]]        # no promotion yet
    assert rules("class", 0, gen, level, gen) == [[0]]      # a foreground entry is foreground
    assert rules("class", 0, 0, level, gen) == [[0]]


# ---- the header and the export ---------------------------------------------------------------------------------------
def test_header_declares_npow_submit_background_within_abi_7():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+npow_submit_background\s*\(([^)]*)\)", txt)
    assert m, "include/nanopow.h does not declare npow_submit_background"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "const uint8_t root[32]", "uint64_t threshold", "uint64_t start", "uint64_t device_mask",
        "const volatile uint32_t* cancel", "uint64_t* ticket"]
    assert re.search(r"#define NPOW_ABI_VERSION (\d+)", txt).group(1) == "7"
    assert _lib.NPOW_ABI_VERSION == 7
    rev = raw[raw.index("ABI revision"):raw.index("#define NPOW_ABI_VERSION")]
    assert "npow_submit_background" in rev


def test_library_exports_npow_submit_background():
    lib = _lib.load()
    assert hasattr(lib, "npow_submit_background") and hasattr(lib, "npow_ticket_background")
    assert "npow_submit_background" in _lib.EXPORTED_SYMBOLS
    assert lib.npow_abi_version() == 7


def test_engine_submit_background_needs_the_symbol():
    class OldLib:
        pass

    eng = _lib.Engine.__new__(_lib.Engine)
    eng.lib = OldLib()
    with pytest.raises(_lib.NanoPowError) as e:
        eng.submit(b"\0" * 32, 1, background=True)
    assert e.value.code == _lib.NPOW_ERR_BAD_ARGUMENT


# ---- the JSON server against a fake engine ---------------------------------------------------------------------------
LOW = "ff00000000000000"
A, B, C, D = "AA" * 32, "BB" * 32, "CC" * 32, "DD" * 32


class _Ticket:
    def __init__(self, eng, threshold):
        self.eng, self.threshold = eng, threshold
        self.promoted = []

    def wait(self, timeout=None):
        # (never for ever: a test that fails before it opens the gate must not leave a thread behind)
        if not self.eng.gate.wait(20 if timeout is None else timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, 0x1234, self.threshold, 1)

    def promote(self, weight):
        self.promoted.append(weight)


class FakeEngine:
    def __init__(self):
        self.gate = threading.Event()
        self.calls = []  # (root, the keywords beyond the usual ones)
        self.tickets = []

    def submit(self, root, threshold, start=0, device_mask=0, max_nonces_per_device=0, cancel=None, **kw):
        assert set(kw) <= {"weight", "background"}, kw
        self.calls.append((root, kw))
        self.tickets.append(_Ticket(self, threshold))
        return self.tickets[-1]

    def work_value(self, root, nonce):
        return 0


class _Asker:
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
    eng = FakeEngine()
    srv = WorkServer(eng, max_active=1).start()
    asker = _Asker(srv)
    yield eng, srv, asker
    eng.gate.set()
    asker.join()
    srv.stop()


def test_keyword_is_passed_only_when_asked_for(served):
    eng, srv, asker = served
    asker.ask(A, background=True)
    _until(lambda: len(eng.tickets) == 1)
    assert srv.status() == {"generating": "1", "queue_size": "0", "background": "1"}
    asker.ask(B)  # a foreground request does not wait for the background one, even at max_active 1
    _until(lambda: len(eng.tickets) == 2)
    asker.ask(C, background=False)
    _until(lambda: int(srv.status()["queue_size"]) == 1)
    eng.gate.set()
    asker.join()
    b = bytes.fromhex
    assert eng.calls == [(b(A), {"background": True}), (b(B), {}), (b(C), {})]
    assert srv.status() == {"generating": "0", "queue_size": "0"}
    assert all(r.get("work") == "0000000000001234" for r in asker.replies)


@pytest.mark.parametrize("value", [1, 0, "true", "1", 2.0, [True], {}])
def test_non_boolean_background_is_rejected(served, value):
    eng, srv, asker = served
    eng.gate.set()  # (a server that took the request would answer it with work at once, not block this thread)
    reply = srv.handle({"action": "work_generate", "hash": A, "difficulty": LOW, "background": value})
    assert reply == {"error": "Bad background", "hint": "Expecting true or false"}
    assert eng.calls == []


def test_foreground_duplicate_promotes_a_running_background_job(served):
    eng, srv, asker = served
    asker.ask(A, background=True)
    _until(lambda: len(eng.tickets) == 1)
    asker.ask(A, background=True)  # a background duplicate only shares the result
    _until(lambda: _waiters(srv, A) == 2)
    assert eng.tickets[0].promoted == []
    asker.ask(A)  # a foreground one lifts it, at weight 1
    _until(lambda: _waiters(srv, A) == 3)
    assert eng.tickets[0].promoted == [1]
    assert "background" not in srv.status()
    asker.ask(A, weight=4)  # ... and from then on weights rise as for any job
    _until(lambda: _waiters(srv, A) == 4)
    asker.ask(A)
    _until(lambda: _waiters(srv, A) == 5)
    assert eng.tickets[0].promoted == [1, 4]
    assert len(eng.calls) == 1


def test_work_promote_lifts_a_running_background_job(served):
    eng, srv, asker = served
    asker.ask(A, background=True)
    _until(lambda: len(eng.tickets) == 1)
    assert srv.handle({"action": "work_promote", "hash": A, "weight": 2}) == {}
    assert eng.tickets[0].promoted == [2]
    assert srv.handle({"action": "work_promote", "hash": A, "weight": 2}) == {}  # foreground now: nothing to raise
    assert eng.tickets[0].promoted == [2]


def test_queue_order_foreground_first(served):
    eng, srv, asker = served
    asker.ask(A)  # runs (max_active 1)
    _until(lambda: len(eng.tickets) == 1)
    for i, (r, extra) in enumerate(((B, {"background": True}), (C, {"background": True}), (D, {}))):
        asker.ask(r, **extra)
        _until(lambda: int(srv.status()["queue_size"]) == i + 1)
    E = "EE" * 32
    asker.ask(E, weight=2)
    _until(lambda: int(srv.status()["queue_size"]) == 4)
    asker.ask(C)  # a foreground duplicate lifts C where it stands: weight 1 is FIFO by arrival, and C came before D
    _until(lambda: _waiters(srv, C) == 2)
    assert all(t.promoted == [] for t in eng.tickets)
    eng.gate.set()
    asker.join()
    b = bytes.fromhex
    assert eng.calls == [(b(A), {}), (b(E), {"weight": 2}), (b(C), {}), (b(D), {}), (b(B), {"background": True})]


# ---- the DPoW work handler -------------------------------------------------------------------------------------------
class _StubWorker:
    uri = "stub"

    def __init__(self):
        self.bodies = []
        self.release = None

    async def post(self, obj):
        self.bodies.append(dict(obj))
        if obj.get("action") == "work_generate":
            await self.release.wait()
            return {"work": "00000000000000ab"}
        if obj.get("action") in ("work_promote", "work_cancel"):
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


DIFF = "fffffff800000000"


def test_handler_sends_background_types_as_background_and_ondemand_promotes():
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message("work/precache", f"{A},{DIFF}".encode())  # the same type again: ignored
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())  # default weights: still a promotion
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())
        worker.release.set()
        await _settle(lambda: not h.ongoing)
        await asyncio.sleep(0.01)
    bodies, published, stats = _run_handler(script, background_types=("precache",))
    assert [b for b in bodies if b["action"] == "work_generate"] == [
        {"action": "work_generate", "hash": A, "difficulty": DIFF, "background": True}]
    assert [b for b in bodies if b["action"] == "work_promote"] == [
        {"action": "work_promote", "hash": A, "weight": 1}]
    assert published == [("result/ondemand", f"{A},00000000000000ab,nano_payout".encode())]
    assert stats["promoted"] == 1 and stats["ignored"] == 2


def test_handler_retypes_a_queued_background_hash_and_sends_it_foreground():
    async def script(h, worker):
        await h.on_message("work/precache", f"{B},{DIFF}".encode())
        await _settle(lambda: B in h.ongoing)
        await h.on_message("work/precache", f"{A},{DIFF}".encode())  # waits in the queue (concurrency 1)
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())
        assert h.queue[A] == (DIFF, "ondemand")
        worker.release.set()
        await _settle(lambda: not h.ongoing and not h.queue)
    bodies, published, stats = _run_handler(script, background_types=("precache",),
                                            weights={"ondemand": 8, "precache": 1})
    gens = [b for b in bodies if b["action"] == "work_generate"]
    assert gens == [{"action": "work_generate", "hash": B, "difficulty": DIFF, "background": True},
                    {"action": "work_generate", "hash": A, "difficulty": DIFF, "weight": 8}]
    assert not [b for b in bodies if b["action"] == "work_promote"]


def test_handler_without_the_option_is_unchanged():
    async def script(h, worker):
        await h.on_message("work/precache", f"{A},{DIFF}".encode())
        await _settle(lambda: A in h.ongoing)
        await h.on_message("work/ondemand", f"{A},{DIFF}".encode())
        worker.release.set()
        await _settle(lambda: not h.ongoing)
    bodies, published, stats = _run_handler(script)
    assert [b["action"] for b in bodies] == ["invalid", "work_generate"] and "background" not in bodies[1]
    assert stats["promoted"] == 0 and stats["ignored"] == 1
