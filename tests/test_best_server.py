"""The JSON action work_best (this server's extension) against a stand-in engine with best jobs
(tests/best_fake_engine.py): the reply's fields, Exhausted, Cancelled and the parser's errors.  No GPU."""
import threading
import time

import numpy as np
import pytest

import oracle
from best_fake_engine import BestEngine
from fake_engine import OracleEngine
from nanopow import work as W
from nanopow.server import WorkServer

ROOT_A = bytes(range(3, 35))
H = ROOT_A.hex().upper()
START = 0x0123456789abcdef
COUNT = 4097


@pytest.fixture(scope="module")
def want():
    v = oracle.work_values_range(ROOT_A, START, COUNT, threads=2)
    k = int(np.argmax(v))
    return START + k, int(v[k])


def server(eng, **kw):
    return WorkServer(eng, **kw).start()


def test_reply_fields(want):
    eng = BestEngine()
    s = server(eng, device_mask=1)
    r = s.handle({"action": "work_best", "hash": H, "count": COUNT, "start": f"{START:016x}"})
    nonce, value = want
    assert r == {"work": f"{nonce:016x}", "difficulty": f"{value:016x}",
                 "multiplier": W.fmt_multiplier(W.to_multiplier(value, W.DEFAULT_BASE)), "hashes": str(COUNT)}
    assert oracle.work_value_hashlib(ROOT_A, int(r["work"], 16)) == int(r["difficulty"], 16)
    assert eng.best_calls == [(ROOT_A, START, COUNT, 0, 1)]
    # the multiplier is quoted against the server's base difficulty, as work_generate quotes it
    base = 0xfffffe0000000000
    r2 = server(BestEngine(), base_threshold=base).handle(
        {"action": "work_best", "hash": H, "count": str(COUNT), "start": f"{START:016x}"})
    assert r2["work"] == r["work"] and r2["multiplier"] == W.fmt_multiplier(W.to_multiplier(value, base))
    s.stop()


def test_random_start_and_floor_are_passed_on(want):
    eng = BestEngine()
    s = server(eng)
    r = s.handle({"action": "work_best", "hash": H, "count": 64})
    (root, start, count, floor, _), = eng.best_calls
    assert (root, count, floor) == (ROOT_A, 64, 0) and 0 <= start < 1 << 64
    assert oracle.work_value_hashlib(ROOT_A, int(r["work"], 16)) == int(r["difficulty"], 16) and r["hashes"] == "64"
    _, value = want
    r = s.handle({"action": "work_best", "hash": H, "count": COUNT, "start": f"{START:016x}",
                  "difficulty": f"{value:016x}"})
    assert int(r["difficulty"], 16) == value and eng.best_calls[-1][3] == value
    s.stop()


def test_exhausted_when_nothing_reaches_the_floor(want):
    _, value = want
    s = server(BestEngine())
    r = s.handle({"action": "work_best", "hash": H, "count": COUNT, "start": f"{START:016x}",
                  "difficulty": f"{value + 1:016x}"})
    assert r == {"error": "Exhausted"}
    s.stop()


def test_work_cancel_of_the_hash_cancels_it():
    eng = BestEngine(gated=True)
    s = server(eng)
    out = {}
    th = threading.Thread(target=lambda: out.update(
        s.handle({"action": "work_best", "hash": H, "count": 1 << 30, "start": f"{START:016x}"})))
    th.start()
    deadline = time.time() + 10
    while not eng.best_calls and time.time() < deadline:
        time.sleep(0.001)
    assert eng.best_calls
    other = bytes(32).hex()
    assert s.handle({"action": "work_cancel", "hash": other}) == {}  # another hash: it runs on
    th.join(0.05)
    assert th.is_alive()
    assert s.handle({"action": "work_cancel", "hash": H}) == {}
    th.join(10)
    assert not th.is_alive() and out == {"error": "Cancelled"}
    eng.gate.set()
    s.stop()


@pytest.mark.parametrize("count", [0, -1, (1 << 40) + 1, "0", "12x", "", 1.5, True, None, [4], "1" * 30])
def test_bad_counts(count):
    eng = BestEngine()
    r = server(eng).handle({"action": "work_best", "hash": H, "count": count})
    assert r["error"] == "Bad count" and "positive integer" in r["hint"] and not eng.best_calls


def test_count_limit_and_other_parser_errors():
    eng = BestEngine(gated=True)
    s = server(eng)
    assert W.parse_best_count({"count": 1 << 40}) == 1 << 40 and W.parse_best_count({"count": "1"}) == 1
    r = s.handle({"action": "work_best", "hash": H})
    assert r == {"error": "Failed to deserialize JSON", "hint": "count field missing"}
    r = s.handle({"action": "work_best", "count": 64})
    assert r == {"error": "Failed to deserialize JSON", "hint": "Hash field missing"}
    assert s.handle({"action": "work_best", "hash": "zz", "count": 64})["error"] == "Bad block hash"
    for start in ("123", "0x23456789abcdef0", 5, "0123456789abcdeg", "0123456789abcdef0"):
        r = s.handle({"action": "work_best", "hash": H, "count": 64, "start": start})
        assert r == {"error": "Bad start", "hint": "Expecting 16 hex digits for start"}, start
    r = s.handle({"action": "work_best", "hash": H, "count": 64, "difficulty": "nope"})
    assert r["error"] == "Bad difficulty"
    assert not eng.best_calls
    s.stop()


def test_an_engine_without_best_jobs_does_not_know_the_action():
    r = server(OracleEngine()).handle({"action": "work_best", "hash": H, "count": 64})
    assert r == {"error": "Unknown command", "hint": W.SUPPORTED}
