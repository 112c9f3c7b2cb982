"""work_best's ``"background"`` (a background best job, npow_submit_best_background) against a stand-in engine: the
value is parsed as strictly as work_generate's, passed on to the engine only when it is set, and the reply is the
same either way.  The engine is tests/best_fake_engine.py's with the keyword added.  No GPU."""
import numpy as np
import pytest

import oracle
from best_fake_engine import BestEngine, BestTicket
from nanopow import work as W
from nanopow.server import WorkServer

ROOT_A = bytes(range(3, 35))
H = ROOT_A.hex().upper()
START = 0x0123456789abcdef
COUNT = 4097


class BackgroundBestEngine(BestEngine):
    """BestEngine whose submit_best takes `background` and remembers it (None: the keyword was not passed)."""

    def __init__(self):
        super().__init__()
        self.classes = []

    def submit_best(self, root, start, count, floor=0, device_mask=0, cancel=None, **kw):
        assert set(kw) <= {"background"}, kw
        self.classes.append(kw.get("background"))
        self.best_calls.append((root, start, count, floor, device_mask))
        return BestTicket(self, root, start, count, floor, cancel)


@pytest.fixture(scope="module")
def want():
    v = oracle.work_values_range(ROOT_A, START, COUNT, threads=2)
    k = int(np.argmax(v))
    nonce, value = START + k, int(v[k])
    return {"work": f"{nonce:016x}", "difficulty": f"{value:016x}",
            "multiplier": W.fmt_multiplier(W.to_multiplier(value, W.DEFAULT_BASE)), "hashes": str(COUNT)}


def _request(**extra):
    return dict({"action": "work_best", "hash": H, "count": COUNT, "start": f"{START:016x}"}, **extra)


def test_true_is_passed_on_and_the_reply_is_unchanged(want):
    eng = BackgroundBestEngine()
    s = WorkServer(eng, device_mask=1).start()
    assert s.handle(_request(background=True)) == want
    assert eng.classes == [True] and eng.best_calls == [(ROOT_A, START, COUNT, 0, 1)]
    s.stop()


@pytest.mark.parametrize("extra", [{"background": False}, {}, {"background": None}])
def test_false_and_absent_are_a_plain_best_job(want, extra):
    eng = BackgroundBestEngine()
    s = WorkServer(eng).start()
    assert s.handle(_request(**extra)) == want
    assert eng.classes == [None]  # the keyword is passed only when it is set
    # ... so an engine from before the class still serves the plain request
    old = BestEngine()
    s2 = WorkServer(old).start()
    assert s2.handle(_request(**extra)) == want and len(old.best_calls) == 1
    s.stop()
    s2.stop()


@pytest.mark.parametrize("bad", ["true", "false", 1, 0, "1", "", [True], {"x": 1}, 1.0])
def test_a_non_boolean_is_refused_as_work_generate_refuses_it(bad):
    eng = BackgroundBestEngine()
    s = WorkServer(eng).start()
    r = s.handle(_request(background=bad))
    assert r == {"error": "Bad background", "hint": "Expecting true or false"}
    assert r == s.handle({"action": "work_generate", "hash": H, "background": bad})
    assert not eng.best_calls
    s.stop()


def test_the_floor_and_a_random_start_go_with_it(want):
    eng = BackgroundBestEngine()
    s = WorkServer(eng).start()
    floor = int(want["difficulty"], 16)
    r = s.handle(_request(background=True, difficulty=f"{floor:016x}"))
    assert r == want and eng.best_calls[-1][3] == floor and eng.classes[-1] is True
    assert s.handle(_request(background=True, difficulty=f"{floor + 1:016x}")) == {"error": "Exhausted"}
    r = s.handle({"action": "work_best", "hash": H, "count": 64, "background": True})
    assert oracle.work_value_hashlib(ROOT_A, int(r["work"], 16)) == int(r["difficulty"], 16) and r["hashes"] == "64"
    assert eng.classes == [True, True, True]
    s.stop()
