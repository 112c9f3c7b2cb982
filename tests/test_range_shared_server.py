"""work_best's ``"shared"`` (a shared best job, npow_submit_best_shared) against a stand-in engine: the value is parsed
as strictly as ``"background"``, passed on to the engine only when it is set, refused together with ``"background"``,
and the reply is the same either way.  The engine is tests/best_fake_engine.py's with the keywords added.  No GPU."""
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


class ClassBestEngine(BestEngine):
    """BestEngine whose submit_best takes `background` and `shared` and remembers the keywords it was given."""

    def __init__(self):
        super().__init__()
        self.classes = []

    def submit_best(self, root, start, count, floor=0, device_mask=0, cancel=None, **kw):
        assert set(kw) <= {"background", "shared"}, kw
        self.classes.append(dict(kw))
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


def test_true_reaches_submit_best_and_the_reply_is_unchanged(want):
    eng = ClassBestEngine()
    s = WorkServer(eng, device_mask=1).start()
    assert s.handle(_request(shared=True)) == want
    assert eng.classes == [{"shared": True}] and eng.best_calls == [(ROOT_A, START, COUNT, 0, 1)]
    assert s.handle(_request(shared=True, background=False)) == want
    assert eng.classes[-1] == {"shared": True}
    s.stop()


@pytest.mark.parametrize("extra", [{"shared": False}, {}, {"shared": None}])
def test_false_and_absent_are_a_plain_best_job(want, extra):
    eng = ClassBestEngine()
    s = WorkServer(eng).start()
    assert s.handle(_request(**extra)) == want
    assert eng.classes == [{}]  # the keyword is passed only when it is set
    old = BestEngine()  # ... so an engine from before the class still serves the plain request
    s2 = WorkServer(old).start()
    assert s2.handle(_request(**extra)) == want and len(old.best_calls) == 1
    assert s.handle(_request(background=True, **extra)) == want and eng.classes[-1] == {"background": True}
    s.stop()
    s2.stop()


def test_shared_together_with_background_is_refused():
    eng = ClassBestEngine()
    s = WorkServer(eng).start()
    r = s.handle(_request(shared=True, background=True))
    assert r == {"error": "Bad shared", "hint": "Expecting shared or background, not both"}
    assert not eng.best_calls
    s.stop()


@pytest.mark.parametrize("bad", ["true", "false", 1, 0, "1", "", [True], {"x": 1}, 1.0])
def test_a_non_boolean_is_refused_as_background_refuses_it(bad):
    eng = ClassBestEngine()
    s = WorkServer(eng).start()
    assert s.handle(_request(shared=bad)) == {"error": "Bad shared", "hint": "Expecting true or false"}
    assert not eng.best_calls
    s.stop()
