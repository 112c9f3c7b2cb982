"""A stand-in engine with best jobs (TEST INFRASTRUCTURE): tests/fake_engine.py's OracleEngine plus submit_best,
answered from the oracle's work values of the range -- argmax, first occurrence on ties -- as the library's best job
is.  A gated engine holds every best job in flight until the test opens the gate or cancels it.  No GPU."""
import threading

import numpy as np

import oracle
from fake_engine import OracleEngine
from nanopow import _lib


class BestTicket:
    def __init__(self, eng, root, start, count, floor, cancel):
        self.eng, self.root, self.start, self.count, self.floor, self.cancel_token = eng, root, start, count, floor, cancel

    def wait(self, timeout=None):
        while not self.eng.gate.wait(0.005):
            if self.cancel_token is not None and self.cancel_token.is_set:
                return _lib.BestResult(_lib.NPOW_CANCELLED, None, None, 0)
        v = oracle.work_values_range(self.root, self.start, self.count, threads=2)
        k = int(np.argmax(v))
        if int(v[k]) < self.floor:
            return _lib.BestResult(_lib.NPOW_EXHAUSTED, None, None, self.count)
        return _lib.BestResult(_lib.NPOW_OK, (self.start + k) & ((1 << 64) - 1), int(v[k]), self.count)


class BestEngine(OracleEngine):
    def __init__(self, gated=False):
        super().__init__()
        self.gate = threading.Event()
        if not gated:
            self.gate.set()
        self.best_calls = []  # (root, start, count, floor, device_mask)

    def submit_best(self, root, start, count, floor=0, device_mask=0, cancel=None):
        self.best_calls.append((root, start, count, floor, device_mask))
        return BestTicket(self, root, start, count, floor, cancel)
