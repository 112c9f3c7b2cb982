"""A gated stand-in engine whose tickets record retarget calls (TEST INFRASTRUCTURE): tests/fake_engine.py's
OracleEngine with submit() replaced, so that a search stays in flight until the test opens the gate and answers at
the threshold its ticket holds by then.  No GPU."""
import threading

from fake_engine import OracleEngine
from nanopow import _lib


class RetargetTicket:
    def __init__(self, eng, root, threshold):
        self.eng, self.root, self.threshold = eng, root, threshold
        self.retargeted = []   # every threshold asked for
        self.promoted = []

    def wait(self, timeout=None):
        if not self.eng.gate.wait(timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, 0x1234, self.threshold, 1)

    def promote(self, weight):
        self.promoted.append(weight)

    def retarget(self, threshold):
        self.retargeted.append(threshold)
        if self.eng.too_late:
            return False
        self.threshold = max(self.threshold, threshold)
        return True


class OldTicket:
    """A ticket of an engine without retargeting."""

    def __init__(self, eng, root, threshold):
        self.eng, self.root, self.threshold = eng, root, threshold

    def wait(self, timeout=None):
        if not self.eng.gate.wait(timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, 0x1234, self.threshold, 1)


class RetargetEngine(OracleEngine):
    def __init__(self, ticket_cls=RetargetTicket, too_late=False):
        super().__init__()
        self.gate = threading.Event()
        self.ticket_cls = ticket_cls
        self.too_late = too_late   # retarget() answers False: the search was already decided
        self.submits = []          # (root, threshold)
        self.tickets = []

    def submit(self, root, threshold, start=0, device_mask=0, max_nonces_per_device=0, cancel=None, **kw):
        assert set(kw) <= {"weight"}, kw
        self.submits.append((root, threshold))
        t = self.ticket_cls(self, root, threshold)
        self.tickets.append(t)
        return t
