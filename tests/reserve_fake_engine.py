"""A gated stand-in engine whose tickets hold a scripted reserve (TEST INFRASTRUCTURE): tests/fake_engine.py's
OracleEngine with submit() replaced, so that a search stays in flight until the test opens the gate -- or a relax is
answered from the reserve -- and answers at the threshold its ticket holds by then.  No GPU."""
import threading

from fake_engine import OracleEngine
from nanopow import _lib

WIN_NONCE = 0x1234


class ReserveTicket:
    def __init__(self, eng, root, threshold, reserve):
        self.eng, self.root, self.threshold, self.reserve_threshold = eng, root, threshold, reserve
        self.held = eng.scripted      # (nonce, value) or None: what reserve() reports
        self.relaxed = []             # every threshold asked for
        self.retargeted = []
        self.peeks = 0
        self.answered = threading.Event()
        self.ev = threading.Event()   # the search is over: the gate was opened, or a relax was answered
        if eng.gate.is_set():
            self.ev.set()

    def wait(self, timeout=None):
        if not self.ev.wait(timeout):
            return None
        if self.answered.is_set():
            return _lib.SearchResult(_lib.NPOW_OK, self.held[0], self.held[1], 1)
        return _lib.SearchResult(_lib.NPOW_OK, WIN_NONCE, self.threshold, 1)

    def reserve(self):
        self.peeks += 1
        return None if self.held is None else _lib.SearchResult(_lib.NPOW_OK, self.held[0], self.held[1], 0)

    def relax(self, threshold):
        self.relaxed.append(threshold)
        if self.reserve_threshold is None or threshold < self.reserve_threshold:
            raise _lib.NanoPowError(_lib.NPOW_ERR_BAD_ARGUMENT, "below the search's reserve threshold")
        if self.eng.too_late:
            return None
        if threshold >= self.threshold:
            return False
        self.threshold = threshold
        if self.held is not None and self.held[1] >= threshold:
            self.answered.set()
            self.ev.set()
            return True
        return False

    def retarget(self, threshold):
        self.retargeted.append(threshold)
        self.threshold = max(self.threshold, threshold)
        return True


class OldTicket:
    """A ticket of an engine without reserves."""

    def __init__(self, eng, root, threshold, reserve):
        self.eng, self.root, self.threshold = eng, root, threshold
        self.ev = threading.Event()
        if eng.gate.is_set():
            self.ev.set()

    def wait(self, timeout=None):
        if not self.ev.wait(timeout):
            return None
        return _lib.SearchResult(_lib.NPOW_OK, WIN_NONCE, self.threshold, 1)


class _Gate:
    """Opened by the test: every search in flight, and every later one, ends."""

    def __init__(self, eng):
        self.eng, self.open = eng, False

    def set(self):
        self.open = True
        for t in list(self.eng.tickets):
            t.ev.set()

    def is_set(self):
        return self.open


class ReserveEngine(OracleEngine):
    """work_value: the scripted reserve nonce has the scripted value (the server re-validates a reserve reply);
    every other nonce the oracle's."""

    def __init__(self, ticket_cls=ReserveTicket, scripted=None, too_late=False):
        super().__init__()
        self.gate = _Gate(self)
        self.ticket_cls = ticket_cls
        self.scripted = scripted
        self.too_late = too_late
        self.submits = []   # (root, threshold, keywords)
        self.tickets = []
        self.slock = threading.Lock()

    def work_value(self, root, nonce):
        if self.scripted is not None and nonce == self.scripted[0]:
            return self.scripted[1]
        return super().work_value(root, nonce)

    def submit(self, root, threshold, start=0, device_mask=0, max_nonces_per_device=0, cancel=None, **kw):
        assert set(kw) <= {"weight", "reserve"}, kw
        self.submits.append((root, threshold, dict(kw)))
        with self.slock:  # (a ticket made while the gate opens is in the list, or sees the gate open)
            t = self.ticket_cls(self, root, threshold, kw.get("reserve"))
            self.tickets.append(t)
        if self.gate.is_set():
            t.ev.set()
        return t
