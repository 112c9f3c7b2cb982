"""ctypes binding of libnanopow.so (the C ABI declared in include/nanopow.h).

The product path has no CPU fallback: if the HIP library is missing, or no
GPU is visible, every entry point here raises :class:`NanoPowError`.  ctypes
releases the GIL for the duration of each foreign call, so searches can run in
worker threads while the HTTP server keeps serving ``work_cancel``
(client/work_handler.py:61-80 sends it on a second connection while a
``work_generate`` is pending).
"""
from __future__ import annotations

import ctypes
import os
import threading
import time
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NANOPOW_LIB", os.path.join(_HERE, "libnanopow.so"))

NPOW_OK = 0
NPOW_CANCELLED = 1
NPOW_EXHAUSTED = 2
NPOW_PENDING = 3
NPOW_TOO_LATE = 4  # npow_retarget, npow_relax: the search was already decided or cancelled (not yet collected)
NPOW_ERR_NOT_INITIALISED = -1
NPOW_ERR_NO_DEVICE = -2
NPOW_ERR_BAD_ARGUMENT = -3
NPOW_ERR_HIP = -4
NPOW_ERR_INVALID_WORK = -5
NPOW_ERR_CAPACITY = -6
NPOW_ERR_INTERNAL = -7

NPOW_ABI_VERSION = 7
NPOW_RESERVE_MIN = 0xfffff00000000000  # the lowest reserve threshold (npow_submit_reserve)
# hash paths of npow_values_path
NPOW_PATH_SEARCH = 0   # the stream the search and sweep kernels execute (four 512-lane workgroups per CU)
NPOW_PATH_SEQ = 1      # a second generated stream, scheduled without barriers
NPOW_PATH_GENERIC = 2  # plain HIP C++ of the 12 rounds, one (root, nonce) per lane

NPOW_SWEEP_JOB_HITS = 1 << 20  # hits one device keeps for one sweep job (Engine.submit_sweep)

M64 = (1 << 64) - 1

# Every symbol include/nanopow.h declares (tests/test_abi.py checks the export table).
EXPORTED_SYMBOLS = (
    "npow_init", "npow_shutdown", "npow_last_error", "npow_work_value", "npow_search",
    "npow_search_batch", "npow_sweep", "npow_values", "npow_values_pairs", "npow_set_tuning",
    "npow_device_stats_get", "npow_device_stats_reset", "npow_version",
    "npow_submit", "npow_wait", "npow_cancel", "npow_pool_config", "npow_pool_status",
    "npow_set_pool_tuning", "npow_values_path", "npow_wait_info", "npow_device_stats_get_sized",
    "npow_abi_version", "npow_config_cpu_threads", "npow_wait_result", "npow_submit_weighted",
    "npow_promote", "npow_retarget", "npow_submit_background", "npow_ticket_background",
    "npow_submit_reserve", "npow_ticket_reserve", "npow_relax", "npow_submit_sweep", "npow_wait_sweep",
    "npow_submit_sweep_background", "npow_ticket_sweep", "npow_submit_best", "npow_wait_best", "npow_ticket_best",
    "npow_submit_best_background", "npow_ticket_best_hold",
    "npow_submit_sweep_shared", "npow_submit_best_shared", "npow_ticket_share",
)


class NanoPowError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"nanopow error {code}: {message}")
        self.code = code
        self.message = message


class DeviceStats(ctypes.Structure):
    _fields_ = [
        ("launches", ctypes.c_uint64),
        ("nonces", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("invalid_work", ctypes.c_uint64),
        ("cus", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("clock_mhz", ctypes.c_double),
        ("host_cpu_ms", ctypes.c_double),
        ("host_wall_ms", ctypes.c_double),
        ("dead", ctypes.c_int32),
        ("pool_groups", ctypes.c_int32),
        ("early_finishes", ctypes.c_uint64),
        ("early_mismatches", ctypes.c_uint64),
        ("yields", ctypes.c_uint64),
        ("dyn_entries", ctypes.c_uint64),
        ("kills_relayed", ctypes.c_uint64),  # ABI 3
        ("late_nonces", ctypes.c_uint64),    # ABI 4
        ("hip_device", ctypes.c_int32),
        ("cu_first", ctypes.c_int32),
        ("idle_ms", ctypes.c_double),        # ABI 5
        ("idle_gaps", ctypes.c_uint64),
        ("affinity_checks", ctypes.c_uint64),
        ("affinity_failures", ctypes.c_uint64),
        ("watcher_decisions", ctypes.c_uint64),
        # ABI 6
        ("stale_drains", ctypes.c_uint64),
        ("linger_ms", ctypes.c_double),
        ("linger_relays", ctypes.c_uint64),
        ("stale_late", ctypes.c_uint64),
        ("stale_missing", ctypes.c_uint64),
        ("stale_gpu_delay_us", ctypes.c_double),
        ("promotions", ctypes.c_uint64),     # ABI 7, with npow_promote
    ]


class SearchInfo(ctypes.Structure):
    """npow_search_info: one search's outcome and host timeline (us since npow_submit)."""
    _fields_ = [
        ("size", ctypes.c_uint32),
        ("status", ctypes.c_int32),
        ("nonce", ctypes.c_uint64),
        ("value", ctypes.c_uint64),
        ("nonces_done", ctypes.c_uint64),
        ("winner_device", ctypes.c_int32),
        ("n_devices", ctypes.c_int32),
        ("decide_us", ctypes.c_double),
        ("finish_us", ctypes.c_double),
        ("stop_after_decide_us", ctypes.c_double),
        ("overshoot_nonces", ctypes.c_uint64),
        ("late_nonces_losers", ctypes.c_uint64),  # ABI 4: counted on the devices
        ("late_nonces_winner", ctypes.c_uint64),
        ("adopt_us", ctypes.c_double),            # ABI 5: host timeline
        ("launch_us", ctypes.c_double),
        ("launch_all_us", ctypes.c_double),
        ("win_seen_us", ctypes.c_double),
        ("retargets", ctypes.c_uint64),           # ABI 7, with npow_retarget
        ("stale_hits", ctypes.c_uint64),
        ("stale_wins", ctypes.c_uint64),
    ]


class ReserveInfo(ctypes.Structure):
    """npow_reserve_info: the reserve of a search submitted with a reserve threshold (npow_ticket_reserve)."""
    _fields_ = [
        ("size", ctypes.c_uint32),
        ("armed", ctypes.c_uint32),
        ("reserve_threshold", ctypes.c_uint64),
        ("threshold", ctypes.c_uint64),
        ("nonce", ctypes.c_uint64),
        ("value", ctypes.c_uint64),
        ("device", ctypes.c_int32),
        ("answered", ctypes.c_uint32),
        ("relaxes", ctypes.c_uint64),
        ("candidates", ctypes.c_uint64),
    ]


class _SweepInfoStruct(ctypes.Structure):
    """npow_sweep_info as the C ABI lays it out (npow_ticket_sweep)."""
    _fields_ = [
        ("size", ctypes.c_uint32),
        ("background", ctypes.c_uint32),
        ("count", ctypes.c_uint64),
        ("nonces_done", ctypes.c_uint64),
        ("hits", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("launches_cut", ctypes.c_uint64),
        ("held_us", ctypes.c_uint64),
        ("finished", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
    ]


@dataclass
class SweepInfo:
    """A look at an uncollected sweep job (SweepTicket.info, npow_ticket_sweep)."""
    background: bool       # submitted with background=True
    count: int             # nonces of the range
    nonces_done: int       # credited by the launches retired so far
    hits: int              # read from the launches retired so far
    launches: int          # launches that held an entry of the job, summed over its devices
    launches_cut: int      # of those, launches a yield or the time budget ended before their span was hashed
    held_us: int           # time the job sat admitted but left out of its devices' tables
    finished: bool         # wait() would return at once


class _BestInfoStruct(ctypes.Structure):
    """npow_best_info as the C ABI lays it out (npow_ticket_best)."""
    _fields_ = [
        ("size", ctypes.c_uint32),
        ("finished", ctypes.c_uint32),
        ("count", ctypes.c_uint64),
        ("nonces_done", ctypes.c_uint64),
        ("nonce", ctypes.c_uint64),
        ("value", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("records", ctypes.c_uint64),
        ("records_max", ctypes.c_uint64),
        ("room", ctypes.c_uint64),
    ]


@dataclass
class BestInfo:
    """A look at an uncollected best job (BestTicket.info, npow_ticket_best)."""
    finished: bool         # wait() would return at once
    count: int             # nonces of the range
    nonces_done: int       # credited by the launches retired so far
    nonce: int             # the best candidate of the launches retired so far ...
    value: int             # ... and its work value (0: none yet)
    launches: int          # launches that held an entry of the job, summed over its devices
    records: int           # candidates those launches recorded, all told
    records_max: int       # the most one launch's entry recorded
    room: int              # the fewest records one of its entries had room for (0: no launch retired yet)


class _BestHoldStruct(ctypes.Structure):
    """npow_best_hold_info as the C ABI lays it out (npow_ticket_best_hold)."""
    _fields_ = [
        ("size", ctypes.c_uint32),
        ("background", ctypes.c_uint32),
        ("launches_cut", ctypes.c_uint64),
        ("held_us", ctypes.c_uint64),
    ]


@dataclass
class BestHold:
    """A best job's class and what it cost it (BestTicket.hold, npow_ticket_best_hold); a plain job reads 0, 0, 0."""
    background: int        # 1: submitted with background=True
    launches_cut: int      # launches a yield or the time budget ended before their span was hashed
    held_us: int           # time the job sat admitted but left out of its devices' tables

    def __iter__(self):    # background, launches_cut, held_us = ticket.hold()
        return iter((self.background, self.launches_cut, self.held_us))


class _RangeShareStruct(ctypes.Structure):
    """npow_range_share_info as the C ABI lays it out (npow_ticket_share)."""
    _fields_ = [
        ("size", ctypes.c_uint32),
        ("klass", ctypes.c_uint32),
        ("launches", ctypes.c_uint64),
        ("launches_cut", ctypes.c_uint64),
        ("held_us", ctypes.c_uint64),
        ("moves", ctypes.c_uint64),
    ]


RANGE_PLAIN, RANGE_BACKGROUND, RANGE_SHARED = 0, 1, 2  # npow_range_share_info.klass


@dataclass
class RangeShare:
    """The class of a sweep or best job and what came with it (SweepTicket.share, BestTicket.share,
    npow_ticket_share)."""
    klass: int             # RANGE_PLAIN, RANGE_BACKGROUND or RANGE_SHARED
    launches: int          # launches that held an entry of the job, summed over its devices
    launches_cut: int      # of those, launches a yield or the time budget ended before their span was hashed
    held_us: int           # time the job sat admitted but left out of its devices' tables (background jobs only)
    moves: int             # workgroups that came to the job's entry from another entry of a running launch


@dataclass
class BestResult:
    status: int            # NPOW_OK / NPOW_EXHAUSTED (nothing reached the floor) / NPOW_CANCELLED
    nonce: Optional[int]   # the range's strongest nonce (cancelled: the best found so far; None: none)
    value: Optional[int]
    nonces_done: int       # == count unless cancelled

    def __iter__(self):    # status, nonce, value, nonces_done = ticket.wait()
        return iter((self.status, self.nonce, self.value, self.nonces_done))


@dataclass
class SweepResult:
    status: int            # NPOW_OK, or NPOW_CANCELLED (hits then holds what was found before it)
    hits: List[int]        # ascending (nonce - start); at most cap of them
    total: int             # exact number of hits (may exceed len(hits) only with status != OK)
    nonces_done: Optional[int] = None  # a sweep job's (SweepTicket.wait): nonces hashed, == count when status is OK


@dataclass
class SearchResult:
    status: int            # NPOW_OK / NPOW_CANCELLED / NPOW_EXHAUSTED
    nonce: Optional[int]
    value: Optional[int]
    nonces_done: int


_lib: Optional[ctypes.CDLL] = None
_lib_lock = threading.Lock()


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libnanopow.so and declare every prototype (no device is touched)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise NanoPowError(NPOW_ERR_NOT_INITIALISED,
                               f"{path} not built: run `make -C nano-dpow_amd/csrc` "
                               "(or __graft_entry__.build())")
        lib = ctypes.CDLL(path)
        u8p = ctypes.c_char_p
        u64, u32 = ctypes.c_uint64, ctypes.c_uint32
        pu64 = ctypes.POINTER(ctypes.c_uint64)
        p = ctypes.c_void_p
        lib.npow_init.argtypes = [ctypes.POINTER(ctypes.c_int)]
        lib.npow_init.restype = ctypes.c_int
        lib.npow_shutdown.argtypes = []
        lib.npow_shutdown.restype = None
        lib.npow_last_error.argtypes = []
        lib.npow_last_error.restype = ctypes.c_char_p
        lib.npow_version.argtypes = []
        lib.npow_version.restype = ctypes.c_char_p
        lib.npow_work_value.argtypes = [u8p, u64]
        lib.npow_work_value.restype = u64
        lib.npow_search.argtypes = [u8p, u64, u64, u64, u64, p, pu64, pu64, pu64]
        lib.npow_search.restype = ctypes.c_int
        lib.npow_search_batch.argtypes = [u8p, p, u32, u64, u64, p, p, p, p, pu64]
        lib.npow_search_batch.restype = ctypes.c_int
        lib.npow_sweep.argtypes = [u8p, u64, u64, u64, u64, p, p, u64, pu64]
        lib.npow_sweep.restype = ctypes.c_int
        lib.npow_values.argtypes = [ctypes.c_int, u8p, u64, u64, p]
        lib.npow_values.restype = ctypes.c_int
        lib.npow_values_pairs.argtypes = [ctypes.c_int, u8p, p, u32, p]
        lib.npow_values_pairs.restype = ctypes.c_int
        lib.npow_set_tuning.argtypes = [u32, u32, u32]
        lib.npow_set_tuning.restype = ctypes.c_int
        lib.npow_device_stats_get.argtypes = [ctypes.c_int, ctypes.POINTER(DeviceStats)]
        lib.npow_device_stats_get.restype = ctypes.c_int
        lib.npow_device_stats_reset.argtypes = [ctypes.c_int]
        lib.npow_device_stats_reset.restype = ctypes.c_int
        lib.npow_submit.argtypes = [u8p, u64, u64, u64, u64, p, pu64]
        lib.npow_submit.restype = ctypes.c_int
        lib.npow_wait.argtypes = [u64, ctypes.c_int64, pu64, pu64, pu64]
        lib.npow_wait.restype = ctypes.c_int
        lib.npow_cancel.argtypes = [u64]
        lib.npow_cancel.restype = ctypes.c_int
        lib.npow_pool_config.argtypes = [u32]
        lib.npow_pool_config.restype = ctypes.c_int
        lib.npow_pool_status.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        lib.npow_pool_status.restype = ctypes.c_int
        lib.npow_set_pool_tuning.argtypes = [u32, u32]
        lib.npow_set_pool_tuning.restype = ctypes.c_int
        # ABI 3 (a library of an earlier revision, e.g. an A/B build of round-2 sources, lacks them:
        # stats() then falls back to npow_device_stats_get, whose struct is a prefix of DeviceStats)
        if hasattr(lib, "npow_abi_version"):
            lib.npow_values_path.argtypes = [ctypes.c_int, u8p, u64, u64, ctypes.c_int, p]
            lib.npow_values_path.restype = ctypes.c_int
            lib.npow_wait_info.argtypes = [u64, ctypes.c_int64, ctypes.POINTER(SearchInfo)]
            lib.npow_wait_info.restype = ctypes.c_int
            lib.npow_device_stats_get_sized.argtypes = [ctypes.c_int, ctypes.POINTER(DeviceStats), u64]
            lib.npow_device_stats_get_sized.restype = ctypes.c_int
            lib.npow_abi_version.argtypes = []
            lib.npow_abi_version.restype = ctypes.c_int
        if hasattr(lib, "npow_config_cpu_threads"):  # ABI 4
            lib.npow_config_cpu_threads.argtypes = [u32]
            lib.npow_config_cpu_threads.restype = ctypes.c_int
            lib.npow_wait_result.argtypes = [u64, ctypes.c_int64, pu64, pu64]
            lib.npow_wait_result.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_weighted"):  # ABI 7
            lib.npow_submit_weighted.argtypes = [u8p, u64, u64, u64, u64, p, u32, pu64]
            lib.npow_submit_weighted.restype = ctypes.c_int
        if hasattr(lib, "npow_promote"):  # added within ABI 7: probed for
            lib.npow_promote.argtypes = [u64, u32]
            lib.npow_promote.restype = ctypes.c_int
        if hasattr(lib, "npow_retarget"):  # added within ABI 7: probed for
            lib.npow_retarget.argtypes = [u64, u64]
            lib.npow_retarget.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_background"):  # added within ABI 7: probed for
            lib.npow_submit_background.argtypes = [u8p, u64, u64, u64, p, pu64]
            lib.npow_submit_background.restype = ctypes.c_int
            lib.npow_ticket_background.argtypes = [u64, ctypes.POINTER(ctypes.c_uint32)]
            lib.npow_ticket_background.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_reserve"):  # added within ABI 7: probed for
            lib.npow_submit_reserve.argtypes = [u8p, u64, u64, u64, u64, p, u32, u32, pu64]
            lib.npow_submit_reserve.restype = ctypes.c_int
            lib.npow_ticket_reserve.argtypes = [u64, ctypes.POINTER(ReserveInfo)]
            lib.npow_ticket_reserve.restype = ctypes.c_int
            lib.npow_relax.argtypes = [u64, u64, ctypes.POINTER(ctypes.c_uint32)]
            lib.npow_relax.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_sweep"):  # added within ABI 7: probed for
            lib.npow_submit_sweep.argtypes = [u8p, u64, u64, u64, u64, p, pu64]
            lib.npow_submit_sweep.restype = ctypes.c_int
            lib.npow_wait_sweep.argtypes = [u64, ctypes.c_int64, p, u64, pu64, pu64]
            lib.npow_wait_sweep.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_sweep_background"):  # added within ABI 7: probed for
            lib.npow_submit_sweep_background.argtypes = [u8p, u64, u64, u64, u64, p, pu64]
            lib.npow_submit_sweep_background.restype = ctypes.c_int
            lib.npow_ticket_sweep.argtypes = [u64, ctypes.POINTER(_SweepInfoStruct)]
            lib.npow_ticket_sweep.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_best"):  # added within ABI 7: probed for
            lib.npow_submit_best.argtypes = [u8p, u64, u64, u64, u64, p, pu64]
            lib.npow_submit_best.restype = ctypes.c_int
            lib.npow_wait_best.argtypes = [u64, ctypes.c_int64, pu64, pu64, pu64]
            lib.npow_wait_best.restype = ctypes.c_int
            lib.npow_ticket_best.argtypes = [u64, ctypes.POINTER(_BestInfoStruct)]
            lib.npow_ticket_best.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_best_background"):  # added within ABI 7: probed for
            lib.npow_submit_best_background.argtypes = [u8p, u64, u64, u64, u64, p, pu64]
            lib.npow_submit_best_background.restype = ctypes.c_int
            lib.npow_ticket_best_hold.argtypes = [u64, ctypes.POINTER(_BestHoldStruct)]
            lib.npow_ticket_best_hold.restype = ctypes.c_int
        if hasattr(lib, "npow_submit_sweep_shared"):  # added within ABI 7: probed for
            for f in (lib.npow_submit_sweep_shared, lib.npow_submit_best_shared):
                f.argtypes = [u8p, u64, u64, u64, u64, p, pu64]
                f.restype = ctypes.c_int
            lib.npow_ticket_share.argtypes = [u64, ctypes.POINTER(_RangeShareStruct)]
            lib.npow_ticket_share.restype = ctypes.c_int
        _lib = lib
        return lib


def _check(rc: int, lib: ctypes.CDLL, ok=(NPOW_OK,)) -> int:
    if rc in ok:
        return rc
    msg = lib.npow_last_error()
    raise NanoPowError(rc, msg.decode("utf-8", "replace") if msg else "")


def _root(root: bytes) -> bytes:
    if not isinstance(root, (bytes, bytearray)) or len(root) != 32:
        raise ValueError("root must be 32 bytes")
    return bytes(root)


class CancelToken:
    """A caller-owned 32-bit word the engine polls; set() stops a running search."""

    def __init__(self) -> None:
        self._word = ctypes.c_uint32(0)

    def set(self) -> None:
        self._word.value = 1

    def clear(self) -> None:
        self._word.value = 0

    @property
    def is_set(self) -> bool:
        return bool(self._word.value)

    @property
    def address(self) -> int:
        return ctypes.addressof(self._word)


_ORPHANED_CANCEL_WORDS: list = []


class _JobTicket:
    """What the tickets of the three kinds of pool job share.  Each kind has its wait() and _collect_abandoned(lib): its
    own wait of up to 10 s, the result thrown away, which returns the status."""

    def __init__(self, engine: "Engine", ticket: int, cancel: Optional[CancelToken]) -> None:
        self.engine = engine
        self.ticket = ticket
        self.cancel_token = cancel  # keeps the cancel word alive while the engine may read it
        self.result = None

    @staticmethod
    def _us(timeout: Optional[float]) -> int:
        return -1 if timeout is None else max(0, int(timeout * 1e6))

    @staticmethod
    def _need(lib, name: str) -> None:
        if not hasattr(lib, name):
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, f"the loaded libnanopow has no {name}")

    @staticmethod
    def _u64(name: str, v) -> None:
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= M64:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, f"{name} must be an integer in [0, 2^64)")

    def _uncollected(self) -> None:
        if self.result is not None:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "the ticket's result was already collected")

    def cancel(self) -> None:
        if self.result is None and self.ticket:
            _check(self.engine.lib.npow_cancel(self.ticket), self.engine.lib)

    def __del__(self) -> None:
        # An abandoned ticket: cancel its job and collect it, so the engine forgets the job
        # and stops reading this ticket's cancel word before that word is freed.  A job that
        # does not end within 10 s keeps its cancel word alive for the life of the process.
        if self.result is not None or not getattr(self, "ticket", 0):
            return
        try:
            lib = self.engine.lib
            lib.npow_cancel(self.ticket)
            if self._collect_abandoned(lib) == NPOW_PENDING:
                _ORPHANED_CANCEL_WORDS.append(self.cancel_token)
        except Exception:  # interpreter shutdown: the library may already be gone
            pass


class Ticket(_JobTicket):
    """A submitted search (npow_submit); wait() returns its SearchResult once."""

    def __init__(self, engine: "Engine", ticket: int, cancel: Optional[CancelToken]) -> None:
        super().__init__(engine, ticket, cancel)
        self.submitted_background = False  # Engine.submit(background=True): wait_info then reports how it ended

    def wait(self, timeout: Optional[float] = None) -> Optional[SearchResult]:
        """Block until the search ends (timeout None) or up to `timeout` seconds; None if
        it is still running then."""
        if self.result is not None:
            return self.result
        lib = self.engine.lib
        nonce, value, done = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib.npow_wait(self.ticket, self._us(timeout), ctypes.byref(nonce), ctypes.byref(value), ctypes.byref(done))
        if rc == NPOW_PENDING:
            return None
        self.cancel_token = None
        _check(rc, lib, ok=(NPOW_OK, NPOW_CANCELLED, NPOW_EXHAUSTED))
        self.result = (SearchResult(rc, nonce.value, value.value, done.value) if rc == NPOW_OK
                       else SearchResult(rc, None, None, done.value))
        return self.result

    def wait_result(self, timeout: Optional[float] = None) -> Optional[SearchResult]:
        """The search's outcome as soon as it is known (npow_wait_result: the winner accepted, the cancellation
        seen), before the other devices of a split search have stopped; None if still running after `timeout`
        seconds.  nonces_done is 0 here: wait() or wait_info() must still collect the ticket."""
        if self.result is not None:
            return self.result
        lib = self.engine.lib
        nonce, value = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib.npow_wait_result(self.ticket, self._us(timeout), ctypes.byref(nonce), ctypes.byref(value))
        if rc == NPOW_PENDING:
            return None
        _check(rc, lib, ok=(NPOW_OK, NPOW_CANCELLED, NPOW_EXHAUSTED))
        return (SearchResult(rc, nonce.value, value.value, 0) if rc == NPOW_OK
                else SearchResult(rc, None, None, 0))

    def wait_info(self, timeout: Optional[float] = None) -> Optional[SearchInfo]:
        """wait() with the search's timeline (npow_wait_info): winner device, host times of the
        decision and the finish, and the other devices' overshoot after the decision.  None if
        still running after `timeout` seconds."""
        if self.result is not None:
            raise RuntimeError("the ticket's result was already collected")
        lib = self.engine.lib
        info = SearchInfo()
        info.size = ctypes.sizeof(SearchInfo)
        us = self._us(timeout)
        # info.background (a Python attribute: npow_search_info keeps its layout): 1 if the search ended still
        # background.  Only a ticket submitted so can: its class is read once the search is decided (it no longer
        # changes then, npow_ticket_background) and before the ticket is released.
        ended_bg = 0
        if self.submitted_background:
            t0 = time.monotonic()
            if lib.npow_wait_result(self.ticket, us, None, None) == NPOW_PENDING:
                return None
            bg = ctypes.c_uint32(0)
            _check(lib.npow_ticket_background(self.ticket, ctypes.byref(bg)), lib)
            ended_bg = bg.value
            if us >= 0:
                us = max(0, us - int((time.monotonic() - t0) * 1e6))
        rc = lib.npow_wait_info(self.ticket, us, ctypes.byref(info))
        if rc == NPOW_PENDING:
            return None
        info.background = ended_bg
        self.cancel_token = None
        _check(rc, lib, ok=(NPOW_OK, NPOW_CANCELLED, NPOW_EXHAUSTED))
        self.result = (SearchResult(rc, info.nonce, info.value, info.nonces_done) if rc == NPOW_OK
                       else SearchResult(rc, None, None, info.nonces_done))
        return info

    def cancel(self) -> None:
        if self.result is None:
            _check(self.engine.lib.npow_cancel(self.ticket), self.engine.lib)

    def promote(self, weight: int) -> None:
        """Raise the search's weight to max(current, weight), weight in {1, 2, 4, 8} (npow_promote): a waiting
        search moves up the admission queue, a running one gets its new share inside the launch that holds it.
        A background search (submit(background=True)) becomes a foreground search of that weight, whatever the weight.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) for another weight, a collected ticket, a bounded search -- and when
        the loaded library has no npow_promote."""
        lib = self.engine.lib
        self._need(lib, "npow_promote")
        if not isinstance(weight, int) or isinstance(weight, bool) or not 0 <= weight <= 0xffffffff:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "weight must be 1, 2, 4 or 8")
        self._uncollected()
        _check(lib.npow_promote(self.ticket, weight), lib)

    def retarget(self, threshold: int) -> bool:
        """Raise the search's threshold to max(current, threshold) in place (npow_retarget): a waiting search is
        admitted with it, a running one keeps its slot, weight and nonce position and passes over hits that no
        longer qualify.  True when it holds -- every result the ticket returns from now on has a value at or
        above `threshold` -- and False when it came too late (NPOW_TOO_LATE: the search was already decided or
        cancelled; its result stands).  NanoPowError(NPOW_ERR_BAD_ARGUMENT) for a threshold outside 64 bits, a
        collected ticket -- and when the loaded library has no npow_retarget."""
        lib = self.engine.lib
        self._need(lib, "npow_retarget")
        self._u64("threshold", threshold)
        self._uncollected()
        return _check(lib.npow_retarget(self.ticket, threshold), lib, ok=(NPOW_OK, NPOW_TOO_LATE)) == NPOW_OK

    def reserve_info(self) -> ReserveInfo:
        """The search's reserve as npow_ticket_reserve reports it (a look: the search is not disturbed).
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) for a collected ticket -- and when the loaded library has no
        npow_ticket_reserve."""
        lib = self.engine.lib
        self._need(lib, "npow_ticket_reserve")
        self._uncollected()
        info = ReserveInfo()
        info.size = ctypes.sizeof(ReserveInfo)
        _check(lib.npow_ticket_reserve(self.ticket, ctypes.byref(info)), lib)
        return info

    def reserve(self) -> Optional[SearchResult]:
        """The best nonce the search has passed whose value is at or above its reserve threshold but below its
        threshold (submit(reserve=...)), validated on the CPU; None while there is none.  nonces_done is 0."""
        info = self.reserve_info()
        return SearchResult(NPOW_OK, info.nonce, info.value, 0) if info.value else None

    def relax(self, threshold: int) -> Optional[bool]:
        """Lower the search's threshold to min(current, threshold) in place (npow_relax; a search submitted with a
        reserve threshold, down to that threshold).  True when the search was decided at once from its reserve --
        wait_result() then returns without waiting -- False when the threshold was lowered inside the running search
        or nothing changed, None when it came too late (NPOW_TOO_LATE: the search was already decided or cancelled).
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) for a threshold outside 64 bits or below the reserve threshold, a search
        without a reserve, a collected ticket -- and when the loaded library has no npow_relax."""
        lib = self.engine.lib
        self._need(lib, "npow_relax")
        self._u64("threshold", threshold)
        self._uncollected()
        answered = ctypes.c_uint32(0)
        rc = _check(lib.npow_relax(self.ticket, threshold, ctypes.byref(answered)), lib, ok=(NPOW_OK, NPOW_TOO_LATE))
        return None if rc == NPOW_TOO_LATE else bool(answered.value)

    def _collect_abandoned(self, lib) -> int:
        return lib.npow_wait(self.ticket, 10_000_000, None, None, None)


def _range_share(t: "_JobTicket") -> RangeShare:
    lib = t.engine.lib
    t._need(lib, "npow_ticket_share")
    if not t.ticket:
        raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "the ticket is collected")
    i = _RangeShareStruct()
    i.size = ctypes.sizeof(_RangeShareStruct)
    _check(lib.npow_ticket_share(t.ticket, ctypes.byref(i)), lib)
    return RangeShare(i.klass, i.launches, i.launches_cut, i.held_us, i.moves)


class SweepTicket(_JobTicket):
    """A submitted sweep job (npow_submit_sweep); wait() returns its SweepResult once."""

    def __init__(self, engine: "Engine", ticket: int, cancel: Optional[CancelToken], cap: int) -> None:
        super().__init__(engine, ticket, cancel)
        self.cap = cap

    def wait(self, timeout: Optional[float] = None) -> Optional[SweepResult]:
        """Block until the job ends (timeout None) or up to `timeout` seconds; None if it is still running then.
        The result's status is NPOW_OK (hits is the exact hit set of the range, nonces_done == count),
        NPOW_CANCELLED (the hits found so far) or NPOW_ERR_CAPACITY (more hits than `cap`, or than
        NPOW_SWEEP_JOB_HITS on one device: total is exact, hits holds the first ones); any other error raises."""
        if self.result is not None:
            return self.result
        lib = self.engine.lib
        out = (ctypes.c_uint64 * max(self.cap, 1))()
        n, done = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib.npow_wait_sweep(self.ticket, self._us(timeout), ctypes.addressof(out), self.cap, ctypes.byref(n),
                                 ctypes.byref(done))
        if rc == NPOW_PENDING:
            return None
        self.cancel_token = None
        self.ticket = 0  # collected, whatever the status
        _check(rc, lib, ok=(NPOW_OK, NPOW_CANCELLED, NPOW_ERR_CAPACITY))
        self.result = SweepResult(rc, list(out[: min(n.value, self.cap)]), n.value, done.value)
        return self.result

    def info(self) -> SweepInfo:
        """The job's progress so far (npow_ticket_sweep); never waits for a GPU.  NanoPowError(NPOW_ERR_BAD_ARGUMENT)
        once the ticket is collected, or when the loaded library has no npow_ticket_sweep."""
        lib = self.engine.lib
        self._need(lib, "npow_ticket_sweep")
        if not self.ticket:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "the sweep ticket is collected")
        i = _SweepInfoStruct()
        i.size = ctypes.sizeof(_SweepInfoStruct)
        _check(lib.npow_ticket_sweep(self.ticket, ctypes.byref(i)), lib)
        return SweepInfo(bool(i.background), i.count, i.nonces_done, i.hits, i.launches, i.launches_cut, i.held_us,
                         bool(i.finished))

    def share(self) -> RangeShare:
        """The job's class (plain, background, shared), its launches, the launches cut, the time held out and the
        workgroups that moved to it inside running launches (npow_ticket_share); never waits for a GPU.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) once the ticket is collected, or when the loaded library has no
        npow_ticket_share."""
        return _range_share(self)

    def _collect_abandoned(self, lib) -> int:
        return lib.npow_wait_sweep(self.ticket, 10_000_000, None, 0, ctypes.byref(ctypes.c_uint64(0)), None)


class BestTicket(_JobTicket):
    """A submitted best job (npow_submit_best); wait() returns its BestResult once."""

    def wait(self, timeout: Optional[float] = None) -> Optional[BestResult]:
        """Block until the job ends (timeout None) or up to `timeout` seconds; None if it is still running then.
        The result unpacks as status, nonce, value, nonces_done.  NPOW_OK: the range's strongest nonce and its work
        value, nonces_done == count; NPOW_EXHAUSTED: nothing reached the floor; NPOW_CANCELLED: the best found so
        far (nonce None: none); an error raises."""
        if self.result is not None:
            return self.result
        lib = self.engine.lib
        nonce, value, done = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib.npow_wait_best(self.ticket, self._us(timeout), ctypes.byref(nonce), ctypes.byref(value),
                                ctypes.byref(done))
        if rc == NPOW_PENDING:
            return None
        self.cancel_token = None
        self.ticket = 0  # collected, whatever the status
        _check(rc, lib, ok=(NPOW_OK, NPOW_CANCELLED, NPOW_EXHAUSTED))
        found = rc == NPOW_OK or (rc == NPOW_CANCELLED and value.value != 0)
        self.result = BestResult(rc, nonce.value if found else None, value.value if found else None, done.value)
        return self.result

    def info(self) -> BestInfo:
        """The job's progress and best candidate so far (npow_ticket_best); never waits for a GPU.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) once the ticket is collected."""
        lib = self.engine.lib
        if not self.ticket:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "the best ticket is collected")
        i = _BestInfoStruct()
        i.size = ctypes.sizeof(_BestInfoStruct)
        _check(lib.npow_ticket_best(self.ticket, ctypes.byref(i)), lib)
        return BestInfo(bool(i.finished), i.count, i.nonces_done, i.nonce, i.value, i.launches, i.records,
                        i.records_max, i.room)

    def hold(self) -> BestHold:
        """The job's class, the launches cut and the time held out (npow_ticket_best_hold); never waits for a GPU.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) once the ticket is collected, or when the loaded library has no
        npow_ticket_best_hold."""
        lib = self.engine.lib
        self._need(lib, "npow_ticket_best_hold")
        if not self.ticket:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "the best ticket is collected")
        i = _BestHoldStruct()
        i.size = ctypes.sizeof(_BestHoldStruct)
        _check(lib.npow_ticket_best_hold(self.ticket, ctypes.byref(i)), lib)
        return BestHold(i.background, i.launches_cut, i.held_us)

    def share(self) -> RangeShare:
        """The job's class (plain, background, shared), its launches, the launches cut, the time held out and the
        workgroups that moved to it inside running launches (npow_ticket_share); never waits for a GPU.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) once the ticket is collected, or when the loaded library has no
        npow_ticket_share."""
        return _range_share(self)

    def _collect_abandoned(self, lib) -> int:
        n, v = ctypes.c_uint64(0), ctypes.c_uint64(0)
        return lib.npow_wait_best(self.ticket, 10_000_000, ctypes.byref(n), ctypes.byref(v), None)


class Engine:
    """Thin object wrapper over the C ABI (one per process is enough)."""

    def __init__(self, path: str = LIB_PATH, cpu_threads: int = 0) -> None:
        """cpu_threads > 0: add that many CPU worker threads as one more logical device after the GPUs
        (npow_config_cpu_threads; the reference work server's --cpu-threads).  npow_init is process-wide:
        asking for CPU threads once the engine is initialised in this process raises NanoPowError
        (NPOW_ERR_BAD_ARGUMENT), as npow_config_cpu_threads must precede npow_init."""
        self.lib = load(path)
        if cpu_threads:
            _check(self.lib.npow_config_cpu_threads(cpu_threads), self.lib)
        n = ctypes.c_int(0)
        _check(self.lib.npow_init(ctypes.byref(n)), self.lib)
        self.n_devices = n.value
        self.cpu_device = None  # logical id of the CPU workers' device, if any
        for d in range(self.n_devices):
            if self.stats(d).hip_device < 0:
                self.cpu_device = d
        self.gpu_mask = ((1 << self.n_devices) - 1) & ~(0 if self.cpu_device is None else 1 << self.cpu_device)

    # -- CPU helpers -------------------------------------------------------------------
    def work_value(self, root: bytes, nonce: int) -> int:
        return int(self.lib.npow_work_value(_root(root), nonce & M64))

    # -- GPU paths ---------------------------------------------------------------------
    def search(self, root: bytes, threshold: int, start: int = 0, device_mask: int = 0,
               max_nonces_per_device: int = 0, cancel: Optional[CancelToken] = None) -> SearchResult:
        nonce = ctypes.c_uint64(0)
        value = ctypes.c_uint64(0)
        done = ctypes.c_uint64(0)
        rc = self.lib.npow_search(_root(root), threshold & M64, start & M64, device_mask,
                                  max_nonces_per_device, cancel.address if cancel else None,
                                  ctypes.byref(nonce), ctypes.byref(value), ctypes.byref(done))
        _check(rc, self.lib, ok=(NPOW_OK, NPOW_CANCELLED, NPOW_EXHAUSTED))
        if rc == NPOW_OK:
            return SearchResult(rc, nonce.value, value.value, done.value)
        return SearchResult(rc, None, None, done.value)

    # -- work pool: asynchronous searches ---------------------------------------------------
    def submit(self, root: bytes, threshold: int, start: int = 0, device_mask: int = 0,
               max_nonces_per_device: int = 0, cancel: Optional[CancelToken] = None, weight: int = 1,
               background: bool = False, reserve: Optional[int] = None) -> "Ticket":
        """Queue a first-win search and return at once (npow_submit_weighted).  Keep `cancel` alive
        until the ticket's result has been collected (the Ticket holds a reference).
        weight (1, 2, 4 or 8): the search's share of each GPU among the live unbounded searches, weight /
        (sum of weights), and its place among the jobs waiting for admission (heaviest first).
        background=True (npow_submit_background; unbounded, weight 1): the search hashes only on workgroups no
        foreground search wants, until Ticket.promote lifts it.  NanoPowError(NPOW_ERR_BAD_ARGUMENT) when the loaded
        library has no npow_submit_background, and with max_nonces_per_device or a weight other than 1.
        reserve (npow_submit_reserve; unbounded): a reserve threshold in [NPOW_RESERVE_MIN, threshold] -- the search
        remembers the best nonce it passes whose value is at or above it (Ticket.reserve) and can be lowered to any
        level down to it while it runs (Ticket.relax).  NanoPowError(NPOW_ERR_BAD_ARGUMENT) when the loaded library
        has no npow_submit_reserve, and with max_nonces_per_device."""
        t = ctypes.c_uint64(0)
        if reserve is not None:
            _JobTicket._need(self.lib, "npow_submit_reserve")
            _JobTicket._u64("reserve", reserve)
            if not isinstance(weight, int) or isinstance(weight, bool) or not 0 <= weight <= 0xffffffff:
                raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "weight must be 1, 2, 4 or 8")
            if max_nonces_per_device or (background and weight != 1):
                raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "a search with a reserve is unbounded (and a background "
                                                          "one has weight 1)")
            _check(self.lib.npow_submit_reserve(_root(root), threshold & M64, reserve, start & M64, device_mask,
                                                cancel.address if cancel else None, weight, 1 if background else 0,
                                                ctypes.byref(t)), self.lib)
            tk = Ticket(self, t.value, cancel)
            tk.submitted_background = bool(background)
            return tk
        if background:
            _JobTicket._need(self.lib, "npow_submit_background")
            if max_nonces_per_device or weight != 1:
                raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "a background search is unbounded and has weight 1")
            _check(self.lib.npow_submit_background(_root(root), threshold & M64, start & M64, device_mask,
                                                   cancel.address if cancel else None, ctypes.byref(t)), self.lib)
            tk = Ticket(self, t.value, cancel)
            tk.submitted_background = True
            return tk
        args = (_root(root), threshold & M64, start & M64, device_mask, max_nonces_per_device,
                cancel.address if cancel else None)
        if hasattr(self.lib, "npow_submit_weighted"):
            if not isinstance(weight, int) or isinstance(weight, bool) or not 0 <= weight <= 0xffffffff:
                raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "weight must be 1, 2, 4 or 8")
            _check(self.lib.npow_submit_weighted(*args, weight, ctypes.byref(t)), self.lib)
        elif weight != 1:
            raise NanoPowError(NPOW_ERR_BAD_ARGUMENT, "the loaded libnanopow (ABI below 7) has no job weights")
        else:
            _check(self.lib.npow_submit(*args, ctypes.byref(t)), self.lib)
        return Ticket(self, t.value, cancel)

    def pool_config(self, max_active: int) -> None:
        _check(self.lib.npow_pool_config(max_active), self.lib)

    def pool_status(self) -> Tuple[int, int]:
        q, a = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(self.lib.npow_pool_status(ctypes.byref(q), ctypes.byref(a)), self.lib)
        return q.value, a.value

    def search_batch(self, roots: Sequence[bytes], thresholds: Sequence[int], device_mask: int = 0,
                     max_nonces_per_root: int = 0,
                     cancels: Optional[Sequence[Optional[CancelToken]]] = None) -> Tuple[List[SearchResult], int]:
        n = len(roots)
        if len(thresholds) != n:
            raise ValueError("roots and thresholds differ in length")
        rb = b"".join(_root(r) for r in roots)
        th = (ctypes.c_uint64 * n)(*[t & M64 for t in thresholds])
        nonces = (ctypes.c_uint64 * n)()
        values = (ctypes.c_uint64 * n)()
        status = (ctypes.c_int32 * n)()
        done = ctypes.c_uint64(0)
        cptr = None
        if cancels is not None:
            arr = (ctypes.c_void_p * n)(*[(c.address if c else None) for c in cancels])
            cptr = ctypes.addressof(arr)
        rc = self.lib.npow_search_batch(rb, ctypes.addressof(th), n, device_mask, max_nonces_per_root, cptr,
                                        ctypes.addressof(nonces), ctypes.addressof(values),
                                        ctypes.addressof(status), ctypes.byref(done))
        _check(rc, self.lib)
        out = []
        for i in range(n):
            if status[i] == NPOW_OK:
                out.append(SearchResult(NPOW_OK, nonces[i], values[i], 0))
            else:
                out.append(SearchResult(status[i], None, None, 0))
        return out, done.value

    def sweep_result(self, root: bytes, threshold: int, start: int, count: int, device_mask: int = 0,
                     cap: int = 1 << 16, cancel: Optional[CancelToken] = None) -> SweepResult:
        """npow_sweep with its status: a cancelled sweep returns status NPOW_CANCELLED and the
        hits found so far, never mistakable for the exact hit set of the range."""
        out = (ctypes.c_uint64 * max(cap, 1))()
        n = ctypes.c_uint64(0)
        rc = self.lib.npow_sweep(_root(root), threshold & M64, start & M64, count, device_mask,
                                 cancel.address if cancel else None, ctypes.addressof(out), cap,
                                 ctypes.byref(n))
        _check(rc, self.lib, ok=(NPOW_OK, NPOW_CANCELLED))
        return SweepResult(rc, list(out[: min(n.value, cap)]), n.value)

    def submit_sweep(self, root: bytes, threshold: int, start: int, count: int, device_mask: int = 0,
                     cancel: Optional[CancelToken] = None, cap: int = 1 << 16, *,
                     background: bool = False, shared: bool = False) -> SweepTicket:
        """Queue a sweep job and return at once (npow_submit_sweep): every hit of [start, start + count) enumerated
        inside the work pool's launches, beside the live searches, where sweep() takes the devices from the pool.
        SweepTicket.wait collects up to `cap` hits.  Keep `cancel` alive until then (the ticket holds a reference).
        background=True (npow_submit_sweep_background): each GPU hashes the job only while no foreground job wants
        it, and a search that arrives waits one short chunk; continuous foreground load starves the job.
        shared=True (npow_submit_sweep_shared): the job takes a weight-1 share of each GPU beside the searches and
        the workgroups they no longer want, is never held out, and a search that arrives waits one short chunk;
        SweepTicket.share tells the class and the moves.  ValueError with background=True as well.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) when the loaded library lacks the call."""
        if shared and background:
            raise ValueError("a range job is shared or background, not both")
        name = ("npow_submit_sweep_shared" if shared else
                "npow_submit_sweep_background" if background else "npow_submit_sweep")
        _JobTicket._need(self.lib, name)
        t = ctypes.c_uint64(0)
        _check(getattr(self.lib, name)(_root(root), threshold & M64, start & M64, count, device_mask,
                                       cancel.address if cancel else None, ctypes.byref(t)), self.lib)
        return SweepTicket(self, t.value, cancel, cap)

    def submit_best(self, root: bytes, start: int, count: int, floor: int = 0, device_mask: int = 0,
                    cancel: Optional[CancelToken] = None, background: bool = False,
                    shared: bool = False) -> BestTicket:
        """Queue a best job and return at once (npow_submit_best): the nonce of [start, start + count) with the
        highest work value, found inside the work pool's launches beside the live searches -- exact at any floor
        (only values >= floor are candidates; 0 allowed).  BestTicket.wait gives status, nonce, value, nonces_done.
        Keep `cancel` alive until then (the ticket holds a reference).
        background=True (npow_submit_best_background): each GPU hashes the job only while no foreground job wants
        it, and a search that arrives waits one short chunk; the best so far (BestTicket.info) survives every
        interruption; continuous foreground load starves the job.  BestTicket.hold tells what the class cost.
        shared=True (npow_submit_best_shared): the job takes a weight-1 share of each GPU beside the searches and
        the workgroups they no longer want, is never held out, and a search that arrives waits one short chunk;
        BestTicket.share tells the class and the moves.  ValueError with background=True as well.
        NanoPowError(NPOW_ERR_BAD_ARGUMENT) when the loaded library lacks the call."""
        if shared and background:
            raise ValueError("a range job is shared or background, not both")
        name = ("npow_submit_best_shared" if shared else
                "npow_submit_best_background" if background else "npow_submit_best")
        _JobTicket._need(self.lib, name)
        t = ctypes.c_uint64(0)
        _check(getattr(self.lib, name)(_root(root), floor & M64, start & M64, count, device_mask,
                                       cancel.address if cancel else None, ctypes.byref(t)), self.lib)
        return BestTicket(self, t.value, cancel)

    def sweep(self, root: bytes, threshold: int, start: int, count: int, device_mask: int = 0,
              cap: int = 1 << 16, cancel: Optional[CancelToken] = None) -> List[int]:
        """Every hit of [start, start + count) (exact).  Raises NanoPowError(NPOW_CANCELLED) if
        `cancel` stopped it (sweep_result() returns the partial hits with the status)."""
        r = self.sweep_result(root, threshold, start, count, device_mask, cap, cancel)
        if r.status != NPOW_OK:
            raise NanoPowError(r.status, f"sweep cancelled after {r.total} hits: the hit set is partial")
        return r.hits

    def values(self, root: bytes, start: int, count: int, device: int = 0, path: Optional[int] = None) -> List[int]:
        """Work values of start .. start + count - 1: npow_values (the search kernels' stream), or
        npow_values_path with an NPOW_PATH_* constant."""
        out = (ctypes.c_uint64 * max(count, 1))()
        if path is None:
            rc = self.lib.npow_values(device, _root(root), start & M64, count, ctypes.addressof(out))
        else:
            rc = self.lib.npow_values_path(device, _root(root), start & M64, count, path, ctypes.addressof(out))
        _check(rc, self.lib)
        return list(out[:count])

    def values_array(self, root: bytes, start: int, count: int, device: int = 0, path: int = NPOW_PATH_SEARCH):
        """The same as values() into a numpy uint64 array (large ranges)."""
        import numpy as np
        out = np.empty(max(count, 1), dtype=np.uint64)
        _check(self.lib.npow_values_path(device, _root(root), start & M64, count, path, out.ctypes.data), self.lib)
        return out[:count]

    def values_pairs(self, roots: Sequence[bytes], nonces: Sequence[int], device: int = 0) -> List[int]:
        n = len(nonces)
        if len(roots) != n:  # the library reads n * 32 root bytes
            raise ValueError(f"{len(roots)} roots for {n} nonces")
        rb = b"".join(_root(r) for r in roots)
        nn = (ctypes.c_uint64 * max(n, 1))(*[x & M64 for x in nonces])
        out = (ctypes.c_uint64 * max(n, 1))()
        _check(self.lib.npow_values_pairs(device, rb, ctypes.addressof(nn), n, ctypes.addressof(out)), self.lib)
        return list(out[:n])

    def set_tuning(self, iters_per_launch: int = 0, poll_interval: int = 0, blocks_per_cu: int = 0) -> None:
        _check(self.lib.npow_set_tuning(iters_per_launch, poll_interval, blocks_per_cu), self.lib)

    def set_pool_tuning(self, budget_us: Optional[int] = None, blocks_per_cu: int = 0) -> None:
        """Search launches: time budget in us (0 = off, None keeps) and workgroups per CU (0 keeps)."""
        _check(self.lib.npow_set_pool_tuning(0xffffffff if budget_us is None else budget_us, blocks_per_cu),
               self.lib)

    def set_launch_budget(self, budget_us: int) -> None:
        self.set_pool_tuning(budget_us=budget_us)

    def stats(self, device: int = 0) -> DeviceStats:
        s = DeviceStats()
        if hasattr(self.lib, "npow_device_stats_get_sized"):
            _check(self.lib.npow_device_stats_get_sized(device, ctypes.byref(s), ctypes.sizeof(s)), self.lib)
        else:
            _check(self.lib.npow_device_stats_get(device, ctypes.byref(s)), self.lib)
        return s

    def abi_version(self) -> int:
        return int(self.lib.npow_abi_version())

    def reset_stats(self, device: int = 0) -> None:
        _check(self.lib.npow_device_stats_reset(device), self.lib)

    def version(self) -> str:
        return self.lib.npow_version().decode()


_engine: Optional[Engine] = None
_engine_lock = threading.Lock()


def engine(cpu_threads: int = 0) -> Engine:
    """Process-wide engine (initialised on first use; raises if no GPU).  cpu_threads: CPU workers
    beside the GPUs (Engine), honoured by the first call only."""
    global _engine
    with _engine_lock:
        if _engine is None:
            _engine = Engine(cpu_threads=cpu_threads)
        return _engine
