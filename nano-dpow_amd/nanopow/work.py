"""Field rules of the nano-work-server JSON surface (hashes, work, thresholds, multipliers).

The DPoW client sends these fields verbatim from MQTT (client/dpow_client.py:63-75,
docs/specification.md:19-31): the hash as 64 hex characters in any case, the
difficulty as 16 hex characters.  Error strings follow the reference work
server's (client/bin/windows/nano-work-server.exe @1677928..1679336).
The multiplier formulas are the DPoW server's (server/dpow_server.py:250-255,
275-280, 296-305): multiplier = (2^64 - base) / (2^64 - d).
"""
from __future__ import annotations

import re
from typing import Any, Dict, Tuple

M64 = (1 << 64) - 1
TWO64 = 1 << 64

# Epoch-2 thresholds (the live network's send/change and receive thresholds).
SEND_THRESHOLD = 0xfffffff800000000
RECEIVE_THRESHOLD = 0xfffffe0000000000
# Base threshold the multiplier is quoted against (nano-work-server.exe @1681900:
# "Configured for the live network with threshold fffffff800000000").
DEFAULT_BASE = SEND_THRESHOLD
# The lowest reserve difficulty (include/nanopow.h NPOW_RESERVE_MIN; --reserve-difficulty, a request's "reserve")
RESERVE_MIN = 0xfffff00000000000

SUPPORTED = "Supported commands: work_generate, work_cancel, work_validate, benchmark, status"

# 1..16 hex digits and nothing else: int(x, 16) alone also takes "-1", "+f", "0x1f", " ff", "f_f"
_HEX64 = re.compile(r"[0-9a-fA-F]{1,16}")


class RequestError(Exception):
    """A request the server answers with {"error": ..., "hint": ...} (HTTP 200)."""

    def __init__(self, error: str, hint: str = "") -> None:
        super().__init__(error)
        self.error = error
        self.hint = hint

    def reply(self) -> Dict[str, str]:
        out = {"error": self.error}
        if self.hint:
            out["hint"] = self.hint
        return out


def parse_hash(req: Dict[str, Any]) -> bytes:
    if "hash" not in req:
        raise RequestError("Failed to deserialize JSON", "Hash field missing")
    h = req["hash"]
    if not isinstance(h, str):
        raise RequestError("Bad block hash", "Expecting a hex string")
    if h == "":
        raise RequestError("Bad block hash", "Hash is empty. Expecting a hex string")
    try:
        raw = bytes.fromhex(h)
    except ValueError:
        raise RequestError("Bad block hash", "Expecting a hex string") from None
    if len(raw) < 32:
        raise RequestError("Bad block hash", "Hash is too short (should be 32 bytes)")
    if len(raw) > 32:
        raise RequestError("Bad block hash", "Hash is too long (should be 32 bytes)")
    return raw


def parse_work(req: Dict[str, Any]) -> int:
    if "work" not in req:
        raise RequestError("Failed to deserialize JSON", "Work field missing")
    w = req["work"]
    if not isinstance(w, str):
        raise RequestError("Bad work", "Expecting a hex string for work")
    if w == "":
        raise RequestError("Bad work", "Work is empty. Expecting a hex string")
    if len(w) > 16:
        raise RequestError("Bad work", "Work is too long (should be 8 bytes)")
    if not _HEX64.fullmatch(w):
        raise RequestError("Bad work", "Expecting a hex string for work")
    return int(w, 16)


def parse_threshold(s: Any) -> int:
    if not isinstance(s, str):
        raise RequestError("Bad difficulty", "Expecting a hex string for difficulty")
    if not _HEX64.fullmatch(s):
        raise RequestError("Bad difficulty",
                           "Threshold not a valid unsigned long (u64). Example: 'ffffffc000000000'")
    return int(s, 16)


def parse_multiplier(x: Any) -> float:
    try:
        m = float(x)
    except (TypeError, ValueError):
        raise RequestError("Bad multiplier", "Expecting a positive number for multiplier") from None
    if not (m > 0.0) or m != m or m == float("inf"):
        raise RequestError("Bad multiplier", "Expecting a positive number for multiplier")
    return m


def from_multiplier(multiplier: float, base: int = DEFAULT_BASE) -> int:
    """d = 2^64 - (2^64 - base) / multiplier  (dpow_server.py:275-280)."""
    d = TWO64 - int((TWO64 - base) / multiplier)
    return max(0, min(M64, d))


def to_multiplier(difficulty: int, base: int = DEFAULT_BASE) -> float:
    """(2^64 - base) / (2^64 - d)  (dpow_server.py:250-255, 296-305)."""
    return float(TWO64 - base) / float(TWO64 - difficulty)


def requested_threshold(req: Dict[str, Any], base: int) -> int:
    """difficulty, else multiplier x base, else the base threshold."""
    if req.get("difficulty") is not None:
        return parse_threshold(req["difficulty"])
    if req.get("multiplier") is not None:
        return from_multiplier(parse_multiplier(req["multiplier"]), base)
    return base


def parse_reserve(req: Dict[str, Any], minimum: int):
    """The optional ``"reserve"`` of a work_generate request (16 hex digits like a difficulty; this server's
    extension): the reserve difficulty of the request's search (npow_submit_reserve), at least `minimum`.  None when
    absent."""
    r = req.get("reserve")
    if r is None:
        return None
    bad = RequestError("Bad reserve", f"Expecting a hex difficulty of at least {minimum:016x}")
    if not isinstance(r, str) or not _HEX64.fullmatch(r):
        raise bad
    if int(r, 16) < minimum:
        raise bad
    return int(r, 16)


WEIGHTS = (1, 2, 4, 8)


def parse_background(req: Dict[str, Any]) -> bool:
    """The optional ``"background"`` of a work_generate or work_best request (a JSON boolean; this server's
    extension): the search hashes only on what no foreground search wants (npow_submit_background), the best job only
    while no foreground job wants the GPU (npow_submit_best_background).  False when absent."""
    b = req.get("background")
    if b is None:
        return False
    if not isinstance(b, bool):
        raise RequestError("Bad background", "Expecting true or false")
    return b


def parse_shared(req: Dict[str, Any]) -> bool:
    """The optional ``"shared"`` of a work_best request (a JSON boolean; this server's extension): the best job takes a
    weight-1 share of each GPU beside the searches and is never held out (npow_submit_best_shared).  False when
    absent; together with ``"background": true`` the request is refused."""
    s = req.get("shared")
    if s is None:
        return False
    if not isinstance(s, bool):
        raise RequestError("Bad shared", "Expecting true or false")
    if s and parse_background(req):
        raise RequestError("Bad shared", "Expecting shared or background, not both")
    return s


def parse_weight(req: Dict[str, Any]) -> int:
    """The optional ``"weight"`` of a work_generate or work_promote request (an integer or a decimal string; this server's
    extension -- the reference has no such field): the request's share of each GPU among the searches in
    flight, 1 when absent."""
    w = req.get("weight")
    if w is None:
        return 1
    bad = RequestError("Bad weight", "Expecting 1, 2, 4 or 8")
    if isinstance(w, bool) or not isinstance(w, (int, str)):
        raise bad
    if isinstance(w, str):
        if not (w.isascii() and w.isdigit()):
            raise bad
        w = int(w)
    if w not in WEIGHTS:
        raise bad
    return w


def fmt_u64(x: int) -> str:
    return f"{x & M64:016x}"


def fmt_multiplier(m: float) -> str:
    return repr(float(m))


def parse_count(req: Dict[str, Any]) -> int:
    if "count" not in req:
        raise RequestError("Failed to deserialize JSON", "count field missing")
    try:
        c = int(req["count"])
    except (TypeError, ValueError):
        raise RequestError("Bad count", "Expecting a positive number for count") from None
    if c <= 0:
        raise RequestError("Bad count", "Expecting a positive number for count")
    return c


BEST_MAX_COUNT = 1 << 40  # nonces one work_best request may ask for (~40 s of one GPU)


def parse_best_count(req: Dict[str, Any]) -> int:
    """The ``"count"`` of a work_best request (an integer or a decimal string; this server's extension): the nonces
    to hash, 1 .. 2^40."""
    if "count" not in req:
        raise RequestError("Failed to deserialize JSON", "count field missing")
    c = req["count"]
    bad = RequestError("Bad count", f"Expecting a positive integer of at most {BEST_MAX_COUNT} for count")
    if isinstance(c, bool) or not isinstance(c, (int, str)):
        raise bad
    if isinstance(c, str):
        if not (c.isascii() and c.isdigit()) or len(c) > 20:
            raise bad
        c = int(c)
    if not 0 < c <= BEST_MAX_COUNT:
        raise bad
    return c


def parse_start(req: Dict[str, Any]):
    """The optional ``"start"`` of a work_best request: the range's first nonce, 16 hex digits like a work value.
    None when absent."""
    s = req.get("start")
    if s is None:
        return None
    if not isinstance(s, str) or len(s) != 16 or not _HEX64.fullmatch(s):
        raise RequestError("Bad start", "Expecting 16 hex digits for start")
    return int(s, 16)


def parse_gpu_spec(spec: str) -> Tuple[int, int, int]:
    """``PLATFORM:DEVICE[:THREADS]`` (nano-work-server.exe @1681064).  HIP has a single
    platform, so PLATFORM is accepted and ignored; THREADS (nonces per launch,
    default 1048576) becomes a lower bound on the launch chunk (__main__.apply_threads)."""
    parts = spec.split(":")
    if len(parts) not in (2, 3):
        raise ValueError(f"bad --gpu spec {spec!r}: expected PLATFORM:DEVICE[:THREADS]")
    platform, device = int(parts[0]), int(parts[1])
    threads = int(parts[2]) if len(parts) == 3 else 1048576
    if platform < 0 or device < 0 or threads <= 0:
        raise ValueError(f"bad --gpu spec {spec!r}")
    return platform, device, threads
