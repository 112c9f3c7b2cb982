"""Child process of tests/test_gpu_reserve.py (the engine reads its environment once).  One JSON line on stdout.

NANOPOW_VIRTUAL_DEVICES=2: the fixture root is searched from S over both CU partitions (device_mask 3) at a threshold
nothing meets, with fffffff800000000 as its reserve, in launches that outlast it.  Once either device's reserve has
reached the host the search is relaxed to the reserve threshold: answered at once, and both devices' final counts
arrive."""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

OLD = 0xfffffff800000000
M64 = (1 << 64) - 1
FIXTURE_ROOT = "2f843c5852a3950673ee3fce36f431b3656c0edbb0dbfe7692753660ae88e712"
S = 0x846e097c0


def value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


def device(st):
    return {k: getattr(st, k) for k in ("launches", "yields", "invalid_work", "dead", "early_mismatches",
                                        "stale_missing")}


def main():
    eng = _lib.Engine()
    assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
    root = bytes.fromhex(FIXTURE_ROOT)
    eng.set_pool_tuning(budget_us=600000)  # one launch per device outlasts the search
    eng.set_tuning(65536)
    t = eng.submit(root, M64, start=S, device_mask=3, reserve=OLD)
    try:
        deadline = time.monotonic() + 10
        r = None
        while r is None and time.monotonic() < deadline:
            r = t.reserve()
            if r is None:
                time.sleep(0.0005)
        assert r is not None, "no reserve within 10 s"
        held = t.reserve_info()
        answered = t.relax(OLD)
        res = t.wait_result(0)
        ri = t.reserve_info()
        info = t.wait_info(60)
    finally:
        if t.result is None:
            t.cancel()
            t.wait(30)
    after = [device(eng.stats(d)) for d in range(2)]
    print(json.dumps({"reserve_nonce": r.nonce, "reserve_value": r.value, "reserve_hashlib": value(root, r.nonce),
                      "reserve_device": held.device, "answered": answered,
                      "result_at_once": res is not None and res.status == _lib.NPOW_OK,
                      "status": info.status, "nonce": info.nonce, "value": info.value,
                      "hashlib": value(root, info.nonce) if info.status == _lib.NPOW_OK else None,
                      "info_answered": ri.answered, "relaxes": ri.relaxes, "nonces_done": info.nonces_done,
                      "n_devices": info.n_devices, "after": after}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
