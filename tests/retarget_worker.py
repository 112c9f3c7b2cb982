"""Child process of tests/test_gpu_retarget.py (the engine reads its environment once).  One JSON line on stdout.

  partitions  NANOPOW_VIRTUAL_DEVICES=2: one search split over both CU partitions (device_mask 3) in launches that
              outlast it, retargeted 5 ms after its submit, while both devices hash it.
  blind       NANOPOW_FAULT_RETARGET_BLIND=1 with NANOPOW_TEST_HOOKS=1: the solo search of the fixture root from S,
              retargeted while its launch runs; no floor record is written, so the launch publishes its first hit
              under the old threshold and the host has to refuse it (stale_wins) and re-arm the search."""
import hashlib
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402

OLD, NEW = 0xfffffff800000000, 0xfffffffe00000000
FIXTURE_ROOT = "2f843c5852a3950673ee3fce36f431b3656c0edbb0dbfe7692753660ae88e712"
S = 0x846e097c0


def value(root, nonce):
    return int.from_bytes(hashlib.blake2b(nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")


def device(st):
    return {k: getattr(st, k) for k in ("launches", "yields", "invalid_work", "dead", "early_mismatches",
                                        "stale_missing")}


def main(mode):
    eng = _lib.Engine()
    n = 2 if mode == "partitions" else 1
    if mode == "partitions":
        assert eng.n_devices == 2 == int(os.environ["NANOPOW_VIRTUAL_DEVICES"])
        root = bytes(random.Random(95).getrandbits(8) for _ in range(32))
        start, mask = 0, 3
    else:
        root, start, mask = bytes.fromhex(FIXTURE_ROOT), S, 1
    eng.set_pool_tuning(budget_us=600000)  # one launch per device outlasts the search
    eng.set_tuning(65536)
    before = [device(eng.stats(d)) for d in range(n)]
    t = eng.submit(root, OLD, start=start, device_mask=mask)
    time.sleep(0.005)  # (its launches are running)
    held = t.retarget(NEW)
    info = t.wait_info(60)
    after = [device(eng.stats(d)) for d in range(n)]
    print(json.dumps({"held": held, "status": info.status, "nonce": info.nonce, "value": info.value,
                      "hashlib": value(root, info.nonce) if info.status == _lib.NPOW_OK else None,
                      "retargets": info.retargets, "stale_hits": info.stale_hits, "stale_wins": info.stale_wins,
                      "n_devices": info.n_devices, "before": before, "after": after}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
