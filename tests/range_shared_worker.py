"""Child process of tests/test_gpu_range_shared.py: one shared sweep job split over two CU partitions.
Run with NANOPOW_VIRTUAL_DEVICES=2 (two logical devices over the one physical GPU, each with its own stream, hit
records, claim and move counters and worker): npow_submit_sweep_shared of the first 2^24 fixture of
tests/golden/sweeps_small.json over both devices, beside an unending weight-8 search on both, so that each
partition's tables are map-dealt.  The merged hit set must equal the fixture's and both devices must have hashed.
Prints one JSON line; exits non-zero on any mismatch."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nano-dpow_amd"))

from nanopow import _lib  # noqa: E402


def main():
    eng = _lib.Engine()
    G = eng.n_devices
    assert G == int(os.environ["NANOPOW_VIRTUAL_DEVICES"]) == 2, G
    with open(os.path.join(HERE, "golden", "sweeps_small.json")) as f:
        c = json.load(f)["cases"][-3]
    assert c["count"] == 1 << 24
    for d in range(G):
        eng.reset_stats(d)
    tok = _lib.CancelToken()
    search = eng.submit(bytes([0x79]) * 32, (1 << 64) - 1, device_mask=0, cancel=tok, weight=8)
    try:
        t = eng.submit_sweep(bytes.fromhex(c["root"]), int(c["threshold"], 16), int(c["start"], 16), c["count"],
                             device_mask=0, shared=True)
        deadline = time.time() + 60
        while not t.info().finished and time.time() < deadline:
            time.sleep(0.001)
        i, s = t.info(), t.share()
        r = t.wait(60)
    finally:
        tok.set()
    assert search.wait(30).status == _lib.NPOW_CANCELLED
    assert r is not None and r.status == _lib.NPOW_OK, r
    assert [f"{h:016x}" for h in r.hits] == c["hits"], (len(r.hits), len(c["hits"]))
    assert r.total == len(c["hits"]) and r.nonces_done == c["count"]
    assert s.klass == _lib.RANGE_SHARED and s.held_us == 0, s
    per = [eng.stats(d).nonces for d in range(G)]
    print(json.dumps({"ok": True, "devices": G, "hits": len(r.hits), "nonces_done": r.nonces_done,
                      "nonces_per_device": per, "launches": i.launches, "launches_cut": i.launches_cut,
                      "moves": s.moves,
                      "affinity": [sum(eng.stats(d).affinity_checks for d in range(G)),
                                   sum(eng.stats(d).affinity_failures for d in range(G))]}), flush=True)


if __name__ == "__main__":
    main()
