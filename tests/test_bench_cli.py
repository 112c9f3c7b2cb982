"""bench.py's command line on the oracle stand-in engine (host logic; CPU): a plain run does the warmup and the
timed steps and nothing else, --full adds the other legs, --dump-outputs writes the last timed search's result."""
import hashlib
import json
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fake_engine import OracleEngine  # noqa: E402

THR = 0xfff0000000000000  # 2^12 nonces expected: the stand-in hashes on the CPU
LEGS = ("cpu_baseline", "_http_ttw", "regime_child")


@pytest.fixture
def run_bench(monkeypatch, capsys):
    """bench.main() with argv on a fresh OracleEngine at THR; the legs beside the headline are stubs that count
    their calls.  Returns (rc, result line, engine, calls)."""
    def run(*argv):
        import nanopow
        eng = OracleEngine(count_stats=True)
        calls = {k: 0 for k in LEGS}

        def stub(name, out):
            def f(*a, **kw):
                calls[name] += 1
                return out
            return f
        monkeypatch.setattr(nanopow, "engine", lambda *a, **kw: eng)
        monkeypatch.setattr(bench, "SEND", THR)
        monkeypatch.setattr(bench, "cpu_baseline", stub("cpu_baseline", {"value": 0.04, "kind": "reference"}))
        monkeypatch.setattr(bench, "_http_ttw", stub("_http_ttw", [0.001, 0.002]))
        monkeypatch.setattr(bench, "regime_child", stub("regime_child", {"devices": 8}))
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        rc = bench.main()
        out = capsys.readouterr().out.strip().splitlines()
        assert len(out) == 1, out
        return rc, json.loads(out[0]), eng, calls
    return run


def test_plain_run_times_the_steps_and_nothing_else(run_bench):
    rc, line, eng, calls = run_bench("--gpus", "1", "--steps", "7", "--warmup", "2")
    assert rc == 0
    assert len(eng.calls) == 2 + 7  # the warmup and the timed searches: no other search
    assert calls == {k: 0 for k in LEGS}
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_ttw"] == 7
    assert line["metric"] == bench.METRIC and line["unit"] == "Gnonce/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u64" and line["value"] > 0 and line["ms_per_step"] > 0
    # ms_per_step is the timed wall time per step, value the timed nonces over that time
    timed_nonces = eng.stats(0).nonces  # reset after the warmup, and nothing ran after the timed steps
    assert line["value"] == pytest.approx(timed_nonces / (line["ms_per_step"] * 1e-3 * 7) / 1e9, rel=1e-3, abs=1e-4)
    assert line["cpu_baseline"] is None
    for k in ("ttw_c_abi_ms", "steady_state", "http_ttw_ms", "node_ttw_8x_regime", "node_ttw_ms"):
        assert k not in line


def test_full_run_adds_the_other_legs(run_bench):
    rc, line, eng, calls = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                                     "--latency-searches", "0")
    assert rc == 0
    assert calls == {k: 1 for k in LEGS}
    assert line["steps"] == 3 and line["n_ttw"] == 3
    assert line["cpu_baseline"]["kind"] == "reference"
    assert line["http_ttw_ms"]["n"] == 2 and line["node_ttw_8x_regime"] == {"devices": 8}


def test_full_run_legs_can_be_switched_off(run_bench):
    rc, line, eng, calls = run_bench("--steps", "2", "--warmup", "0", "--full", "--no-cpu-baseline",
                                     "--latency-searches", "0", "--http-requests", "0", "--regime-searches", "0")
    assert rc == 0 and calls == {k: 0 for k in LEGS} and len(eng.calls) == 2


def test_dump_outputs_writes_the_last_timed_search(run_bench, tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    rc, line, eng, _ = run_bench("--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs", str(d1))
    assert rc == 0
    got = {p.name: np.load(p) for p in d1.iterdir()}
    assert sorted(got) == ["status.npy", "work_value.npy", "work_value_rehashed.npy"]
    assert all(a.dtype == np.float64 and a.shape == (1,) for a in got.values())
    # the last timed step is search 3 of rank 0's roots: its own root and start nonce, nothing else after it
    root, thr, start = eng.calls[-1]
    assert (root, thr, start) == (bench.bench_root(1_000_003), THR, bench.bench_start(1_000_003))
    found = eng.search(root, THR, start)
    assert got["status.npy"][0] == 0.0
    assert got["work_value.npy"][0] == float(found.value) >= float(THR)
    want = int.from_bytes(hashlib.blake2b(found.nonce.to_bytes(8, "little") + root, digest_size=8).digest(), "little")
    assert got["work_value_rehashed.npy"][0] == float(want) == got["work_value.npy"][0]
    # the same arguments: the same inputs, search for search, and the same files
    rc, _, eng2, _ = run_bench("--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs", str(d2))
    assert rc == 0 and eng2.calls == eng.calls[:-1]
    for name, a in got.items():
        assert np.array_equal(np.load(d2 / name), a)


def test_dump_outputs_tells_a_wrong_nonce():
    """work_value_rehashed is the CPU's value of the returned nonce: an engine that returned a nonce which is not
    the work it claims shows as work_value != work_value_rehashed."""
    import tempfile
    root = bench.bench_root(5)
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, root, 0, 12345, 0xfffffff912345678)
        v, r = (np.load(f"{d}/{n}.npy")[0] for n in ("work_value", "work_value_rehashed"))
    assert v == float(0xfffffff912345678) and r != v


@pytest.mark.parametrize("argv", [("--gpus", "2"), ("--workload", "sweep")])
def test_dump_outputs_is_for_the_one_gpu_search(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv, "--dump-outputs", "unused"])
    with pytest.raises(SystemExit):
        bench.main()
