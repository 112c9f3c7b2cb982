"""bench.py's plain run on the GPU: the driver's command with a few steps, in a process of its own as the driver
starts it -- the result line's headline fields, none of the --full legs, and --dump-outputs' files.
Run on an MI355X: ``pytest -m gpu``.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
SEND = 0xfffffff800000000


def test_plain_run_with_dumped_outputs(tmp_path):
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["n_ttw"] == 3 and line["warmup"] == 1
    assert line["unit"] == "Gnonce/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["device_check"]["ok"]
    # the timed region held the 3 searches and nothing else: its kernels' nonces are the searches' nonces
    assert line["device_check"]["kernel_nonces"] == line["device_check"]["search_nonces"] > 0
    assert line["cpu_baseline"] is None
    for k in ("ttw_c_abi_ms", "steady_state", "http_ttw_ms", "node_ttw_8x_regime"):
        assert k not in line
    got = {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert sorted(got) == ["status.npy", "work_value.npy", "work_value_rehashed.npy"]
    assert all(a.dtype == np.float64 and a.shape == (1,) for a in got.values())
    assert got["status.npy"][0] == 0.0
    # the engine's value of its nonce is hashlib's (bench.dump_outputs re-hashes the nonce on the CPU), and it is work
    assert got["work_value.npy"][0] == got["work_value_rehashed.npy"][0] >= float(SEND)


def test_full_run_adds_its_legs():
    """--full with its legs sized down (the CPU baseline and the regime child off: each takes ten seconds or more)."""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--latency-searches", "20", "--http-requests", "5", "--regime-searches", "0"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["n_ttw"] == 3 and line["device_check"]["ok"]
    assert line["ttw_c_abi_ms"]["n"] == 20 and line["http_ttw_ms"]["n"] == 5
    assert line["value_steady"] == line["steady_state"]["value"] > 0
    assert line["cpu_baseline"] is None and "node_ttw_8x_regime" not in line
