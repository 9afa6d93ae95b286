"""bench.py's plain run and `--dump-outputs`: a plain run times its steps and prints the headline
line without the side measurements (those need `--full`), and the dumped arrays are what the last
timed check returned, here on 2pc N=5 against the CPU oracle (one GPU, and two ranks on this GPU
over the shared-memory transport, where the deferred discovery paths are built collectively)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import TWO_PHASE, OracleRun

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5
PROPERTIES = ["abort agreement", "commit agreement", "consistent"]  # 2pc's properties() order
SIDE = ("roofline", "levels", "no_hint", "config4", "replicas", "cpu_baseline")


@pytest.fixture(scope="module")
def oracle():
    o = OracleRun(TWO_PHASE, [N])
    lengths = [-1 if o.discovery_actions(p) is None else len(o.discovery_actions(p)) for p in PROPERTIES]
    return [o.unique_state_count, o.state_count, o.max_depth], lengths


def bench(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rm-count", str(N)] + args,
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def check_dump(d, oracle):
    counts, lengths = oracle
    assert sorted(os.listdir(d)) == ["counts.npy", "discovery_lengths.npy"]
    got_counts, got_lengths = np.load(os.path.join(d, "counts.npy")), np.load(os.path.join(d, "discovery_lengths.npy"))
    assert got_counts.dtype == np.float64 and got_lengths.dtype == np.float64
    assert got_counts.tolist() == counts
    assert got_lengths.tolist() == lengths


def test_plain_run_and_dump(tmp_path, oracle):
    line = bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "unique states/s" and line["dtype"] == "u64"
    # value and ms_per_step describe the same timed steps
    assert line["value"] == pytest.approx(oracle[0][0] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in SIDE if k in line]
    check_dump(tmp_path / "out", oracle)


def test_two_ranks_dump(tmp_path, oracle):
    line = bench(["--gpus", "2", "--comm", "shm", "--steps", "2", "--warmup", "1",
                  "--dump-outputs", str(tmp_path / "out")])
    assert line["n_gpus"] == 2 and line["config"]["comm"] == "shm"
    assert not [k for k in SIDE if k in line]
    check_dump(tmp_path / "out", oracle)
