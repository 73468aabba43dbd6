"""bench.py on one GPU: a plain run prints the headline line and nothing that needs runs of its own, --full adds `roofline` and
`cpu_baseline`, and --dump-outputs writes the last timed step's results from seeded inputs (the same in both runs, so they agree)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "tiny"] + list(extra)
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _dumped(d):
    names = sorted(os.listdir(d))
    arrays = {n[:-4]: np.load(os.path.join(d, n), allow_pickle=False) for n in names}
    assert all(n.endswith(".npy") for n in names), names
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    assert sum(os.path.getsize(os.path.join(d, n)) for n in names) <= 64 << 20
    return arrays


def test_bench_plain_full_and_dumped_outputs(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["losses_finite"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert k in plain, k
    assert "roofline" not in plain and "cpu_baseline" not in plain
    full = _bench("--full", "--dump-outputs", str(tmp_path / "full"))
    assert full["roofline"]["launches_per_step"] > 0 and full["cpu_baseline"].get("value"), (full["roofline"], full["cpu_baseline"])
    a, b = _dumped(tmp_path / "plain"), _dumped(tmp_path / "full")
    assert sorted(a) == sorted(b) and "state_sample" in a
    assert {"loss_" + k for k in plain["last_losses"]} == set(a) - {"state_sample"}
    for k in plain["last_losses"]:
        assert abs(float(a["loss_" + k][0]) - plain["last_losses"][k]) < 1e-5 * max(1.0, abs(plain["last_losses"][k])), k
    # same seeded inputs and the same number of steps before the dump: equal up to the order of fp32 sums.  Where a gradient is ~0, Adam
    # turns that last-bit noise into a step of up to ~3 lr either way: over the ~21 steps here the learning rates sum to 1e-5, hence atol
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-3, atol=1e-4, err_msg=k)
