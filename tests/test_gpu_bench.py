"""`bench.py` without `--full`: the result line holds the headline and nothing measured beside it, `--steps` sets the timed
steps, and `--dump-outputs` writes the last timed step's outputs, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--steps", "3", "--warmup", "2", "--per-gpu-batch", "16"]


def _bench(out_dir):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a
    assert a["unit"] == "spectrograms/s" and a["higher_is_better"] is True and a["n_gpus"] == 1
    assert a["steps"] == 3 and a["warmup"] == 2 and a["value"] > 0
    assert abs(a["value"] - 16 * 1e3 / a["ms_per_step"]) <= 1e-3 * a["value"]
    for k in ("roofline", "strong_scaling", "loader_path", "shotgun_path", "cpu_baseline"):
        assert k not in a
    assert "exposed_comm_ms_per_step" not in a["dist"]

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "grad.fc1.weight.npy", "param.fc8.bias.npy", "buffer.bn1.running_mean.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x))
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-7, err_msg=n)
        total += x.nbytes
    assert total <= 64 << 20
    loss = float(np.load(tmp_path / "a" / "loss.npy")[0])
    assert abs(loss / 16 - a["elbo_last_batch_mean"]) <= 1e-3 + 1e-6 * abs(loss)
