"""bench.py host logic that needs no GPU: argument defaults (>= 100 timed / >= 20 warm-up steps), the
self-launch of N ranks when `--gpus N` is given without a launcher and the writer of `--dump-outputs`."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_defaults_follow_the_measurement_plan():
    a = bench.parse([])
    assert a.gpus == 1 and a.steps >= 100 and a.warmup >= 20 and a.batch == 256 and a.z_dim == 32
    assert a.global_batch == 1024 and a.backend == "nccl"
    assert not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    assert bench.parse(["--per-gpu-batch", "128"]).batch == 128 and bench.parse(["--batch", "64"]).batch == 64


def test_gpus_n_without_launcher_starts_n_ranks(monkeypatch):
    seen = {}

    class Res:
        returncode = 0
        stdout = 'rank noise\n{"metric": "x", "n_gpus": 4}\n'

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["cmd"], seen["env"] = cmd, env
        return Res()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and os.path.basename(cmd[-5]) == "bench.py"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_dump_outputs_writes_every_tensor_within_the_budget(tmp_path):
    import numpy as np
    import torch
    from ava_amd.vae import VAE
    torch.manual_seed(1234)
    model = VAE(z_dim=32, device_name="cpu")
    model._loss_buf[0] = 12345.5
    for p in model.parameters():                       # each gradient numbers its entries (exact in fp32: < 2**24)
        p.grad.copy_(torch.arange(p.numel(), dtype=torch.float32).view(p.shape))
    nbytes = bench.dump_outputs(model, str(tmp_path / "a"))
    bench.dump_outputs(model, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    params = dict(model.named_parameters())
    assert len(names) == 1 + 2 * len(params) + len(dict(model.named_buffers()))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total == nbytes <= 64 << 20
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [12345.5]
    for name, p in params.items():
        g = np.load(tmp_path / "a" / ("grad.%s.npy" % name))
        w = np.load(tmp_path / "a" / ("param.%s.npy" % name))
        if p.numel() <= bench.DUMP_SAMPLE:
            assert np.array_equal(w.reshape(p.shape), p.detach().numpy())
            assert np.array_equal(g, np.arange(p.numel(), dtype=np.float32))
        else:                               # a sample: distinct flat entries in increasing order
            assert w.size == g.size == bench.DUMP_SAMPLE and np.all(np.diff(g) > 0)
            assert np.array_equal(w, p.detach().reshape(-1).numpy()[g.astype(np.int64)])
