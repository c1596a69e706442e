"""bench.py's command line and --dump-outputs writer, without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import srfrd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_loss_and_every_parameter_as_float32(tmp_path):
    torch.manual_seed(0)
    model = srfrd_amd.SASRec(100, 20, 50, 0.5, 2, 1, "cpu")
    loss = torch.tensor([1.25])
    n_bytes = bench.dump_outputs(str(tmp_path / "out"), loss, model)
    sd = model.state_dict()
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted([k + ".npy" for k in sd] + ["loss.npy"])
    assert n_bytes == 4 + sum(v.numel() * 4 for v in sd.values())
    for k, v in sd.items():
        a = np.load(tmp_path / "out" / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.numpy())
    assert np.load(tmp_path / "out" / "loss.npy").tolist() == [1.25]


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    model = srfrd_amd.SASRec(100, 20, 50, 0.5, 2, 1, "cpu")
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "out"), torch.zeros(1), model)
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--dump-outputs", "d", "--predict"], ["--dump-outputs", "d", "--workload", "C4"]])
def test_bad_arguments_are_refused_before_any_gpu_work(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr
    assert "error:" in r.stderr
