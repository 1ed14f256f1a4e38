"""CPU: bench.py's command line -- --steps is validated, and --dump-outputs writes the timed path's results as float32 .npy files."""
import os
import sys

import numpy as np
import pytest
import torch

import bench
import brainxai


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_steps_and_dump_dir_are_parsed(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out")
    assert (args.steps, args.warmup, args.dump_outputs) == (7, 2, "out")
    assert _parse(monkeypatch).dump_outputs is None


def test_zero_steps_is_refused(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_every_result_as_float32(tmp_path):
    model = brainxai.build_multimodal(19, 2000, 4, dropout=0.5, compute_dtype=torch.bfloat16)
    loss = torch.tensor(0.25)
    out = torch.log_softmax(torch.randn(64, 6), 1).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "dump"), loss, out, model)
    names = set(os.listdir(tmp_path / "dump"))
    params = dict(model.named_parameters())
    buffers = {n: b for n, b in model.named_buffers() if b.is_floating_point()}
    assert names == {"loss.npy", "log_probs.npy"} | {f"param.{n}.npy" for n in params} | {f"buffer.{n}.npy" for n in buffers}
    total = 0
    for name in names:
        a = np.load(tmp_path / "dump" / name)
        assert a.dtype == np.float32, name
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "dump" / "loss.npy") == np.float32(0.25)
    np.testing.assert_array_equal(np.load(tmp_path / "dump" / "log_probs.npy"), out.float().numpy())
    w = "spectrogram_model.block1.conv1.weight"
    np.testing.assert_array_equal(np.load(tmp_path / "dump" / f"param.{w}.npy"), params[w].detach().numpy())
