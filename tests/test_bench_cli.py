"""CPU: bench.py's command line -- a plain run measures the headline only, `--full` adds the extra measurements -- and the files of
`--dump-outputs` (float32, a fixed parameter sample, identical for identical inputs)."""
import sys

import numpy as np
import pytest
import torch

import bench


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_skips_the_extra_measurements(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_secondary and a.no_roofline and a.no_cpu_baseline


def test_full_run_keeps_the_extra_measurements(monkeypatch):
    a = _args(monkeypatch, "--full")
    assert not (a.no_secondary or a.no_roofline or a.no_cpu_baseline)
    a = _args(monkeypatch, "--full", "--no-roofline")
    assert a.no_roofline and not (a.no_secondary or a.no_cpu_baseline)


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--steps", "0")


def test_dump_outputs(tmp_path):
    g = torch.Generator().manual_seed(3)
    params = [torch.randn(20000, generator=g), torch.randn(3, 5, generator=g), torch.randn(100, 300, generator=g).t()]
    last = {"logits": torch.randn(4, 7, generator=g), "grad_norm": torch.tensor(2.5, dtype=torch.float64)}
    loss = torch.tensor(1.25, dtype=torch.bfloat16)
    names = bench.dump_outputs(str(tmp_path / "a"), loss, last, params)
    assert names == ["loss", "logits", "grad_norm", "params_sample"]
    out = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(v.dtype == np.float32 for v in out.values())
    assert out["loss"].tolist() == [1.25] and out["grad_norm"].tolist() == [2.5]
    np.testing.assert_array_equal(out["logits"], last["logits"].numpy())
    k = bench.DUMP_PARAM_ELEMS
    sample = out["params_sample"]
    assert sample.shape == (k + 15 + k,)
    np.testing.assert_array_equal(sample[k:k + 15], params[1].reshape(-1).numpy())       # a small tensor is dumped whole
    assert np.isin(sample[:k], params[0].numpy()).all()
    bench.dump_outputs(str(tmp_path / "b"), loss, last, params)
    for n in names:
        np.testing.assert_array_equal(out[n], np.load(tmp_path / "b" / f"{n}.npy"))    # the sample is fixed
    assert bench.dump_outputs(str(tmp_path / "c"), loss, {}, params) == ["loss", "params_sample"]
