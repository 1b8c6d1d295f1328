"""bench.py --dump-outputs: what the timed path computed in its last step goes to DIR/<name>.npy in float32, under the
64 MB budget, with a fixed seeded sample of the large arrays, so that two builds can be compared output for output.
Runs here on CPU tensors through bench.dump_outputs; the GPU run only feeds it device tensors."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _step_outputs(n=3000, cols=68):
    torch.manual_seed(0)
    pool = torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.BatchNorm1d(4))
    pool(torch.randn(16, 8)).square().sum().backward()
    x = torch.randn(4, 6, 8, 16).contiguous(memory_format=torch.channels_last).requires_grad_()
    x.grad = torch.randn(4, 6, 8, 16).contiguous(memory_format=torch.channels_last)
    return torch.randn(n, cols), x, pool


def test_small_outputs_are_dumped_whole(tmp_path):
    bench = _bench()
    fused, x, pool = _step_outputs()
    shapes = bench.dump_outputs(str(tmp_path), fused, x, pool)
    names = {"fused", "x_grad", "grad_0_weight", "grad_0_bias", "grad_1_weight", "grad_1_bias"}
    assert set(shapes) == names
    assert {f[:-4] for f in os.listdir(tmp_path)} == names
    for name in names:
        assert np.load(tmp_path / f"{name}.npy").dtype == np.float32
    np.testing.assert_array_equal(np.load(tmp_path / "fused.npy"), fused.numpy())
    # logical [B, C, H, W] order, whatever the memory format
    np.testing.assert_array_equal(np.load(tmp_path / "x_grad.npy"), x.grad.contiguous().reshape(-1).numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "grad_0_weight.npy"), pool[0].weight.grad.numpy())


def test_large_outputs_are_a_fixed_sample_under_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 4 * 68 * 10)
    fused, x, pool = _step_outputs()
    bench.dump_outputs(str(tmp_path / "a"), fused, x, pool)
    bench.dump_outputs(str(tmp_path / "b"), fused, x, pool)
    a = np.load(tmp_path / "a" / "fused.npy")
    assert a.shape == (10, 68)
    np.testing.assert_array_equal(a, np.load(tmp_path / "b" / "fused.npy"))          # the same rows every run
    rows = [int(np.flatnonzero((fused.numpy() == r).all(1))[0]) for r in a]
    assert rows == sorted(set(rows))                                                   # distinct, ascending
    g = np.load(tmp_path / "a" / "x_grad.npy")
    assert g.shape == (68 * 10,)
    np.testing.assert_array_equal(g, np.load(tmp_path / "b" / "x_grad.npy"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < bench.DUMP_BUDGET_BYTES


def test_default_sample_fits_the_budget_at_the_headline_shape():
    bench = _bench()
    n, cols, maps = 1 << 20, 4 + 64, 32 * 64 * 64 * 128
    rows = min(n, bench.DUMP_SAMPLE_BYTES // (4 * cols))
    assert rows * cols * 4 + min(maps, bench.DUMP_SAMPLE_BYTES // 4) * 4 + (1 << 20) < bench.DUMP_BUDGET_BYTES


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
