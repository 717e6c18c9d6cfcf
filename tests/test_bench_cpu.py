"""CPU: bench.py's bookkeeping -- `--steps` timed steps split into blocks, and `--dump-outputs` (dtypes, the 64 MB cap and
its seeded sample)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("steps,blocks", [(1, 1), (7, 1), (4, 2), (3, 2), (100, 12), (2, 5)])
def test_split_steps_covers_exactly_the_timed_steps(steps, blocks):
    sizes = bench.split_steps(steps, blocks)
    assert sum(sizes) == steps
    assert len(sizes) == min(steps, blocks) and min(sizes) >= 1 and max(sizes) - min(sizes) <= 1


def test_steps_below_one_is_an_error():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_writes_float_arrays(tmp_path):
    arrays = {"hazards": torch.rand(1, 4), "Y_hat": torch.tensor([[3]]), "A_raw": torch.randn(1, 10).to(torch.bfloat16),
              "loss": torch.tensor(0.5, dtype=torch.float64), "grad.classifier.weight": torch.randn(4, 256)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in arrays)
    for k, v in arrays.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == (np.float64 if v.dtype == torch.float64 else np.float32), k
        np.testing.assert_array_equal(a, v.to(torch.float64).numpy(), err_msg=k)


def test_dump_outputs_samples_above_the_limit(tmp_path):
    big, small = torch.arange(5000, dtype=torch.float32), torch.randn(10)      # big: each value is its own index
    limit = 4 * 2000                                   # 8 kB: two arrays, a 4 kB share each
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, limit_bytes=limit)
    a, b = (np.load(tmp_path / d / "big.npy") for d in ("a", "b"))
    assert a.size == 1000 and a.nbytes + np.load(tmp_path / "a" / "small.npy").nbytes <= limit
    np.testing.assert_array_equal(a, b)                # the same seeded sample every run
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 5000     # distinct elements of the array, in index order
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
