"""GPU: a plain `bench.py` run prints the headline line and nothing that needs runs of its own; `--full` adds the legs
beside the headline (here the ones every N = 1 run has: one bag at a time, per-step percentiles, per-kernel times, the
autograd surface)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("one_bag_in_flight", "value_one_bag_per_step", "step_ms_device", "kernels_us", "autograd_surface",
             "other_sizes", "n_sweep", "gemm_bf16x3", "pcie_inclusive", "cpu_baseline")


def _line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--bag", "3000",
           *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


def test_plain_run_is_the_headline_only():
    out = _line()
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "bags/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 3 and sum(out["blocks"]["steps_per_block"]) == 3
    assert not set(FULL_ONLY) & set(out), sorted(set(FULL_ONLY) & set(out))


def test_full_adds_the_legs_beside_the_headline():
    out = _line("--full", "--no-extras", "--no-cpu-baseline")
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["one_bag_in_flight"]["value"] > 0 and out["value_one_bag_per_step"] > 0
    assert out["autograd_surface"]["ms_per_step"] > 0 and out["step_ms_device"]["p50"] > 0
    assert out["kernels_us"] and all(v > 0 for v in out["kernels_us"].values())
    assert "other_sizes" not in out and "cpu_baseline" not in out        # --no-extras / --no-cpu-baseline still hold
