"""GPU: `bench.py --dump-outputs` writes what the LAST timed step computed.  A short run with two bags in flight, in eval mode
(no dropout draw); the step of the bag that run issued last is recomputed here with the bench's own model and bags and must
match it array for array (the bench's bags in flight pick other tiles: rounding differs, wiring mistakes do not pass)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    steps, warmup, N, inflight = 3, 1, 3000, 2
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--bag", str(N), "--inflight", str(inflight), "--eval-mode", "--no-extras", "--no-cpu-baseline",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    res = json.loads(line[0])
    assert res["steps"] == steps and sum(res["blocks"]["steps_per_block"]) == steps and res["ms_per_step"] > 0

    dev = torch.device("cuda", 0)
    model = bench.build_model(dev, eval_mode=True)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)                                   # rank 0's bag
    x = torch.randn(N, 1024, device=dev, generator=g)
    bag = bench.distinct_bags(x, inflight)[(warmup + steps - 1) % inflight]
    grads = [torch.empty_like(p) for p in model.parameters()]
    out = model.nll_step(bag, torch.tensor([1], device=dev), torch.tensor([0.0], device=dev), alpha=0.0, grad_out=grads,
                         accumulate=False)
    torch.cuda.synchronize()
    want = bench.step_outputs(model, out, grads)
    assert {"hazards", "S", "Y_hat", "A_raw", "loss", "grad.classifier.weight"} <= set(want)
    assert sorted(os.listdir(out_dir)) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        got, ref = np.load(out_dir / (k + ".npy")), v.float().cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape, (k, got.dtype, got.shape, ref.shape)
        err = np.abs(got.astype(np.float64) - ref).max()
        assert err <= 1e-4 * max(np.abs(ref).max(), 1e-12), (k, err)
