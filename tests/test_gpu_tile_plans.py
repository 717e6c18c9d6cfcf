"""GPU parity of every large-bag tile plan against the fp64 oracle.

Above 16,384 rows (8,192 for the `big` head) the fp32 stack's projection and K-dh pick a tile height per bag size, each
height (and each K-dh variant) its own compiled kernel; the grouped step has its own instantiations, and bf16 storage
takes 256-row tiles on its unfused route from ~16k-32k rows.  The size tables of tests/launch_plans.py reach every plan
the planner can reach (pinned on CPU by tests/test_launch_plans_cpu.py); here each case runs on the GPU against the
oracle with the suite's existing bars: compare() of test_gpu_path.py, check_group() of test_gpu_group_step.py and
test_gpu_radio_group_step.py, compare_bf16() of test_gpu_bf16.py."""
import functools

import numpy as np
import pytest
import torch

import launch_plans as lp
from oracle import cases
from test_gpu_bf16 import _oracle as bf16_oracle
from test_gpu_bf16 import _xq, compare_bf16, run_path_hip_bf16
from test_gpu_nll_step import run_step
from test_gpu_path import DEV, _grads, _load, _t, compare, relu_kink_units, run_path_hip

pytestmark = pytest.mark.gpu


def _meta(N, head, gated, dropout, train):
    return dict(N=N, gated=gated, size=head, K=4, dropout=dropout, y=N % 4, c=N % 2, alpha=0.1, bias_std=0.05,
                train=train, seed=9100 + N % 997, x_seed=9200 + N % 991, mask_seed=4321 + N % 13)


@functools.lru_cache(maxsize=2)
def _oracle(N, head, gated, dropout, train):
    m = _meta(N, head, gated, dropout, train)
    sd, x, _ = cases.path_inputs(m)
    return cases.run_path(m), relu_kink_units(sd, x)


def _run_flight(m, monkeypatch):
    """The headline's route: the bag issued twice through BagsInFlight(model, 2) (one per stream, concurrent hint
    raised, loss_scale 1/2 each); each call's outputs and the reduced gradient stand for one bag."""
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    from multimodalfusion_amd.pipeline import BagsInFlight
    sd, x, _ = cases.path_inputs(m)
    model = _load(MIL_Attention_fc_surv_path(gate_path=m["gated"], model_size_wsi=m["size"], dropout=m["dropout"],
                                             n_classes=m["K"]), sd)
    model.train() if m["train"] else model.eval()
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: m["mask_seed"])
    xt = _t(x)
    y, c = torch.tensor([m["y"]], device=DEV), torch.tensor([float(m["c"])], device=DEV)
    pipe = BagsInFlight(model, 2)
    outs = [pipe.run_fused(model, xt, y, c, m["alpha"], loss_scale=0.5, inputs=(xt,)) for _ in range(2)]
    pipe.assign_grads(pipe.reduce())
    torch.cuda.synchronize()
    assert ops.set_concurrent(False) == 0          # BagsInFlight restored the hint
    res = []
    for hz, S, Yh, A_raw, loss, _ in outs:
        res.append(dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(), A_raw=A_raw.cpu().numpy(),
                        loss=float(loss), M=None, grads={}))
    res[0]["grads"] = _grads(model)
    return res


@pytest.mark.parametrize("N,head,gated,dropout,train,concurrent,route,why", lp.ONE_BAG,
                         ids=[f"{c[0]}-{c[1]}-{c[6]}" + ("-concurrent" if c[5] else "") for c in lp.ONE_BAG])
def test_one_bag_tile_plan(N, head, gated, dropout, train, concurrent, route, why, monkeypatch):
    from multimodalfusion_amd import ops
    m = _meta(N, head, gated, dropout, train)
    tag = f"N={N} {head} gated={gated} dropout={dropout} train={train} concurrent={concurrent} {route}: {why}"
    if route == "flight":
        res = _run_flight(m, monkeypatch)
        ref, kinks = _oracle(N, head, gated, dropout, train)
        compare(res[1], dict(ref, grads={}), tag + " (second stream)")
        compare(res[0], ref, tag, kink_units=kinks)
        return
    prev = ops.set_concurrent(concurrent)
    try:
        if route == "autograd":
            res = run_path_hip(m, monkeypatch)
        else:
            res, _ = run_step(m, monkeypatch)
    finally:
        ops.set_concurrent(prev)
    ref, kinks = _oracle(N, head, gated, dropout, train)
    compare(res, ref, tag, kink_units=kinks)


# ---- grouped windows above the wide threshold ------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,head,gated,K,train,dropout,why", lp.GROUPED,
                         ids=[f"{sum(c[0])}x{len(c[0])}-{c[1]}" for c in lp.GROUPED])
def test_grouped_window_tile_plan(sizes, head, gated, K, train, dropout, why, monkeypatch):
    from test_gpu_group_step import _bag_meta, check_group, group_oracle, run_group
    base = dict(gated=gated, size=head, K=K, dropout=dropout, alpha=0.3, bias_std=0.05, train=train, seed=5151,
                x_seed=700 + len(sizes), mask_seed=1700)
    metas = [_bag_meta(base, g, n) for g, n in enumerate(sizes)]
    scale = 1.0 / len(sizes)
    res, _, _ = run_group(metas, monkeypatch, scale)
    check_group(res, scale, *group_oracle(metas), tag=f"{sum(sizes)} rows {head}: {why}: ")


@pytest.mark.parametrize("sizes,n_mod,gated,K,train,dropout,why", lp.RADIO,
                         ids=[f"radio-{sum(c[0])}x{c[1]}" for c in lp.RADIO])
def test_radio_window_tile_plan(sizes, n_mod, gated, K, train, dropout, why, monkeypatch):
    from test_gpu_radio_group_step import _bag_meta, check_group, run_group
    base = dict(gated=gated, n_mod=n_mod, K=K, dropout=dropout, alpha=0.2, bias_std=0.05, train=train, seed=6161,
                x_seed=800, mask_seed=1800)
    metas = [_bag_meta(base, g, n) for g, n in enumerate(sizes)]
    scale = 1.0 / len(sizes)
    res = run_group(metas, monkeypatch, scale)
    check_group(res, scale, metas)


# ---- bf16 storage on its unfused route ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,head,gated,dropout,train,why", lp.BF16, ids=[f"{c[0]}-{c[1]}" for c in lp.BF16])
def test_bf16_unfused_tile_plan(N, head, gated, dropout, train, why, monkeypatch):
    m = dict(seed=13, gated=gated, size=head, K=4, dropout=dropout, bias_std=0.02, x_seed=N % 1000, N=N, train=train,
             mask_seed=2424, y=N % 4, c=N % 2, alpha=0.0)
    xq = _xq(m)
    res = run_path_hip_bf16(m, monkeypatch, xq)
    compare_bf16(res, bf16_oracle(m, xq), f"N={N} {head}: {why}", a_tol=5e-3, h_tol=2e-3, l_tol=1e-3, g_rel=1e-2)
