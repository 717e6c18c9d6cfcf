"""GPU: the one-call stage-2 training step (model.step -> ops.stage2_step -> mmf_stage2_step) on every case of
tests/stage2_step_cases.py against the float64 oracle and against the autograd route of the same model, its call behaviour,
its launch budget, poisoned memory, step_ok and the fused training / validation loops.

Every comparison prints its largest error / bar ratio (-s); the bars are the case module's (tests/test_gpu_stage2.py's)."""
import copy
import functools

import numpy as np
import pytest
import torch

import stage2_step_cases as sc
from test_gpu_path import DEV
from test_gpu_poison import MODES, poison  # noqa: F401  (the fixture)
from test_gpu_stage2 import _loss_fn

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in sc.CASES]


def _inputs(c):
    hs, Y, cens, t = sc.batch(c)
    return [torch.as_tensor(h).to(DEV) for h in hs], torch.as_tensor(Y).to(DEV), torch.as_tensor(cens).to(DEV), t


def _collect(model, risk, hazards, S, loss):
    torch.cuda.synchronize()
    out = dict(risk=risk.detach().cpu().numpy().reshape(-1), loss=float(loss.detach()),
               grads={k: (p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                      for k, p in model.named_parameters()},
               none={k for k, p in model.named_parameters() if p.grad is None},
               buffers={k: b.detach().cpu().numpy() for k, b in model.named_buffers() if "running" in k},
               tracked={k: int(b) for k, b in model.named_buffers() if "num_batches_tracked" in k})
    if hazards is not None:
        out.update(hazards=hazards.detach().cpu().numpy(), S=S.detach().cpu().numpy())
    return out


def _pinned(c):
    """ops.next_dropout_seed pinned to the case's mask seed for the duration (as run_hip of tests/test_gpu_stage2.py does)."""
    from multimodalfusion_amd import ops
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "next_dropout_seed", lambda: sc.meta(c)["mask_seed"])
    return mp


def _step(c, model=None, **kw):
    model = model if model is not None else sc.make_model(c)[0].to(DEV)
    (hr, hp, ho), Y, cens, t = _inputs(c)
    mp = _pinned(c)
    try:
        out = model.step(hr, hp, ho, _loss_fn(c.loss), label=Y, event_time=t, c=cens, **kw)
    finally:
        mp.undo()
    return model, out


@functools.lru_cache(maxsize=None)
def fused(name):
    model, out = _step(sc.BY_NAME[name])
    return _collect(model, *out)


@functools.lru_cache(maxsize=None)
def autograd(name):
    from multimodalfusion_amd.utils.core_utils_pretrained import _loss
    c = sc.BY_NAME[name]
    model = sc.make_model(c)[0].to(DEV)
    (hr, hp, ho), Y, cens, t = _inputs(c)
    mp = _pinned(c)
    try:
        risk, hazards, S = model(h_radio=hr, h_path=hp, h_omic=ho)
        loss = _loss(_loss_fn(c.loss), risk, hazards, S, Y, t, cens, DEV)
        loss.backward()
    finally:
        mp.undo()
    return _collect(model, risk, hazards, S, loss)


@pytest.mark.parametrize("name", NAMES)
def test_step_matches_the_float64_oracle(name):
    c = sc.BY_NAME[name]
    res, ref = fused(name), sc.oracle(name)
    worst = sc.check(res, ref, c, what="step vs oracle ")
    print(f"{name}: worst error / bar = {worst:.3f}")
    assert all(v == (1 if c.train else 0) for v in res["tracked"].values()) and res["tracked"], name
    if c.special in ("all_censored", "no_pair"):
        assert res["loss"] == 0.0 and all(not g.any() for g in res["grads"].values()), name


@pytest.mark.parametrize("name", NAMES)
def test_step_matches_the_autograd_route(name):
    c = sc.BY_NAME[name]
    res, ref = fused(name), autograd(name)
    ref = dict(ref, risk=ref["risk"].reshape(-1))
    worst = sc.check(res, ref, c, factor=2.0, what="step vs autograd ", basis=sc.oracle(name))
    print(f"{name}: worst error / (2 bars) = {worst:.3f}")
    assert res["none"] == ref["none"], (name, res["none"] ^ ref["none"])
    assert res["tracked"] == ref["tracked"], name


CALL_CASES = [n for n in NAMES if "_b32_" in n]


@pytest.mark.parametrize("name", CALL_CASES)
def test_call_behaviour(name):
    c = sc.BY_NAME[name]
    base = fused(name)
    model0 = sc.make_model(c)[0].to(DEV)
    params = lambda m: list(m.parameters())
    names = [k for k, _ in model0.named_parameters()]
    # two calls are bit-identical
    again = _collect(*[(m, *o) for m, o in [_step(c)]][0])
    for k in ("risk", "hazards", "S"):
        if k in base:
            assert np.array_equal(base[k], again[k]), (name, k)
    assert base["loss"] == again["loss"]
    for k in names:
        assert np.array_equal(base["grads"][k], again["grads"][k]), (name, k)
    # grad_out is honoured: overwritten (NaN before), .grad untouched, the idle entries zeroed
    model = copy.deepcopy(model0)
    out = [torch.full_like(p, float("nan")) for p in params(model)]
    _step(c, model, grad_out=out, accumulate=False)
    assert all(p.grad is None for p in params(model))
    for k, o in zip(names, out):
        assert np.array_equal(o.cpu().numpy(), base["grads"][k]), (name, k)
    # accumulate adds (one rounding of base + gradient)
    gen = torch.Generator().manual_seed(7)
    seed = [torch.randn(p.shape, generator=gen) for p in params(model0)]
    model = copy.deepcopy(model0)
    out = [s.to(DEV) for s in seed]
    _step(c, model, grad_out=out, accumulate=True)
    for k, o, s in zip(names, out, seed):
        want = s.double().numpy() + base["grads"][k]
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(o.cpu().double().numpy() - want) <= ulp).all(), (name, k)
    # .grad set: added to; the dropped modality's stays None
    model = copy.deepcopy(model0)
    for k, p, s in zip(names, params(model), seed):
        if k not in base["none"]:
            p.grad = s.to(DEV)
    _step(c, model)
    for k, p, s in zip(names, params(model), seed):
        if k in base["none"]:
            assert p.grad is None, (name, k)
        else:
            want = s.double().numpy() + base["grads"][k]
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(p.grad.cpu().double().numpy() - want) <= ulp).all(), (name, k)
    # loss_scale scales the gradients and not the loss
    model, o = _step(c, loss_scale=0.25)
    half = _collect(model, *o)
    assert half["loss"] == base["loss"]
    for k in names:
        np.testing.assert_allclose(half["grads"][k], 0.25 * base["grads"][k], rtol=1e-5, atol=1e-9, err_msg=f"{name} {k}")
    # backward=False: the same forward values, no gradient touched
    model, o = _step(c, backward=False)
    fwd = _collect(model, *o)
    assert fwd["none"] == set(names)
    for k in ("risk", "hazards", "S"):
        if k in base:
            assert np.array_equal(base[k], fwd[k]), (name, k)
    # the same terms in the same order, but s2s_loss_rows is inlined into two kernels (the head here, the backward there) and
    # the compiler may contract a * b + c differently at the two sites: a few roundings of the largest term, not equality
    assert abs(fwd["loss"] - base["loss"]) <= 2e-6 * max(1.0, abs(base["loss"])), name
    for k, b in base["buffers"].items():
        assert np.array_equal(b, fwd["buffers"][k]), (name, k)


def _launches(c, **kw):
    from multimodalfusion_amd._lib import KernelTrace
    tr = KernelTrace(256)
    try:
        with tr:
            _step(c, **kw)
        torch.cuda.synchronize()
        d = tr.dump()
    finally:
        tr.close()
    assert all(k.startswith("s2s_") for k in d), d
    return sum(n for n, _ in d.values())


@pytest.mark.parametrize("name", [n for n in NAMES if "_b2_" in n or "_b256_" in n or "_b1_" in n])
def test_launch_budget(name):
    c = sc.BY_NAME[name]
    hw = "highway" in c.train_type
    n = _launches(c)
    assert 1 <= n <= (2 * c.n_layers + 4 if hw else 4), (name, n)
    n = _launches(c, backward=False)
    assert 1 <= n <= (c.n_layers + 2 if hw else 2), (name, n)


@pytest.mark.parametrize("name", [n for n in NAMES if "_b33_" in n or "_b3_" in n])
def test_step_on_poisoned_memory(name, poison):  # noqa: F811
    """Workspace, outputs and fresh gradient buffers pre-filled with NaN / 1e30: every output finite and equal to the clean
    run, bit for bit."""
    c = sc.BY_NAME[name]
    base = fused(name)
    for mode in MODES:
        model, o = poison.run(mode, _step, c)
        res = _collect(model, *o)
        for k in ("risk", "hazards", "S"):
            if k in base:
                assert np.isfinite(res[k]).all() and np.array_equal(base[k], res[k]), (name, mode, k)
        assert res["loss"] == base["loss"], (name, mode)
        assert res["none"] == base["none"]
        for k, g in base["grads"].items():
            assert np.isfinite(res["grads"][k]).all() and np.array_equal(g, res["grads"][k]), (name, mode, k)
        for k, b in base["buffers"].items():
            assert np.array_equal(b, res["buffers"][k]), (name, mode, k)
        model, o = poison.run(mode, lambda: _step(c, backward=False))
        res = _collect(model, *o)
        assert np.isfinite(res["risk"]).all() and np.array_equal(base["risk"], res["risk"]) and np.isfinite(res["loss"])


def test_step_ok_says_no():
    from multimodalfusion_amd.models import coxranking_models_pretrained as cm
    from multimodalfusion_amd.models import nll_models_pretrained as nm
    from multimodalfusion_amd.utils.loss_utils import CoxSurvLoss, NLLSurvLoss, RankingSurvLoss
    h = torch.zeros(32, 256, device=DEV)
    model = nm.multimodal_pretrained(train_type="late-fcnn", mode="radio_path").to(DEV)
    assert model.step_ok(h, h, h, NLLSurvLoss()) and model.step_ok(h, h, h, RankingSurvLoss())
    assert not nm.multimodal_pretrained(train_type="kronecker", mode="radio_path").to(DEV).step_ok(h, h, h, NLLSurvLoss())
    big = torch.zeros(257, 256, device=DEV)
    assert not model.step_ok(big, big, big, NLLSurvLoss())
    assert not model.step_ok(h.double(), h.double(), h.double(), NLLSurvLoss())
    assert not model.step_ok(h.cpu(), h.cpu(), h.cpu(), NLLSurvLoss())
    assert not model.step_ok(h[:1], h[:1], h[:1], NLLSurvLoss())                 # train mode needs two rows
    model.eval()
    assert model.step_ok(h[:1], h[:1], h[:1], NLLSurvLoss()) and not model.step_ok(h[:1], h[:1], h[:1], RankingSurvLoss())
    model.train()
    assert not model.step_ok(h, h, h, object())
    model.layer_omic[0].weight.requires_grad_(False)                            # a frozen parameter, even the dropped block's
    assert not model.step_ok(h, h, h, NLLSurvLoss())
    cox = cm.multimodal_pretrained(train_type="late-highway", mode="path_omic").to(DEV)
    assert cox.step_ok(h, h, h, CoxSurvLoss()) and not cox.step_ok(h, h, h, NLLSurvLoss())
    # the measured exceptions (tools/stage2_step_bench.py): early-highway forward only, and two layers below 128 rows
    h128 = torch.zeros(128, 256, device=DEV)
    for mod, fn in ((nm, NLLSurvLoss()), (cm, CoxSurvLoss())):
        one = mod.multimodal_pretrained(train_type="early-highway", mode="path_omic", n_layers=1).to(DEV)
        two = mod.multimodal_pretrained(train_type="early-highway", mode="path_omic", n_layers=2).to(DEV)
        assert one.step_ok(None, h, h, fn) and not two.step_ok(None, h, h, fn) and two.step_ok(None, h128, h128, fn)
        assert not one.eval().step_ok(None, h, h, fn) and not two.eval().step_ok(None, h128, h128, fn)
        assert mod.multimodal_pretrained(train_type="late-highway", n_layers=2).to(DEV).eval().step_ok(h, h, h, fn)
    with pytest.raises(NotImplementedError):
        cox.step(h, h, h, NLLSurvLoss(), label=torch.zeros(32, dtype=torch.int64, device=DEV), c=torch.zeros(32, device=DEV))


def _loop_batches(n, B, K):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(n):
        label = torch.randint(0, K, (B,), generator=g)
        t = (label.double() * 2.0 + torch.randint(0, 4, (B,), generator=g).double() * 0.5).numpy()
        cens = (torch.rand(B, generator=g) < 0.3).float()
        out.append((torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g),
                    label, t, cens, None))
    return out


@pytest.mark.parametrize("gc", [1, 2])
@pytest.mark.parametrize("family,tt,mode,loss", [
    ("nll", "late-fcnn", "radio_path", ("rank_nll", "sigmoid", "mean", 0.15, 0.5)),
    ("nll", "early-highway", "radio_path_omic", ("nll", 0.15)),          # one layer: step_ok keeps deeper ones off below 128 rows
    ("cox", "late-highway", "path_omic", ("cox",)),
    ("cox", "early-fcnn", "radio_omic", ("rank", "relu", "mean")),
])
def test_fused_loops_match_the_default_route(family, tt, mode, loss, gc):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import coxranking_models_pretrained as cm
    from multimodalfusion_amd.models import nll_models_pretrained as nm
    from multimodalfusion_amd.utils import core_utils_pretrained as cu
    K = 4 if family == "nll" else 1
    torch.manual_seed(3)
    model0 = (nm if family == "nll" else cm).multimodal_pretrained(n_classes=K, mode=mode, train_type=tt,
                                                                    n_layers=1 if tt == "early-highway" else 2).to(DEV)
    batches = _loop_batches(4, 16, 4)
    res = {}
    for fused_flag in (False, True):
        model = copy.deepcopy(model0)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        seeds = iter(range(1000, 2000))
        mp = pytest.MonkeyPatch()
        mp.setattr(ops, "next_dropout_seed", lambda: next(seeds))
        try:
            trip = cu.train_loop_survival(0, model, batches, opt, K, mode, loss_fn=_loss_fn(loss), gc=gc, verbose=False,
                                          fused=fused_flag)
            model.eval()
            val = cu._run(model, batches, _loss_fn(loss), None, 0.0, torch.device(DEV), False, fused=fused_flag)
            assert cu.validate_survival(0, 0, model, batches, K, mode, loss_fn=_loss_fn(loss), verbose=False,
                                        fused=fused_flag) is False
        finally:
            mp.undo()
        torch.cuda.synchronize()
        res[fused_flag] = (trip, val, {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()})
    (trip0, val0, sd0), (trip1, val1, sd1) = res[False], res[True]
    for a, b in zip(trip0 + val0, trip1 + val1):
        assert abs(a - b) <= 4e-5 * max(1.0, abs(a)), (trip0, trip1, val0, val1)
    for k, v in sd0.items():
        if "num_batches_tracked" in k:
            assert np.array_equal(v, sd1[k]), k
        else:
            # two SGD steps of lr 0.05 over gradients that agree within twice the gradient bar, 2 (2e-5 + 2e-4 max|g|)
            np.testing.assert_allclose(sd1[k], v, rtol=2e-4, atol=1e-5, err_msg=k)
