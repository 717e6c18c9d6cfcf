"""GPU parity of the grouped training step (include/mmf_amil.h: mmf_amil_nll_step_group; model.nll_step_group): the G bags
of one accumulation window through one launch chain over their concatenated rows.  Per bag, scores / hazards / S and the
loss against the fp64 oracle of that bag alone (with that bag's own dropout masks); the summed gradients against the
oracle's sum_g loss_scale * grads_g; and the grouped route against G nll_step calls with accumulate."""
import numpy as np
import pytest
import torch

from oracle import cases
from test_gpu_path import DEV, _grads, _load, _t, compare, relu_kink_units

pytestmark = pytest.mark.gpu


def _bag_meta(base, g, n):
    m = dict(base)
    m.update(N=n, x_seed=base["x_seed"] + 101 * g, mask_seed=base["mask_seed"] + 7 * g, y=(g + 1) % base["K"], c=g % 2)
    return m


def _model(m):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    sd, _, _ = cases.path_inputs(dict(m, N=1))
    model = _load(MIL_Attention_fc_surv_path(gate_path=m["gated"], model_size_wsi=m["size"], dropout=m["dropout"],
                                             n_classes=m["K"]), sd)
    model.train() if m["train"] else model.eval()
    return model, sd


def _seeds(monkeypatch, metas):
    from multimodalfusion_amd import ops
    it = iter([mm["mask_seed"] for mm in metas])
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: next(it))


def run_group(metas, monkeypatch, loss_scale):
    model, sd = _model(metas[0])
    if metas[0]["train"]:
        _seeds(monkeypatch, metas)
    bags = [_t(cases.path_inputs(mm)[1]) for mm in metas]
    hz, S, Yh, A, loss, risk = model.nll_step_group(bags, torch.tensor([mm["y"] for mm in metas]),
                                                    torch.tensor([float(mm["c"]) for mm in metas]),
                                                    alpha=metas[0]["alpha"], loss_scale=loss_scale)
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(), A=[a.cpu().numpy() for a in A],
                loss=loss.cpu().numpy(), risk=risk.cpu().numpy(), grads=_grads(model)), model, bags


def run_per_bag(metas, monkeypatch, loss_scale):
    model, _ = _model(metas[0])
    if metas[0]["train"]:
        _seeds(monkeypatch, metas)
    out = dict(hazards=[], S=[], Y_hat=[], A=[], loss=[])
    for mm in metas:
        hz, S, Yh, A, loss, _ = model.nll_step(_t(cases.path_inputs(mm)[1]), torch.tensor([mm["y"]]),
                                               torch.tensor([float(mm["c"])]), alpha=mm["alpha"], loss_scale=loss_scale)
        for k, v in (("hazards", hz), ("S", S), ("Y_hat", Yh), ("A", A), ("loss", loss)):
            out[k].append(v.cpu().numpy())
    torch.cuda.synchronize()
    out["grads"] = _grads(model)
    return out


CASES = [
    ([1, 999, 4097, 10000], True, 4, True, True),
    ([1, 999, 4097, 10000], False, 8, True, True),
    ([1, 999, 4097, 10000], True, 8, False, False),
    ([1000] * 16, False, 8, False, False),
    ([17, 33, 2000], False, 8, False, False),
    ([17, 33, 2000], True, 8, True, True),
    ([1000] * 16, True, 8, True, True),
    ([1000] * 16, False, 4, True, False),
]


@pytest.mark.parametrize("sizes,gated,K,train,dropout", CASES)
def test_group_matches_oracle_per_bag(sizes, gated, K, train, dropout, monkeypatch):
    base = dict(gated=gated, size="small", K=K, dropout=dropout, alpha=0.3, bias_std=0.05, train=train, seed=4242,
                x_seed=500, mask_seed=900)
    metas = [_bag_meta(base, g, n) for g, n in enumerate(sizes)]
    G = len(sizes)
    scale = 1.0 / G
    res, _, _ = run_group(metas, monkeypatch, scale)
    check_group(res, scale, *group_oracle(metas))


def group_oracle(metas):
    """-> (the fp64 oracle of each bag alone, the union of the bags' ReLU-kink units)"""
    refs, kinks = [], set()
    for mm in metas:
        refs.append(cases.run_path(mm))
        sd, x, _ = cases.path_inputs(mm)
        kinks |= relu_kink_units(sd, x)
    return refs, kinks


def check_group(res, scale, refs, kinks, tag=""):
    """A grouped step's results (run_group's layout) per bag against that bag's oracle, and its gradients against the
    oracle's sum_g scale * grads_g."""
    gsum = None
    for g, ref in enumerate(refs):
        one = dict(hazards=res["hazards"][g:g + 1], S=res["S"][g:g + 1], A_raw=res["A"][g], loss=float(res["loss"][g]),
                   grads={})
        compare(one, dict(ref, grads={}), f"{tag}bag {g}")
        assert abs(float(res["risk"][g]) + float(res["S"][g].sum())) < 1e-5, f"{tag}bag {g}"
        gsum = {k: scale * v for k, v in ref["grads"].items()} if gsum is None else \
            {k: gsum[k] + scale * v for k, v in ref["grads"].items()}
    compare(dict(hazards=0, S=0, A_raw=0, loss=0.0, grads=res["grads"]), dict(hazards=0, S=0, A_raw=0, loss=0.0, grads=gsum),
            f"{tag}summed grads", kink_units=kinks)


@pytest.mark.parametrize("sizes,gated,K,train,dropout", [CASES[0], CASES[1], CASES[5], CASES[7]])
def test_group_equals_per_bag_route(sizes, gated, K, train, dropout, monkeypatch):
    base = dict(gated=gated, size="small", K=K, dropout=dropout, alpha=0.1, bias_std=0.05, train=train, seed=77,
                x_seed=600, mask_seed=1900)
    metas = [_bag_meta(base, g, n) for g, n in enumerate(sizes)]
    a, _, _ = run_group(metas, monkeypatch, 0.25)
    b = run_per_bag(metas, monkeypatch, 0.25)
    # fp32 rounding only: a bag's tile plan differs between the routes (a 999-row bag alone takes K-split 64-row tiles,
    # inside the window wide ones), so its scores differ in the last bits -- a few ulp of the largest value
    def ulps(v):
        return 4e-6 * max(1.0, float(np.abs(v).max()))
    assert np.array_equal(a["Y_hat"].reshape(-1), np.concatenate(b["Y_hat"]).reshape(-1))
    hb = np.concatenate(b["hazards"])
    np.testing.assert_allclose(a["hazards"], hb, rtol=0, atol=ulps(hb))
    lb = np.array([float(v) for v in b["loss"]])
    np.testing.assert_allclose(a["loss"], lb, rtol=0, atol=ulps(lb))
    for g in range(len(sizes)):
        np.testing.assert_allclose(a["A"][g], b["A"][g], rtol=0, atol=ulps(b["A"][g]))
    kinks = set()
    for mm in metas:
        sd, x, _ = cases.path_inputs(mm)
        kinks |= relu_kink_units(sd, x)
    for k, v in b["grads"].items():   # (+ 1e-6: d attention_c.bias = sum of ds, zero in exact arithmetic per bag)
        tol = 1e-5 * float(np.abs(v).max()) + 1e-6
        bad = np.abs(a["grads"][k] - v) > tol + 1e-5 * np.abs(v)
        if bad.any() and k in ("attention_net_WSI.0.weight", "attention_net_WSI.0.bias"):
            # the two routes' scores round differently (different tile plans), so a unit whose pre-activation sits on the
            # ReLU kink (relu_kink_units) may take the other side in one of them: that row differs by one instance's dh.x
            # -- bounded, as everywhere in the suite, by 1 % of the tensor's max
            rows = set(np.unique(np.nonzero(bad.reshape(bad.shape[0], -1))[0]).tolist())
            assert rows <= kinks, (k, sorted(rows - kinks))
            assert float(np.abs(a["grads"][k] - v).max()) <= 1e-2 * float(np.abs(v).max()), k
            continue
        assert not bad.any(), (k, float(np.abs(a["grads"][k] - v).max()), tol)


def _raw_setup(sizes, gated=True, K=4):
    from multimodalfusion_amd import ops
    base = dict(gated=gated, size="small", K=K, dropout=True, alpha=0.2, bias_std=0.05, train=True, seed=11, x_seed=12,
                mask_seed=13)
    model, _ = _model(base)
    seq, cls = model.attention_net_WSI, model.classifier
    Wa, ba, Wb, bb, Wc, bc = seq[3].stack_params()
    stack = (seq[0].weight.detach(), seq[0].bias.detach(), Wa.detach(), ba.detach(),
             Wb.detach() if gated else None, bb.detach() if gated else None, Wc.detach(), bc.detach())
    params = [*stack, cls.weight.detach(), cls.bias.detach()]
    grads = [None if p is None else torch.zeros_like(p) for p in params]
    x = _t(np.concatenate([cases.path_inputs(_bag_meta(base, g, n))[1] for g, n in enumerate(sizes)]))
    G = len(sizes)
    Y, c = torch.tensor([g % K for g in range(G)]), torch.tensor([float(g % 2) for g in range(G)])

    def call(accumulate=False, seeds=None, **kw):
        return ops.amil_nll_step_group(x, sizes, stack, params[8], params[9], gated, Y, c, 0.2, grads, loss_scale=0.5,
                                       accumulate=accumulate, p_h=0.25, p_att=0.25,
                                       seeds=seeds or [100 + g for g in range(G)], **kw)
    return call, grads, x, stack, params, Y, c


def test_group_call_contract():
    from multimodalfusion_amd import ops
    call, grads, *_ = _raw_setup([300, 1200, 77])
    call()
    first = [None if g is None else g.clone() for g in grads]
    call()
    for a, b in zip(first, grads):
        if a is not None:
            assert torch.equal(a, b)              # overwrite, and bit-identical on a repeat
    call(accumulate=True)
    for a, b in zip(first, grads):
        if a is not None:
            torch.testing.assert_close(b, 2 * a, rtol=1e-5, atol=1e-6 * float(a.abs().max()) + 1e-12)
    torch.cuda.synchronize()
    assert int(ops.sync_words(torch.device(DEV)).abs().sum()) == 0


def test_group_of_one_is_nll_step():
    from multimodalfusion_amd import ops
    call, grads, x, stack, params, Y, c = _raw_setup([2345])
    hz, S, Yh, A, loss, risk = call(seeds=[321])
    torch.cuda.synchronize()
    got = [None if g is None else g.clone() for g in grads]
    hz1, S1, Yh1, A1, loss1, _ = ops.amil_nll_step(x, stack, params[8], params[9], True, Y, c, 0.2, grads,
                                                  loss_scale=0.5, p_h=0.25, p_att=0.25, seed=321)
    torch.cuda.synchronize()
    assert torch.equal(Yh.reshape(-1), Yh1.reshape(-1))
    torch.testing.assert_close(hz, hz1, rtol=0, atol=1e-6)
    torch.testing.assert_close(A[0], A1, rtol=0, atol=1e-6)
    assert abs(float(loss[0]) - float(loss1)) <= 1e-6
    for a, b in zip(got, grads):
        if a is not None:
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5 * float(b.abs().max()) + 1e-6)


def test_group_rejects_bad_calls():
    from multimodalfusion_amd import _lib, ops
    call, grads, x, stack, params, Y, c = _raw_setup([64, 64])
    with pytest.raises(_lib.MmfError):        # an empty bag
        ops.amil_nll_step_group(x, [128, 0], stack, params[8], params[9], True, [0, 0], [0.0, 0.0], 0.0, grads)
    with pytest.raises(_lib.MmfError):        # G > 64
        ops.amil_nll_step_group(x[:65], [1] * 65, stack, params[8], params[9], True, [0] * 65, [0.0] * 65, 0.0, grads)
    with pytest.raises(_lib.MmfError):        # label count != G
        ops.amil_nll_step_group(x, [64, 64], stack, params[8], params[9], True, [0, 1, 2], [0.0, 0.0, 0.0], 0.0, grads)
    with pytest.raises(_lib.MmfError):        # bf16 bags
        ops.amil_nll_step_group(x.to(torch.bfloat16), [64, 64], stack, params[8], params[9], True, Y, c, 0.0, grads)
    prev = ops.set_gemm(1)
    try:
        with pytest.raises(_lib.MmfError, match="invalid argument"):    # bf16x3 GEMMs: MMF_ERR_ARG from the library
            call()
    finally:
        ops.set_gemm(prev)
