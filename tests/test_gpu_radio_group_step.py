"""GPU parity of the radiology head's grouped training step (include/mmf_amil.h: mmf_radio_nll_step_group;
MIL_Attention_fc_surv_radio.nll_step_group): reduce_dim and the stack over the window's rows in one launch chain.  Per bag,
hazards / S / Y_hat / scores / loss / risk against the fp64 oracle of that bag alone (with that bag's own dropout masks);
the summed gradients, reduce_dim's included, against the oracle's sum_g loss_scale * grads_g; the grouped route against G
nll_step calls with accumulate; and the call contract."""
import numpy as np
import pytest
import torch

from oracle import cases
from test_gpu_path import DEV, _grads, _load, _t, compare, relu_kink_units

pytestmark = pytest.mark.gpu


def _bag_meta(base, g, n):
    m = dict(base)
    m.update(n=n, x_seed=base["x_seed"] + 101 * g, mask_seed=base["mask_seed"] + 7 * g, y=(g + 1) % base["K"], c=g % 2)
    return m


def _model(m):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    sd, _, _ = cases.radio_inputs(dict(m, n=1))
    model = _load(MIL_Attention_fc_surv_radio(radio_fusion="concat", gate_radio=m["gated"], dropout=m["dropout"],
                                              n_classes=m["K"], modalities=cases.MODS[:m["n_mod"]]), sd)
    model.train() if m["train"] else model.eval()
    return model, sd


def _seeds(monkeypatch, metas):
    from multimodalfusion_amd import ops
    it = iter([mm["mask_seed"] for mm in metas])
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: next(it))


def _bag(mm):
    return {k: _t(x) for k, x in zip(cases.MODS, cases.radio_inputs(mm)[1])}


def run_group(metas, monkeypatch, loss_scale, model=None, **kw):
    if model is None:
        model, _ = _model(metas[0])
    if metas[0]["train"]:
        _seeds(monkeypatch, metas)
    hz, S, Yh, A, loss, risk = model.nll_step_group([_bag(mm) for mm in metas], torch.tensor([mm["y"] for mm in metas]),
                                                    torch.tensor([float(mm["c"]) for mm in metas]),
                                                    alpha=metas[0]["alpha"], loss_scale=loss_scale, **kw)
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(), A=[a.cpu().numpy() for a in A],
                loss=loss.cpu().numpy(), risk=risk.cpu().numpy(), grads=_grads(model))


def run_per_bag(metas, monkeypatch, loss_scale):
    model, _ = _model(metas[0])
    if metas[0]["train"]:
        _seeds(monkeypatch, metas)
    out = dict(hazards=[], S=[], Y_hat=[], A=[], loss=[])
    for mm in metas:
        hz, S, Yh, A, loss, _ = model.nll_step(torch.tensor([mm["y"]]), torch.tensor([float(mm["c"])]), alpha=mm["alpha"],
                                               loss_scale=loss_scale, **_bag(mm))
        for k, v in (("hazards", hz), ("S", S), ("Y_hat", Yh), ("A", A), ("loss", loss)):
            out[k].append(v.cpu().numpy())
    torch.cuda.synchronize()
    out["grads"] = _grads(model)
    return out


def _kinks(metas):
    """Hidden units of the stack's first layer on the ReLU kink for some row of the window (relu_kink_units on the fp64
    reduce_dim output)."""
    kinks = set()
    for mm in metas:
        sd, xs, _ = cases.radio_inputs(mm)
        if mm["n_mod"] > 1:
            x = np.concatenate([np.asarray(v, np.float64) for v in xs], 1) @ np.asarray(sd["reduce_dim.weight"], np.float64).T \
                + np.asarray(sd["reduce_dim.bias"], np.float64)
        else:
            x = xs[0]
        kinks |= relu_kink_units(sd, x, prefix="attention_net_radio")
    return kinks


def check_group(res, scale, metas):
    gsum = None
    for g, mm in enumerate(metas):
        ref = cases.run_radio(mm)
        one = dict(hazards=res["hazards"][g:g + 1], S=res["S"][g:g + 1], A_raw=res["A"][g], loss=float(res["loss"][g]),
                   grads={})
        compare(one, dict(ref, grads={}), f"bag {g}")
        assert np.array_equal(res["Y_hat"][g].reshape(-1), np.asarray(ref["Y_hat"]).reshape(-1)), f"bag {g}"
        assert abs(float(res["risk"][g]) + float(res["S"][g].sum())) < 1e-5, f"bag {g}"
        gsum = {k: scale * v for k, v in ref["grads"].items()} if gsum is None else \
            {k: gsum[k] + scale * v for k, v in ref["grads"].items()}
    assert set(gsum) == set(res["grads"])
    kinks = _kinks(metas)
    stack = {k: v for k, v in gsum.items() if not k.startswith("reduce_dim")}
    compare(dict(hazards=0, S=0, A_raw=0, loss=0.0, grads=res["grads"]), dict(hazards=0, S=0, A_raw=0, loss=0.0, grads=stack),
            "summed grads", kink_units=kinks, kink_prefix="attention_net_radio")
    for k in ("reduce_dim.weight", "reduce_dim.bias"):
        if k not in gsum:
            continue
        err = float(np.abs(res["grads"][k] - gsum[k]).max())
        top = float(np.abs(gsum[k]).max())
        # a kink unit's row of du differs by one instance's dh, which reaches every column of dW_r through W1
        bar = 1e-2 * top if kinks else 1e-5 + 1e-4 * top
        assert err <= bar, (k, err, bar, sorted(kinks))


RAGGED = [1, 17, 100, 333]                       # 451 rows: a short window, reduce_dim takes its K split
LONG = [600, 1, 1500, 17, 2100, 333]              # 4,551 rows
SIXTY_FOUR = [1 + (37 * g) % 90 for g in range(64)]

# sizes, gated, n_mod, K, train, dropout
CASES = [
    (RAGGED, True, 4, 4, True, True),
    (RAGGED, False, 2, 8, False, False),
    (LONG, True, 4, 4, True, True),
    (LONG, False, 3, 4, False, False),
    (SIXTY_FOUR, False, 4, 4, True, True),
    (SIXTY_FOUR, True, 2, 4, False, False),
    ([777], True, 2, 4, True, True),
    ([17, 300, 64], True, 1, 4, True, True),      # one modality: no reduce_dim, the pathology head's grouped step
]


@pytest.mark.parametrize("sizes,gated,n_mod,K,train,dropout", CASES)
def test_radio_group_matches_oracle_per_bag(sizes, gated, n_mod, K, train, dropout, monkeypatch):
    base = dict(gated=gated, n_mod=n_mod, K=K, dropout=dropout, alpha=0.3, bias_std=0.05, train=train, seed=4343,
                x_seed=510, mask_seed=910)
    metas = [_bag_meta(base, g, n) for g, n in enumerate(sizes)]
    scale = 1.0 / len(sizes)
    check_group(run_group(metas, monkeypatch, scale), scale, metas)


def _ulps(v):
    return 4e-6 * max(1.0, float(np.abs(v).max()))


@pytest.mark.parametrize("sizes,gated,n_mod,K,train,dropout", [CASES[0], CASES[3], CASES[4], CASES[7]])
def test_radio_group_equals_per_bag_route(sizes, gated, n_mod, K, train, dropout, monkeypatch):
    base = dict(gated=gated, n_mod=n_mod, K=K, dropout=dropout, alpha=0.1, bias_std=0.05, train=train, seed=78,
                x_seed=610, mask_seed=1910)
    metas = [_bag_meta(base, g, n) for g, n in enumerate(sizes)]
    a = run_group(metas, monkeypatch, 0.25)
    b = run_per_bag(metas, monkeypatch, 0.25)
    # fp32 rounding only: a bag's tile plans differ between the routes
    assert np.array_equal(a["Y_hat"].reshape(-1), np.concatenate(b["Y_hat"]).reshape(-1))
    hb = np.concatenate(b["hazards"])
    np.testing.assert_allclose(a["hazards"], hb, rtol=0, atol=_ulps(hb))
    lb = np.array([float(v) for v in b["loss"]])
    np.testing.assert_allclose(a["loss"], lb, rtol=0, atol=_ulps(lb))
    for g in range(len(sizes)):
        np.testing.assert_allclose(a["A"][g], b["A"][g], rtol=0, atol=_ulps(b["A"][g]))
    kinks = _kinks(metas)
    for k, v in b["grads"].items():
        tol = 1e-5 * float(np.abs(v).max()) + 1e-6
        bad = np.abs(a["grads"][k] - v) > tol + 1e-5 * np.abs(v)
        if bad.any() and kinks and (k.startswith("reduce_dim") or k.startswith("attention_net_radio.0.")):
            # a unit on the ReLU kink may take the other side in one route (see check_group)
            assert float(np.abs(a["grads"][k] - v).max()) <= 1e-2 * float(np.abs(v).max()), k
            continue
        assert not bad.any(), (k, float(np.abs(a["grads"][k] - v).max()), tol)


def test_radio_group_accumulate_and_grad_out(monkeypatch):
    base = dict(gated=True, n_mod=4, K=4, dropout=True, alpha=0.2, bias_std=0.05, train=True, seed=91, x_seed=92,
                mask_seed=93)
    metas = [_bag_meta(base, g, n) for g, n in enumerate([200, 17, 901])]
    model, _ = _model(metas[0])
    first = run_group(metas, monkeypatch, 0.5, model=model)["grads"]           # .grad None: written
    again = run_group(metas, monkeypatch, 0.5, model=model)["grads"]           # .grad set: added to
    for k, v in first.items():
        np.testing.assert_allclose(again[k], 2 * v, rtol=1e-5, atol=1e-6 * float(np.abs(v).max()) + 1e-12, err_msg=k)
    views = [torch.full_like(p, 3.0) for p in model.parameters()]
    for p in model.parameters():
        p.grad = None
    run_group(metas, monkeypatch, 0.5, model=model, grad_out=views, accumulate=False)
    assert all(p.grad is None for p in model.parameters())
    for (k, _), v in zip(model.named_parameters(), views):
        np.testing.assert_allclose(v.cpu().numpy(), first[k], rtol=1e-5, atol=1e-6 * float(np.abs(first[k]).max()) + 1e-12,
                                   err_msg=k)
    run_group(metas, monkeypatch, 0.5, model=model, grad_out=views, accumulate=True)
    for (k, _), v in zip(model.named_parameters(), views):
        np.testing.assert_allclose(v.cpu().numpy(), 2 * first[k], rtol=1e-5,
                                   atol=1e-6 * float(np.abs(first[k]).max()) + 1e-12, err_msg=k)


def test_radio_group_pre_stacked_equals_dicts(monkeypatch):
    base = dict(gated=True, n_mod=3, K=4, dropout=True, alpha=0.2, bias_std=0.05, train=True, seed=31, x_seed=32,
                mask_seed=33)
    metas = [_bag_meta(base, g, n) for g, n in enumerate([65, 130])]
    model, _ = _model(metas[0])
    a = run_group(metas, monkeypatch, 1.0, model=model)
    ga = {k: p.grad.clone() for k, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    bags = [_bag(mm) for mm in metas]
    x = torch.stack([torch.cat([b[m] for b in bags]) for m in cases.MODS[:3]])
    _seeds(monkeypatch, metas)
    hz, _, _, _, loss, _ = model.nll_step_group((x, [65, 130]), [mm["y"] for mm in metas], [float(mm["c"]) for mm in metas],
                                                alpha=0.2)
    assert np.array_equal(hz.cpu().numpy(), a["hazards"]) and np.array_equal(loss.cpu().numpy(), a["loss"])
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, ga[k]), k


def _raw_setup(sizes, n_mod=4, K=4):
    from multimodalfusion_amd import ops
    base = dict(gated=True, n_mod=n_mod, K=K, dropout=True, alpha=0.2, bias_std=0.05, train=True, seed=11, x_seed=12,
                mask_seed=13)
    model, _ = _model(base)
    seq, cls, rd = model.attention_net_radio, model.classifier, model.reduce_dim
    Wa, ba, Wb, bb, Wc, bc = seq[3].stack_params()
    stack = tuple(p.detach() for p in (seq[0].weight, seq[0].bias, Wa, ba, Wb, bb, Wc, bc))
    params = [rd.weight.detach(), rd.bias.detach(), *stack, cls.weight.detach(), cls.bias.detach()]
    grads = [torch.zeros_like(p) for p in params]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    xs = [torch.randn(sum(sizes), 1024, device=DEV, generator=gen) for _ in range(n_mod)]
    G = len(sizes)
    Y, c = torch.tensor([g % K for g in range(G)]), torch.tensor([float(g % 2) for g in range(G)])

    def call(xs=xs, sizes=sizes, Y=Y, c=c, Wk=params[10], bk=params[11], grads=grads, accumulate=False):
        return ops.radio_nll_step_group(xs, sizes, params[0], params[1], stack, Wk, bk, True, Y, c, 0.2, grads,
                                        loss_scale=0.5, accumulate=accumulate, p_h=0.25, p_att=0.25,
                                        seeds=[100 + g for g in range(len(sizes))])
    return call, grads, xs, params


def test_radio_group_repeat_is_bit_identical_and_leaves_sync_words_zero():
    from multimodalfusion_amd import ops
    call, grads, *_ = _raw_setup([300, 12, 99])
    call()
    first = [g.clone() for g in grads]
    call()
    for a, b in zip(first, grads):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    assert int(ops.sync_words(torch.device(DEV)).abs().sum()) == 0


def test_radio_group_rejects_bad_calls():
    from multimodalfusion_amd import _lib, ops
    call, grads, xs, params = _raw_setup([64, 64])
    with pytest.raises(_lib.MmfError):        # modalities with different row counts
        call(xs=[xs[0], xs[1][:100], xs[2], xs[3]])
    with pytest.raises(_lib.MmfError):        # G > 64
        call(xs=[x[:65] for x in xs], sizes=[1] * 65, Y=[0] * 65, c=[0.0] * 65)
    with pytest.raises(_lib.MmfError):        # an empty bag
        call(sizes=[128, 0], Y=[0, 0], c=[0.0, 0.0])
    with pytest.raises(_lib.MmfError):        # bf16 bags
        call(xs=[x.to(torch.bfloat16) for x in xs])
    Wk = torch.zeros(33, 512, device=DEV)
    with pytest.raises(_lib.MmfError):        # K > 32
        call(Wk=Wk, bk=torch.zeros(33, device=DEV), grads=grads[:10] + [torch.zeros_like(Wk), torch.zeros(33, device=DEV)],
             Y=[0, 1], c=[0.0, 0.0])
    prev = ops.set_gemm(1)
    try:
        with pytest.raises(_lib.MmfError, match="invalid argument"):    # bf16x3 GEMMs: MMF_ERR_ARG from the library
            call()
    finally:
        ops.set_gemm(prev)
    call()                                    # still fine afterwards
    torch.cuda.synchronize()
