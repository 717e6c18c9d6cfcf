"""GPU parity of the multimodal concat head's grouped training step (MM_MIL_Attention_fc_surv.nll_step_group over
include/mmf_amil.h: mmf_amil_group_forward / _backward, mmf_radio_group_forward / _backward,
mmf_surv_head_nll_step_group, mmf_dense_forward_rows / _backward_rows).  Per patient, hazards / S / Y_hat / both score
vectors / loss / risk against the fp64 oracle of that patient alone (train mode: with the masks of that patient's own
seeds); the summed gradients against the oracle's sum_g loss_scale * grads_g; the grouped route against G nll_step calls
on the same seed stream; the call mechanics, the refusals, and the two new raw entry points on their own."""
import numpy as np
import pytest
import torch

from oracle import cases
from oracle import inputs as gen
from oracle import torch_port as tp
from test_gpu_path import DEV, _grads, _load, _t, compare, relu_kink_units
from test_gpu_poison import poison  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BRANCHES = ("radio", "path", "omic")         # nll_step's order of seed draws


def _order(mode):
    return [k for k in BRANCHES if k in mode]


def _metas(base, path_sizes, radio_sizes):
    out = []
    for g, (Np, nr) in enumerate(zip(path_sizes, radio_sizes)):
        m = dict(base, Np=Np, nr=nr, x_seed=base["x_seed"] + 101 * g, y=(g + 1) % base["K"], c=g % 2)
        m["seeds"] = {k: base["mask_seed"] + 1000 * g + 17 * i for i, k in enumerate(BRANCHES)}
        out.append(m)
    return out


def _sd(m):
    return gen.mm_state_dict(seed=m["seed"], input_dim=m["G"], fusion=m.get("fusion", "concat"), gate_path=m["gate_path"],
                             gate_radio=m["gate_radio"], dropout=m["dropout"], n_classes=m["K"], mode=m["mode"], n_mod=4,
                             bias_std=m["bias_std"])


def _model(m):
    from multimodalfusion_amd.models import MM_MIL_Attention_fc_surv
    model = _load(MM_MIL_Attention_fc_surv(input_dim=m["G"], radio_fusion="concat", fusion=m.get("fusion", "concat"),
                                           gate=True, gate_path=m["gate_path"], gate_omic=True,
                                           gate_radio=m["gate_radio"], dropout=m["dropout"], n_classes=m["K"],
                                           mode=m["mode"]), _sd(m))
    model.train() if m["train"] else model.eval()
    return model


def _patient(m):
    _, xs, xp, xo = cases.mm_inputs(dict(m, fusion="concat"))
    kw = {k: _t(x) for k, x in zip(cases.MODS, xs)}
    kw["path_features"] = _t(xp)
    kw["genomic_features"] = _t(xo)
    return kw


def _seed_stream(monkeypatch, metas):
    """ops.next_dropout_seed hands out the patients' seeds in nll_step's order: radio, path, omic of patient 0, then 1, ..."""
    from multimodalfusion_amd import ops
    it = iter([m["seeds"][k] for m in metas for k in _order(m["mode"])])
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: next(it))


def _labels(metas):
    return torch.tensor([m["y"] for m in metas]), torch.tensor([float(m["c"]) for m in metas])


def run_group(metas, monkeypatch, loss_scale, model=None, patients=None, **kw):
    model = _model(metas[0]) if model is None else model
    if metas[0]["train"] and "seeds" not in kw:
        _seed_stream(monkeypatch, metas)
    patients = [_patient(m) for m in metas] if patients is None else patients
    Y, c = _labels(metas)
    hz, S, Yh, A, loss, risk = model.nll_step_group(patients, Y, c, alpha=metas[0]["alpha"], loss_scale=loss_scale, **kw)
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(),
                A={k: [a.cpu().numpy() for a in v] for k, v in A.items()}, loss=loss.cpu().numpy(),
                risk=risk.cpu().numpy(), grads=_grads(model))


def run_per_patient(metas, monkeypatch, loss_scale):
    model = _model(metas[0])
    if metas[0]["train"]:
        _seed_stream(monkeypatch, metas)
    out = dict(hazards=[], S=[], Y_hat=[], A=[], loss=[])
    for m in metas:
        hz, S, Yh, A, loss, _ = model.nll_step(torch.tensor([m["y"]]), torch.tensor([float(m["c"])]), alpha=m["alpha"],
                                               loss_scale=loss_scale, **_patient(m))
        for k, v in (("hazards", hz), ("S", S), ("Y_hat", Yh), ("loss", loss)):
            out[k].append(v.cpu().numpy())
        out["A"].append({k: v.cpu().numpy() for k, v in A.items()})
    torch.cuda.synchronize()
    out["grads"] = _grads(model)
    return out


def oracle_patient(m):
    """The fp64 oracle of one patient alone: cases.run_mm in eval mode; in train mode tp.mm_forward with the masks of the
    patient's three seeds (cases.amil_masks for the stacks, gen.keep_mask for the two AlphaDropout sites)."""
    if not m["train"]:
        assert not m["dropout"]              # cases.mm_inputs builds the state dict without the attention dropout
        return cases.run_mm(dict(m, fusion="concat"))
    _, xs, xp, xo = cases.mm_inputs(dict(m, fusion="concat"))
    sd = tp.to_torch(_sd(m), torch.float64)
    T = lambda a: torch.as_tensor(np.asarray(a)).double()
    tm = lambda d: {k: T(v) for k, v in d.items()}
    s = m["seeds"]
    masks = {"radio": tm(cases.amil_masks(s["radio"], max(m["nr"], 1), 256, 256, m["gate_radio"], m["dropout"])),
             "path": tm(cases.amil_masks(s["path"], max(m["Np"], 1), 256, 256, m["gate_path"], m["dropout"])),
             "omic_keeps": [T(gen.keep_mask(s["omic"], i, 1, 256, 0.25).astype(np.float64)) for i in range(2)]}
    hz, S, Yh, A_raw, _ = tp.mm_forward(sd, [T(x) for x in xs], T(xp), T(xo), fusion="concat", gate_path=m["gate_path"],
                                        gate_radio=m["gate_radio"], dropout=m["dropout"], mode=m["mode"], masks=masks)
    loss = tp.nll_loss(hz, S, torch.tensor([m["y"]]), torch.tensor([float(m["c"])]), alpha=m["alpha"])
    gr = tp.grads_of(loss, sd)
    return dict(hazards=hz.detach().numpy(), S=S.detach().numpy(), Y_hat=Yh.numpy(), loss=float(loss.detach()),
                A_raw={k: v.detach().numpy() for k, v in A_raw.items()},
                grads={k: v.detach().numpy() for k, v in gr.items()})


def _kinks(metas):
    """(pathology, radio) first-layer units on the ReLU kink for some row of the window (relu_kink_units; the radio
    stack's input is the fp64 reduce_dim output)."""
    sd = _sd(metas[0])
    kp, kr = set(), set()
    for m in metas:
        _, xs, xp, _ = cases.mm_inputs(dict(m, fusion="concat"))
        if "path" in m["mode"]:
            kp |= relu_kink_units(sd, xp, prefix="attention_net_WSI")
        if "radio" in m["mode"]:
            x = np.concatenate([np.asarray(v, np.float64) for v in xs], 1) @ np.asarray(sd["reduce_dim.weight"], np.float64).T \
                + np.asarray(sd["reduce_dim.bias"], np.float64)
            kr |= relu_kink_units(sd, x, prefix="attention_net_radio")
    return kp, kr


def _split(grads):
    """(reduce_dim's, the radio stack's, every other) gradient: each part has its own kink rule."""
    rd = {k: v for k, v in grads.items() if k.startswith("reduce_dim")}
    radio = {k: v for k, v in grads.items() if k.startswith("attention_net_radio")}
    rest = {k: v for k, v in grads.items() if k not in rd and k not in radio}
    return rd, radio, rest


def check_group(res, scale, metas):
    gsum = None
    for g, m in enumerate(metas):
        ref = oracle_patient(m)
        keys = {"radiology": "radio", "pathology": "path"}
        one = dict(hazards=res["hazards"][g:g + 1], S=res["S"][g:g + 1], loss=float(res["loss"][g]), grads={},
                   A_raw={k: res["A"][k][g] for k in ref["A_raw"]})
        assert set(res["A"]) == set(ref["A_raw"]) == {k for k, b in keys.items() if b in m["mode"]}
        compare(one, dict(ref, grads={}), f"patient {g}")
        assert int(res["Y_hat"][g]) == int(np.asarray(ref["Y_hat"]).reshape(-1)[0]), f"patient {g}"
        assert abs(float(res["risk"][g]) + float(res["S"][g].sum())) < 1e-5, f"patient {g}"
        gsum = {k: scale * v for k, v in ref["grads"].items()} if gsum is None else \
            {k: gsum[k] + scale * v for k, v in ref["grads"].items()}
    assert set(gsum) == set(res["grads"])
    kp, kr = _kinks(metas)
    zero = dict(hazards=0, S=0, A_raw=0, loss=0.0)
    rd_ref, radio_ref, rest_ref = _split(gsum)
    compare(dict(zero, grads=res["grads"]), dict(zero, grads=rest_ref), "summed grads", kink_units=kp)
    compare(dict(zero, grads=res["grads"]), dict(zero, grads=radio_ref), "summed radio grads", kink_units=kr,
            kink_prefix="attention_net_radio")
    for k, v in rd_ref.items():
        err = float(np.abs(res["grads"][k] - v).max())
        top = float(np.abs(v).max())
        # a kink unit's row of du differs by one instance's dh, which reaches every column of dW_r through W1
        bar = 1e-2 * top if kr else 1e-5 + 1e-4 * top
        assert err <= bar, (k, err, bar, sorted(kr))


RAGGED_P, RAGGED_R = [1, 999, 4097, 10000], [1, 17, 100, 333]
SIXTY_FOUR_P = [1 + (53 * g) % 400 for g in range(64)]
SIXTY_FOUR_R = [1 + (37 * g) % 90 for g in range(64)]

# mode, gate_path, gate_radio, K, pathology sizes, radio sizes, train, attention dropout
CASES = [
    ("radio_path_omic", True, True, 4, RAGGED_P, RAGGED_R, True, True),
    ("radio_path_omic", False, True, 4, RAGGED_P, RAGGED_R, False, False),
    ("radio_path", True, False, 32, [300, 50, 1200], [20, 64, 5], True, True),
    ("path_omic", False, True, 1, [5, 700, 64], [1, 1, 1], False, False),
    ("radio_omic", True, False, 4, [1, 1, 1], [33, 1, 200], True, False),
    ("radio_omic", True, True, 32, [1, 1], [150, 40], False, False),
    ("path_omic", True, True, 4, [64, 2000], [1, 1], True, True),
    ("radio_path_omic", True, True, 4, SIXTY_FOUR_P, SIXTY_FOUR_R, True, True),
    ("radio_path_omic", False, False, 1, SIXTY_FOUR_P, SIXTY_FOUR_R, False, False),
    ("radio_path_omic", False, False, 4, [777], [40], True, True),
    ("radio_path", True, True, 4, [130], [300], False, False),
]


def _base(mode, gate_path, gate_radio, K, train, dropout, **kw):
    base = dict(mode=mode, gate_path=gate_path, gate_radio=gate_radio, K=K, train=train, dropout=dropout, G=80, alpha=0.3,
                bias_std=0.05, seed=4343, x_seed=510, mask_seed=910)
    base.update(kw)
    return base


@pytest.mark.parametrize("mode,gate_path,gate_radio,K,psizes,rsizes,train,dropout", CASES)
def test_mm_group_matches_oracle_per_patient(mode, gate_path, gate_radio, K, psizes, rsizes, train, dropout, monkeypatch):
    metas = _metas(_base(mode, gate_path, gate_radio, K, train, dropout), psizes, rsizes)
    scale = 1.0 / len(metas)
    check_group(run_group(metas, monkeypatch, scale), scale, metas)


def _ulps(v):
    return 4e-6 * max(1.0, float(np.abs(v).max()))


@pytest.mark.parametrize("mode,gate_path,gate_radio,K,psizes,rsizes,train,dropout",
                         [CASES[0], CASES[2], CASES[4], CASES[6], CASES[7]])
def test_mm_group_equals_per_patient_route(mode, gate_path, gate_radio, K, psizes, rsizes, train, dropout, monkeypatch):
    assert train
    metas = _metas(_base(mode, gate_path, gate_radio, K, train, dropout, alpha=0.1, seed=78, x_seed=610, mask_seed=1910),
                   psizes, rsizes)
    a = run_group(metas, monkeypatch, 0.25)
    b = run_per_patient(metas, monkeypatch, 0.25)
    # fp32 rounding only: a bag's tile plans differ between the routes
    assert np.array_equal(a["Y_hat"].reshape(-1), np.concatenate(b["Y_hat"]).reshape(-1))
    hb = np.concatenate(b["hazards"])
    np.testing.assert_allclose(a["hazards"], hb, rtol=0, atol=_ulps(hb))
    lb = np.array([float(v) for v in b["loss"]])
    np.testing.assert_allclose(a["loss"], lb, rtol=0, atol=_ulps(lb))
    for g in range(len(metas)):
        for k, v in b["A"][g].items():
            np.testing.assert_allclose(a["A"][k][g], v, rtol=0, atol=_ulps(v))
    kp, kr = _kinks(metas)
    for k, v in b["grads"].items():
        tol = 1e-5 * float(np.abs(v).max()) + 1e-6
        bad = np.abs(a["grads"][k] - v) > tol + 1e-5 * np.abs(v)
        kinked = (kr and (k.startswith("reduce_dim") or k.startswith("attention_net_radio.0."))
                  or kp and k.startswith("attention_net_WSI.0."))
        if bad.any() and kinked:
            # a unit on the ReLU kink may take the other side in one route (see check_group)
            assert float(np.abs(a["grads"][k] - v).max()) <= 1e-2 * float(np.abs(v).max()), k
            continue
        assert not bad.any(), (k, float(np.abs(a["grads"][k] - v).max()), tol)


MECH = _base("radio_path_omic", True, True, 4, True, True, alpha=0.2, seed=91, x_seed=92, mask_seed=93)


def test_mm_group_accumulate_and_grad_out(monkeypatch):
    metas = _metas(MECH, [200, 17, 901], [30, 64, 7])
    model = _model(metas[0])
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


def _stacked(patients):
    path = (torch.cat([p["path_features"] for p in patients]), [int(p["path_features"].shape[0]) for p in patients])
    radio = (torch.stack([torch.cat([p[m] for p in patients]) for m in cases.MODS]),
             [int(p["T1"].shape[0]) for p in patients])
    omic = torch.stack([p["genomic_features"] for p in patients])
    return path, radio, omic


def test_mm_group_pre_stacked_equals_dicts_and_explicit_seeds(monkeypatch):
    metas = _metas(MECH, [65, 130], [12, 300])
    model = _model(metas[0])
    patients = [_patient(m) for m in metas]
    a = run_group(metas, monkeypatch, 1.0, model=model, patients=patients)
    ga = {k: p.grad.clone() for k, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    b = run_group(metas, monkeypatch, 1.0, model=model, patients=_stacked(patients))
    # ... and the seeds handed in instead of drawn
    for p in model.parameters():
        p.grad = None
    c = run_group(metas, monkeypatch, 1.0, model=model, patients=patients,
                  seeds={k: [m["seeds"][k] for m in metas] for k in BRANCHES})
    for r in (b, c):
        for k in ("hazards", "S", "loss", "risk", "Y_hat"):
            assert np.array_equal(r[k], a[k]), k
        for k in a["A"]:
            assert all(np.array_equal(x, y) for x, y in zip(r["A"][k], a["A"][k])), k
        for k, v in ga.items():
            assert np.array_equal(r["grads"][k], v.cpu().numpy()), k


def test_mm_group_repeat_is_bit_identical_and_leaves_sync_words_zero(monkeypatch):
    from multimodalfusion_amd import ops
    metas = _metas(MECH, [300, 12, 99], [5, 77, 210])
    runs = [run_group(metas, monkeypatch, 0.5) for _ in range(2)]
    for k in ("hazards", "S", "loss", "risk"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    for k, v in runs[0]["grads"].items():
        assert np.array_equal(v, runs[1]["grads"][k]), k
    torch.cuda.synchronize()
    assert int(ops.sync_words(torch.device(DEV)).abs().sum()) == 0


@pytest.mark.parametrize("mode", ["radio_path_omic", "path_omic"])
def test_mm_group_on_poisoned_memory(mode, poison, monkeypatch):  # noqa: F811
    """Workspaces and outputs pre-filled with NaN: every output finite, every gradient equal to the clean run's."""
    metas = _metas(dict(MECH, mode=mode), [150, 9, 1100], [40, 3, 90])
    clean = run_group(metas, monkeypatch, 0.5)
    got = poison.run("nan", run_group, metas, monkeypatch, 0.5)
    for k in ("hazards", "S", "loss", "risk"):
        assert np.isfinite(got[k]).all(), k
        assert np.array_equal(got[k], clean[k]), k
    for k in got["A"]:
        assert all(np.isfinite(a).all() for a in got["A"][k]), k
    for k, v in clean["grads"].items():
        assert np.isfinite(got["grads"][k]).all(), k
        assert np.array_equal(got["grads"][k], v), k


def test_mm_group_rejects_bad_calls(monkeypatch):
    """Argument checks: each raises before anything is launched, and a valid call afterwards still works."""
    from multimodalfusion_amd import _lib, ops
    metas = _metas(MECH, [64, 64], [8, 8])
    model = _model(metas[0])
    patients = [_patient(m) for m in metas]
    Y, c = _labels(metas)
    launches = []
    real = ops.stream_ptr
    monkeypatch.setattr(ops, "stream_ptr", lambda: launches.append(1) or real())     # every C-ABI launch asks for the stream

    def refused(exc, pts, Y=Y, c=c, model=model, **kw):
        n = len(launches)
        with pytest.raises(exc):
            model.nll_step_group(pts, Y, c, **kw)
        assert len(launches) == n, "a refused call launched something"

    tens = _model(dict(metas[0], fusion="tensor"))
    refused(NotImplementedError, patients, model=tens)                       # tensor fusion
    bf = [dict(p, path_features=p["path_features"].to(torch.bfloat16)) for p in patients]
    refused((TypeError, _lib.MmfError), bf)                                  # bf16 bags
    one = patients[0]
    refused(_lib.MmfError, [one] * 65, Y=[0] * 65, c=[0.0] * 65)             # G = 65
    empty = [patients[0], dict(patients[1], path_features=patients[1]["path_features"][:0])]
    refused(_lib.MmfError, empty)                                            # an empty bag
    path, radio, omic = _stacked(patients)
    refused(_lib.MmfError, (path, radio, omic[:1]))                          # patient counts differ between branches
    refused(_lib.MmfError, ((path[0], [128]), radio, omic))
    k33 = _model(dict(metas[0], K=33))
    refused(_lib.MmfError, patients, model=k33)                              # K = 33
    prev = ops.set_gemm(1)
    try:
        refused(_lib.MmfError, patients)                                     # bf16x3 GEMMs
    finally:
        ops.set_gemm(prev)
    _seed_stream(monkeypatch, metas)
    hz, *_ = model.nll_step_group(patients, Y, c)                            # still fine afterwards
    torch.cuda.synchronize()
    assert launches and bool(torch.isfinite(hz).all())


# ---- the raw entry points on their own ------------------------------------------------------------------------------
@pytest.mark.parametrize("F,K,G", [(768, 4, 16), (100, 1, 3), (1024, 32, 64), (7, 3, 1)])
def test_surv_head_nll_step_group_shapes(F, K, G):
    """mmf_surv_head_nll_step_group against torch autograd in fp64, at the bars of test_surv_head_nll_step_shapes."""
    from multimodalfusion_amd import ops
    # loss_scale = 1 / G, the scale of an accumulation window: dWk is a sum of G fp32 slabs, and with terms of size
    # |dlogits| |feat| / G its rounding (G roundings of 6e-8 relative each) stays inside that test's atol = 1e-6
    alpha, scale = 0.3, 1.0 / G
    feat = gen.normal(10, (G, F), stream=F)
    Wk = gen.normal(11, (K, F), stream=K, std=1.0 / np.sqrt(F))
    bk = gen.normal(12, (K,), stream=3, std=0.1)
    Y = [(3 * g + 1) % K for g in range(G)]
    c = [float(g % 2) for g in range(G)]
    dWk, dbk = torch.full((K, F), 7.0, device=DEV), torch.full((K,), 7.0, device=DEV)
    # feat as columns of a wider matrix, as the model hands it over
    wide = torch.full((G, F + 5), float("nan"), device=DEV)
    wide[:, 2:2 + F] = _t(feat)
    hz, S, Yh, loss, risk, dfeat = ops.surv_head_nll_step_group(wide[:, 2:2 + F], _t(Wk), _t(bk), torch.tensor(Y),
                                                                torch.tensor(c), alpha, dWk, dbk, loss_scale=scale)
    base = dWk.clone()
    ops.surv_head_nll_step_group(wide[:, 2:2 + F], _t(Wk), _t(bk), torch.tensor(Y), torch.tensor(c), alpha, dWk, dbk,
                                 loss_scale=scale, accumulate=True)
    torch.cuda.synchronize()
    rf, rW, rb = (torch.as_tensor(a).double().requires_grad_(True) for a in (feat, Wk, bk))
    rhz = torch.sigmoid(torch.nn.functional.linear(rf, rW, rb))
    rS = torch.cumprod(1 - rhz, dim=1)
    losses = torch.stack([tp.nll_loss(rhz[g:g + 1], rS[g:g + 1], torch.tensor([Y[g]]), torch.tensor([c[g]]), alpha=alpha)
                          for g in range(G)])
    (losses.sum() * scale).backward()
    lref = losses.detach().numpy()
    assert (np.abs(loss.cpu().numpy() - lref) <= 1e-5 * np.maximum(1.0, np.abs(lref))).all()
    np.testing.assert_allclose(hz.cpu().numpy(), rhz.detach().numpy(), rtol=0, atol=1e-6)
    # S: a product of K <= 32 fp32 factors, each rounded once (6e-8): 2e-6; risk: a sum of K of them
    np.testing.assert_allclose(S.cpu().numpy(), rS.detach().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(risk.cpu().numpy(), -rS.detach().numpy().sum(1), rtol=0, atol=1e-4)
    assert np.array_equal(Yh.cpu().numpy().reshape(-1), rhz.detach().numpy().argmax(1))
    for got, ref in ((dfeat, rf.grad), (base, rW.grad), (dbk * 0.5, rb.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dWk.cpu().numpy(), 2 * base.cpu().numpy(), rtol=1e-6, atol=1e-12)    # accumulate adds


@pytest.mark.parametrize("kind,act,p", [("alpha", "selu", 0.25), ("dropout", "relu", 0.25), ("none", "selu", 0.0)])
def test_dense_rows_equal_one_row_calls(kind, act, p):
    """mmf_dense_forward_rows / _backward_rows on a G-row batch against G one-row mmf_dense_* calls with seed_g: the same
    masks to the bit (so the same outputs to the bit), dx to the bit, dW / db within fp32 rounding of the sum."""
    from multimodalfusion_amd import _lib, ops
    G, K, N, site = 9, 80, 256, 1
    seeds = [0, 1, 0xFFFFFFFF, 0x9E3779B1] + [1234567 * g + 89 for g in range(5)]
    base = ops.dropout_row_base(seeds, DEV)
    assert [int(v) & 0xFFFFFFFF for v in base.cpu().tolist()] == [_lib.lib().mmf_dropout_row_base(s) for s in seeds]
    x, W, b = _t(gen.normal(1, (G, K), stream=1)), _t(gen.normal(2, (N, K), stream=2, std=0.1)), _t(gen.normal(3, (N,), stream=3))
    wide = torch.zeros((G, N + 8), device=DEV)
    y = ops._dense_rows_fwd_raw(x, W, b, act, kind, p, site, base, out=wide[:, 4:4 + N])
    gwide = torch.zeros((G, N + 3), device=DEV)
    gwide[:, 1:1 + N] = _t(gen.normal(4, (G, N), stream=4))
    gy = gwide[:, 1:1 + N]
    dx, dW, db = ops._dense_rows_bwd_raw(gy, y, x, W, True, act, kind, p, site, base)
    dWs, dbs = torch.zeros_like(W, dtype=torch.float64), torch.zeros_like(b, dtype=torch.float64)
    for g in range(G):
        y1 = ops._dense_fwd_raw(x[g:g + 1].contiguous(), W, b, act, kind, p, seeds[g], site)
        assert torch.equal(y1, y[g:g + 1]), g                       # bit-equal masks and values
        dx1, dW1, db1 = ops._dense_bwd_raw(gy[g:g + 1].contiguous(), y1, x[g:g + 1].contiguous(), W, True, act, kind, p,
                                           seeds[g], site)
        assert torch.equal(dx1, dx[g:g + 1]), g
        dWs += dW1.double()
        dbs += db1.double()
    if kind != "none":                                              # the masks are there
        assert not torch.equal(y, ops._dense_rows_fwd_raw(x, W, b, act, "none", 0.0, site, base))
    for got, ref in ((dW, dWs), (db, dbs)):
        tol = 1e-6 * float(ref.abs().max()) * G
        assert float((got.double() - ref).abs().max()) <= tol
    torch.cuda.synchronize()
