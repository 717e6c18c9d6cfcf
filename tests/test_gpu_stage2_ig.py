"""GPU: integrated gradients of the stage-2 fusion models in one call (include/mmf_amil.h: mmf_stage2_ig) against the float64
oracle of tests/stage2_ig_cases.py, the autograd definition on the GPU, the models' own eval forward, a patient alone, itself
(bit for bit), poisoned memory and the launch list."""
import numpy as np
import pytest
import torch

import stage2_ig_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = [c.name for c in sc.CASES]


def _n(t):
    return t.detach().double().cpu().numpy()


def _setup(name):
    c = sc.BY_NAME[name]
    model, _ = sc.make_model(c)
    x = {n: torch.as_tensor(v).to(DEV) for n, v in sc.inputs(c).items()}
    return c, model.to(DEV).eval(), x


def _call(c, model, x, full, rows=None):
    hs = {("h_" + n): (v if rows is None else v[rows].contiguous()) for n, v in x.items()}
    return model.integrated_gradients(n_steps=c.n_steps, method=c.method, return_full=full, **hs)


def _arrays(c, out):
    ns = sc.names(c.mode)
    return (None if out.attr is None else {n: _n(out.attr[n]) for n in ns},
            np.stack([_n(out.modality_attr[n]) for n in ns], 1), np.stack([_n(out.modality_abs[n]) for n in ns], 1))


@pytest.mark.parametrize("name", NAMES)
def test_against_the_float64_oracle_with_and_without_the_full_attribution(name):
    c, model, x = _setup(name)
    o = sc.oracle(name)
    full, lean, again = _call(c, model, x, True), _call(c, model, x, False), _call(c, model, x, True)
    attr, msum, mabs = _arrays(c, full)
    ok, worst = sc.match(name, attr, msum, mabs)
    print(f"{name}: worst ratio to the bar {worst:.3f}; flagged {sum(len(v) for v in o.flagged.values())}")
    assert ok, worst
    _, lsum, labs = _arrays(c, lean)
    assert lean.attr is None and np.array_equal(lsum, msum) and np.array_equal(labs, mabs)     # bit-identical sums
    for n in sc.names(c.mode):                                                                     # two calls, bit for bit
        assert torch.equal(full.attr[n], again.attr[n]) and torch.equal(full.modality_abs[n], again.modality_abs[n])
    assert torch.equal(full.step_risk, again.step_risk) and torch.equal(full.risk, again.risk)
    for got, want in ((full.risk, o.risk), (full.risk_baseline, o.risk_base), (full.step_risk, o.step_risk)):
        assert np.abs(_n(got) - want).max() <= 1e-4
    if c.family == "nll":
        assert np.abs(_n(full.hazards) - o.hazards).max() <= 1e-4 and np.abs(_n(full.S) - o.S).max() <= 1e-4
    else:
        assert full.hazards is None and full.S is None
    delta = msum.sum(1) - (_n(full.risk) - _n(full.risk_baseline))
    assert np.abs(_n(full.delta) - delta).max() <= 1e-5
    share = sum(_n(v) for v in full.share.values())
    assert np.abs(share - 1).max() <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_against_autograd_on_the_gpu_and_the_models_own_forward(name):
    from multimodalfusion_amd import infer
    c, model, x = _setup(name)
    o = sc.oracle(name)
    out = _call(c, model, x, True)
    al, wt = sc.quadrature(c)
    ref, risk_x, risk_base, step_risk = infer.stage2_integrated_gradients_autograd(model, x["radio"], x["path"], x["omic"], al, wt)
    flagged_patients = {p for p, _ in o.flagged}
    clean = np.array([p not in flagged_patients for p in range(c.P)])
    assert clean.sum() >= (c.P + 1) // 2                 # the comparison below never runs on nothing
    for n in sc.names(c.mode):
        bar = 1e-4 * np.abs(o.attr[n]).max()
        assert np.abs(_n(out.attr[n]) - _n(ref[n]))[clean].max() <= 2 * bar           # each within the bar of the oracle
    assert np.abs(_n(out.step_risk) - _n(step_risk)).max() <= 1e-4
    assert np.abs(_n(out.risk_baseline) - _n(risk_base)).max() <= 1e-4
    with torch.no_grad():
        risk, hz, S = model(x["radio"], x["path"], x["omic"])
    assert np.abs(_n(out.risk) - _n(risk.reshape(-1))).max() <= 1e-4 and np.abs(_n(out.risk) - _n(risk_x)).max() <= 1e-4
    if c.family == "nll":
        assert np.abs(_n(out.hazards) - _n(hz)).max() <= 1e-4 and np.abs(_n(out.S) - _n(S)).max() <= 1e-4


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.P > 1])
def test_a_patient_in_the_cohort_against_the_same_patient_alone(name):
    c, model, x = _setup(name)
    p = c.P - 1
    alone = _call(c, model, x, True, rows=[p])
    attr, msum, mabs = _arrays(c, alone)
    ok, worst = sc.match(name, attr, msum, mabs, patients=[p])
    assert ok, worst
    cohort = _call(c, model, x, True)
    if c.train_type != "kronecker":          # the folded chain sums in an order fixed by the element: the same bits
        for n in sc.names(c.mode):
            assert torch.equal(cohort.attr[n][p], alone.attr[n][0])
    assert np.abs(_n(cohort.risk[p]) - _n(alone.risk[0])) <= 1e-4


MODES = {"nan": (float("nan"), 0xFF), "huge": (1e30, 0x7E)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["nll_early_fcnn_rpo", "nll_late_highway_rp_k32_n64", "cox_late_fcnn_rpo_n64",
                                  "nll_kronecker_rp_3x20", "cox_kronecker_ro_p1_k1", "nll_early_highway_ro_p33",
                                  "nll_early_highway_rpo_deep", "cox_late_highway_rp_deep",
                                  "nll_late_highway_po_deep_two_windows"])
def test_poisoned_workspace_and_outputs(name, mode, monkeypatch):
    c, model, x = _setup(name)
    want = _call(c, model, x, True)
    torch.cuda.synchronize()
    f, u8 = MODES[mode]
    empty, filled = torch.empty, [0]

    def poisoned(*a, **kw):
        t = empty(*a, **kw)
        if t.is_cuda and t.numel():
            t.fill_(u8 if t.dtype == torch.uint8 else f if t.is_floating_point() else -1)
            filled[0] += 1
        return t

    monkeypatch.setattr(torch, "empty", poisoned)
    got = _call(c, model, x, True)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert filled[0] >= 4
    for n in sc.names(c.mode):
        assert torch.equal(got.attr[n], want.attr[n]) and torch.equal(got.modality_attr[n], want.modality_attr[n])
        assert torch.equal(got.modality_abs[n], want.modality_abs[n])
    for a, b in ((got.risk, want.risk), (got.risk_baseline, want.risk_baseline), (got.step_risk, want.step_risk)):
        assert torch.equal(a, b)
    if c.family == "nll":
        assert torch.equal(got.hazards, want.hazards) and torch.equal(got.S, want.S)


def _launches(c, model, x):
    from multimodalfusion_amd import _lib
    tr = _lib.KernelTrace()
    try:
        with tr:
            _call(c, model, x, False)
        torch.cuda.synchronize()
        return tr.dump()
    finally:
        tr.close()


FOLDED = {"stage2_fold_fwd_kernel": 1, "stage2_sweep_kernel": 1, "stage2_attr_kernel": 1}


@pytest.mark.parametrize("name", ["nll_early_fcnn_rpo", "cox_late_fcnn_rpo_n64", "nll_early_highway_rpo", "nll_late_highway_rpo_k1"])
def test_folded_types_take_three_launches_whatever_P_and_n_steps_are(name):
    base, model, _ = _setup(name)
    for P, n in ((1, 4), (33, 4), (1, 64), (33, 64)):
        c = base._replace(P=P, n_steps=n)
        x = {k: torch.randn(P, 256, device=DEV) for k in sc.ALL3}
        got = {k: v[0] for k, v in _launches(c, model, x).items()}
        assert got == FOLDED, (P, n, got)


@pytest.mark.parametrize("name", ["nll_kronecker_rpo_5x20", "nll_kronecker_rp_3x20", "cox_kronecker_ro_p1_k1"])
def test_kronecker_takes_seven_tail_launches_per_window_and_no_weight_gradient(name):
    c, model, x = _setup(name)
    got = {k: v[0] for k, v in _launches(c, model, x).items()}
    windows = -(-c.P * (c.n_steps + 2) // 64)
    tail = ("xgate_group_train_kernel", "kron_dense_group_train_kernel", "dense_segs_group_train_kernel",
            "stage2_kron_head_kernel", "dense_bwd_kernel", "kron_dense_dkr_group_kernel", "xgate_bwd_group_kernel")
    want = {k: windows for k in tail + ("stage2_kron_expand_kernel", "stage2_kron_fold_kernel")}
    want["stage2_kron_attr_kernel"] = 1
    assert got == want, got                               # no weight-gradient launch: nothing else runs


@pytest.mark.parametrize("name", ["nll_early_highway_rpo_deep", "cox_late_highway_rp_deep", "nll_late_highway_po_deep_two_windows"])
def test_deep_highways_run_the_row_kernels_per_window_and_no_weight_gradient(name):
    c, model, x = _setup(name)
    got = {k: v[0] for k, v in _launches(c, model, x).items()}
    windows = -(-c.P * (c.n_steps + 2) // 256)
    per = (c.n_layers - 1) * (len(sc.names(c.mode)) if "late" in c.train_type else 1)      # (layer >= 1, Highway) pairs
    want = {"stage2_fold_fwd_kernel": 1, "stage2_attr_kernel": 1, "stage2_hw_begin_kernel": windows,
            "stage2_hw_head_kernel": windows, "stage2_hw_end_kernel": windows, "dense_fwd_kernel": 3 * per * windows,
            "highway_fwd_kernel": per * windows, "highway_bwd_kernel": per * windows, "dense_bwd_kernel": 3 * per * windows,
            "stage2_hw_add3_kernel": per * windows}
    assert got == want, got                               # no sweep, no dense_dw_kernel, nothing else


def test_attribute_embeddings_averages_duplicate_subject_ids():
    from multimodalfusion_amd import infer
    c, model, x = _setup("nll_early_fcnn_rpo")
    ids = ["b", "a", "b", "c", "a"]
    plain = infer.attribute_embeddings(model, x["radio"], x["path"], x["omic"], n_steps=c.n_steps)
    out = infer.attribute_embeddings(model, x["radio"], x["path"], x["omic"], subject_ids=ids, n_steps=c.n_steps)
    assert list(out["subject_id"]) == ["a", "b", "c"] and plain["subject_id"] is None
    assert set(out["attr"]) == set(out["attr_orig"]) == {"radio_attr", "path_attr", "omic_attr"}
    o = sc.oracle(c.name)
    for i, n in enumerate(sc.names(c.mode)):
        for key, ref in (("attr", o.mod_abs), ("attr_orig", o.mod_sum)):
            v = plain[key][n + "_attr"]
            assert np.abs(v - ref[:, i]).max() <= 1e-4 * np.abs(ref).max()
            want = [(v[1] + v[4]) / 2, (v[0] + v[2]) / 2, v[3]]
            assert np.allclose(out[key][n + "_attr"], want, rtol=1e-12, atol=0)
    model.train()
    infer.attribute_embeddings(model, x["radio"], x["path"], x["omic"], n_steps=4)       # eval for the call, restored
    assert model.training


@pytest.mark.parametrize("name", ["nll_late_fcnn_po_one_node", "cox_late_highway_ro_middle", "nll_kronecker_rp_3x20",
                                  "cox_early_fcnn_rp_p33", "nll_late_highway_rpo_k1"])
def test_captum_methods_return_forwards_risk_and_carry_gradients(name):
    c, model, x = _setup(name)
    ns = sc.names(c.mode)
    method = {("radio", "path"): "captum_radio_path", ("omic", "path"): "captum_path_omic",
              ("radio", "omic"): "captum_radio_omic", ("radio", "path", "omic"): "captum"}[tuple(ns)]
    args = [x[n].clone().requires_grad_() for n in ns]          # the reference's orders: note captum_path_omic(h_omic, h_path)
    risk = getattr(model, method)(*args)
    with torch.no_grad():
        want = model(x["radio"], x["path"], x["omic"])[0]
    assert np.abs(_n(risk.reshape(-1)) - _n(want.reshape(-1))).max() <= 1e-5
    grads = torch.autograd.grad(risk.sum(), args)
    assert all(g.shape == a.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g, a in zip(grads, args))


def test_refusals_of_the_python_surface():
    c, model, x = _setup("nll_early_fcnn_rpo")
    model.train()
    with pytest.raises(RuntimeError):
        _call(c, model, x, False)
    model.eval()
    with pytest.raises(NotImplementedError):
        model.integrated_gradients(x["radio"].double(), x["path"], x["omic"])
    with pytest.raises(ValueError):
        model.integrated_gradients(x["radio"], x["path"], x["omic"], method="riemann_left")
