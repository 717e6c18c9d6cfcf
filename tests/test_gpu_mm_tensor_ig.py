"""GPU: integrated-gradients attribution of the multimodal tensor-fusion head in one call (include/mmf_amil.h:
mmf_mm_ig_tensor; ops.mm_integrated_gradients(xfusion=...), MM_MIL_Attention_fc_surv.integrated_gradients_tensor,
infer.attribute_modalities) against the float64 oracle of tests/mm_tensor_ig_cases.py -- integrated gradients by the
definition over oracle.torch_port.mm_forward(fusion="tensor") -- under that module's combination rule for tail units on a
kink and its plain bars; tier C (the shipped widths) also against the autograd route on the GPU; and the structure of the
call: determinism, windows, the launch list per mode with its seven tail launches per window and no weight-gradient
launch, poisoned memory, absent branches, the head's outputs and the per-node risks against the model's forward."""
import ctypes as C

import numpy as np
import pytest
import torch

import mm_ig_cases as mc
import mm_tensor_ig_cases as tc
from test_gpu_mm_ig import MODS, _from_model, _np, _pack, _stack, _worst
from test_gpu_path import DEV, _load

pytestmark = pytest.mark.gpu


def _xweights(sd, m):
    t = lambda k: torch.as_tensor(sd[k]).to(DEV)
    w = []
    for i in range(m):
        for j in range(3):
            w += [t(f"mm.reduce.{i}.{j}.0.weight"), t(f"mm.reduce.{i}.{j}.0.bias")]
    return w + [t("mm.encoder1.0.weight"), t("mm.encoder1.0.bias"), t("mm.encoder2.0.weight"), t("mm.encoder2.0.bias")]


def _operands(name):
    """(case, the branches in column order, classifier[3], the xfusion triple) as ops.mm_integrated_gradients takes them."""
    c = tc.BY_NAME[name]
    sd, xs, _ = tc.inputs(name)
    t = lambda k: torch.as_tensor(sd[k]).to(DEV)
    dev = lambda a: torch.as_tensor(np.array(a)).to(DEV)
    branches = []
    for b in tc.order(c.mode):
        if b == "path":
            branches.append(("path", dev(xs["path"]), _stack(sd, mc.PRE_P, c.path.gated), c.path.gated))
        elif b == "radio":
            branches.append(("radio", [dev(x) for x in xs["radio"]], t("reduce_dim.weight"), t("reduce_dim.bias"),
                             _stack(sd, mc.PRE_R, c.radio.gated), c.radio.gated))
        else:
            branches.append(("omic", dev(xs["omic"]), t("fc_omic.0.0.weight"), t("fc_omic.0.0.bias"), t("fc_omic.1.0.weight"),
                             t("fc_omic.1.0.bias")))
    xf = (_xweights(sd, len(branches)), t("classifier.0.weight"), t("classifier.0.bias"))
    return c, branches, t("classifier.3.weight"), t("classifier.3.bias"), xf


def _run(name, want_attr=False, window_steps=None):
    from multimodalfusion_amd import ops
    c, branches, Wk, bk, xf = _operands(name)
    a, w = ops.ig_quadrature(c.method, c.n_steps)
    out = ops.mm_integrated_gradients(branches, Wk, bk, a, w, want_attr=want_attr,
                                      window_steps=c.window_steps if window_steps is None else window_steps, xfusion=xf)
    torch.cuda.synchronize()
    return _pack(*out)


def _check(res, o, tag):
    """The combination rule on every array of the call at once, then the sums and the risks; prints each figure first."""
    pick, worst = tc.match(o, res["attr"], res["row_sum"], res["row_abs"])
    flagged = {k: v for k, v in o.flagged.items()}
    print(f"{tag}: flagged tail units {flagged}; combination {pick}; worst err / bar {worst:.3f}")
    for b in o.attr:
        plain = np.abs(res["row_abs"][b] - o.row_abs[b]).max() / (1e-4 * np.abs(o.row_abs[b]).max())
        print(f"{tag} {b} row_abs against float64's own assignment: err / plain bar {plain:.3f}")
    assert pick is not None, (tag, worst)
    assert abs(res["risk"] - o.risk) <= 1e-4 and abs(res["risk_base"] - o.risk_base) <= 1e-4, tag
    err = np.abs(res["step_risk"] - o.step_risk).max()
    print(f"{tag} risk {res['risk']:.6f} / {o.risk:.6f}; step_risk max err {err:.3e}")
    np.testing.assert_allclose(res["step_risk"], o.step_risk, rtol=0, atol=1e-4, err_msg=tag)
    np.testing.assert_allclose(res["hazards"], o.hazards, rtol=0, atol=1e-4, err_msg=tag)
    np.testing.assert_allclose(res["S"], o.S, rtol=0, atol=1e-4, err_msg=tag)
    return pick


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_case_matches_the_oracle_with_and_without_the_full_attribution(name):
    c = tc.BY_NAME[name]
    o = tc.oracle(name)
    full, rows = _run(name, want_attr=True), _run(name, want_attr=False)
    assert set(full["attr"]) == set(tc.order(c.mode))
    for b in full["attr"]:
        assert full["attr"][b].shape == o.attr[b].shape and full["row_sum"][b].shape == o.row_sum[b].shape, b
    _check(full, o, name)
    # attr == NULL only drops the stores: the sums are the same additions
    for b in full["attr"]:
        for key in ("row_sum", "row_abs"):
            np.testing.assert_array_equal(full[key][b], rows[key][b], err_msg=f"{b} {key}")
        if b != "omic":
            assert rows["attr"][b] is None
    np.testing.assert_array_equal(full["step_risk"], rows["step_risk"])
    assert full["risk"] == rows["risk"] and full["risk_base"] == rows["risk_base"]


def _model(name):
    """The case as a model with its inputs: the stock class, its modules replaced by ones of the case's widths."""
    from torch import nn
    from multimodalfusion_amd.models.model_modules import Attn_Net, Attn_Net_Gated, SNN_Block
    from multimodalfusion_amd.models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    c = tc.BY_NAME[name]
    sd, xs, _ = tc.inputs(name)
    mods = MODS[:c.radio.nseg] if c.radio else MODS
    m = MM_MIL_Attention_fc_surv(input_dim=c.omic.Gin if c.omic else 80, fusion="tensor", gate_path=c.path.gated if c.path else True,
                                 gate_radio=c.radio.gated if c.radio else True, dropout=False, n_classes=c.K, mode=c.mode)
    dev = lambda a: torch.as_tensor(np.array(a)).to(DEV)
    feats = {}
    if c.radio:
        feats.update({k: dev(x) for k, x in zip(mods, xs["radio"])})
    if c.path:
        feats["path_features"] = dev(xs["path"])
    if c.omic:
        feats["genomic_features"] = dev(xs["omic"])
    if c.tier == "C":
        return c, _load(m, sd).eval(), feats

    def stack(L, H, D, gated):
        att = (Attn_Net_Gated if gated else Attn_Net)(L=H, D=D, dropout=False, n_classes=1)
        return nn.Sequential(nn.Linear(L, H), nn.ReLU(), nn.Dropout(0.25), att)
    from multimodalfusion_amd.models.model_modules import XlinearFusion
    m.modalities = mods
    m.mm = XlinearFusion(dim=tc.dim(c), scale_dim=16, mmhid1=c.tail.mmhid1, mmhid2=c.tail.mmhid2,
                         num_modalities=len(tc.order(c.mode)), gate=True, skip=1)
    m.classifier = nn.Sequential(nn.Linear(c.tail.mmhid2, c.tail.nhid), nn.ReLU(), nn.Dropout(0.25), nn.Linear(c.tail.nhid, c.K))
    if c.omic:
        m.fc_omic = nn.Sequential(SNN_Block(dim1=c.omic.Gin, dim2=c.omic.W0), SNN_Block(dim1=c.omic.W0, dim2=c.omic.We, dropout=0.25))
    if c.radio:
        m.attention_net_radio = stack(c.radio.kseg, c.radio.H, c.radio.D, c.radio.gated)
        m.reduce_dim = nn.Linear(c.radio.kseg * c.radio.nseg, c.radio.kseg)
    if c.path:
        m.attention_net_WSI = stack(c.path.L, c.path.H, c.path.D, c.path.gated)
    res = m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys
    return c, m.to(DEV).eval(), feats


@pytest.mark.parametrize("name", [c.name for c in tc.TIER_C])
def test_shipped_width_matches_the_oracle_and_the_autograd_route(name):
    from multimodalfusion_amd import infer, ops
    c, model, feats = _model(name)
    o = tc.oracle(name)
    out = model.integrated_gradients_tensor(n_steps=c.n_steps, method=c.method, return_full=True, **feats)
    torch.cuda.synchronize()
    res = _from_model(out)
    pick = _check(res, o, name)
    for b in ("radio", "path", "omic"):
        if b not in o.attr:
            assert out.modality_abs[b] is None and out.modality_attr[b] is None and out.share[b] is None
            continue
        assert abs(float(out.modality_abs[b]) - res["row_abs"][b].sum()) <= 1e-5 * o.total_abs
        assert abs(float(out.share[b]) - float(out.modality_abs[b]) / float(out.total_abs)) <= 1e-6
    assert abs(float(out.delta) - (float(out.total) - (res["risk"] - res["risk_base"]))) <= 1e-6
    # infer.attribute_modalities routes a tensor model to the same call
    via = infer.attribute_modalities(model, feats, n_steps=c.n_steps, method=c.method)
    for b, key in (("path", "patch_abs"), ("omic", "gene_attr")):
        assert torch.equal(getattr(via, key), getattr(out, key)), key
    # the autograd route on the GPU, the same fp32 inputs: 1e-4 * max plus the largest single flagged unit's term -- a stack
    # or omic unit's allowance (allow_max), and a flagged tail unit's whole change of the array (the two routes may sit on
    # different sides of it)
    a, w = ops.ig_quadrature(c.method, c.n_steps)
    attrs, risk, base, steps = infer.mm_integrated_gradients_autograd(model, feats, a.astype(np.float32), w.astype(np.float32))
    torch.cuda.synchronize()
    single = {b: np.zeros(v.shape) for b, v in o.attr.items()}
    for _, opts in o.alt:
        for bits, d in opts:
            for b in d:
                np.maximum(single[b], np.abs(d[b]), out=single[b])
    for b, ref in attrs.items():
        ref = _np(ref)
        bar = 1e-4 * np.abs(ref).max() + o.allow_max[b] + single[b]
        ratio, k, err = _worst(res["attr"][b], ref, bar)
        plain = np.abs(res["attr"][b] - ref).max() / (1e-4 * np.abs(ref).max())
        print(f"{name} vs autograd {b} attr: max err {err:.3e}, err / bar {ratio:.3f}, err / tight bar {plain:.3f}")
        assert ratio <= 1.0, (name, b, k)
    assert abs(res["risk"] - float(risk)) <= 1e-5 and abs(res["risk_base"] - float(base)) <= 1e-5
    np.testing.assert_allclose(res["step_risk"], _np(steps), rtol=0, atol=1e-5)


def _same(a, b, tag):
    for key in ("row_sum", "row_abs", "attr"):
        for br in a[key]:
            np.testing.assert_array_equal(a[key][br], b[key][br], err_msg=f"{tag} {br} {key}")
    np.testing.assert_array_equal(a["step_risk"], b["step_risk"], err_msg=tag)
    assert a["risk"] == b["risk"] and a["risk_base"] == b["risk_base"], tag


def test_two_calls_agree_bit_for_bit():
    for name, ws in (("t_rpo_shipped_tail", 0), ("t_rp_remainders_k1", 3), ("t_po_omic_first_k32", 0), ("t_rp_widest_row", 0)):
        _same(_run(name, True, ws), _run(name, True, ws), name)


def test_windows_of_one_three_and_all_nodes_agree():
    """20 nodes + the two riders in windows of 1, 3 and one window: each within the bar of a combination, and node k's risk at
    place k whatever window ran it.  The tail gives a node the same bits whatever its window holds (one output, one wave, one
    order); the stacks' pooling groups depend on the window's rows, so the arrays agree to the bar, not bit for bit."""
    name = "t_rpo_shipped_tail"
    o = tc.oracle(name)
    runs = {ws: _run(name, True, ws) for ws in (1, 3, 0)}
    for ws, r in runs.items():
        _check(r, o, f"{name} window_steps={ws}")
    for ws in (1, 3):
        np.testing.assert_allclose(runs[ws]["step_risk"], runs[0]["step_risk"], rtol=0, atol=1e-5)
        assert abs(runs[ws]["risk"] - runs[0]["risk"]) <= 1e-5 and abs(runs[ws]["risk_base"] - runs[0]["risk_base"]) <= 1e-5
        # array against array: the plain bar of each run, plus the whole change a flagged unit can make where the two runs'
        # pre-activations, which differ by the pooling groups' rounding, sit on different sides of it
        single = {b: np.zeros(v.shape) for b, v in o.attr.items()}
        for _, opts in o.alt:
            for _, d in opts:
                for b in d:
                    np.maximum(single[b], np.abs(d[b]), out=single[b])
        for b in o.attr:
            d = np.abs(runs[ws]["attr"][b] - runs[0]["attr"][b])
            tight = d.max() / (1e-4 * np.abs(o.attr[b]).max())
            print(f"window_steps {ws} vs 0 {b}: max |d attr| {d.max():.3e}, of the plain bar {tight:.3f}")
            assert (d <= 2 * o.bar_attr[b] + single[b]).all(), (ws, b)


def _traced(name, window_steps=None):
    from multimodalfusion_amd import _lib
    t = _lib.KernelTrace()
    try:
        with t:
            _run(name, False, window_steps)
        return t.dump()
    finally:
        t.close()


STACK_WINDOW = ("ig_expand_kernel", "group_rows_kernel", "gate_fwd_kernel", "group_pool_partial_kernel", "group_merge_kernel",
                "group_dm_gather_kernel", "group_bwd_prep_kernel", "bwd_dh_kernel", "ig_fold_kernel")
OMIC_WINDOW = ("ig_omic_fwd_kernel", "ig_omic_bwd_kernel", "ig_omic_fold_kernel")
TAIL_WINDOW = ("xgate_group_train_kernel", "kron_dense_group_train_kernel", "dense_segs_group_train_kernel",
               "xfusion_ig_head_kernel", "dense_bwd_kernel", "kron_dense_dkr_group_kernel", "xgate_bwd_group_kernel")
ONCE = {"path": {"linear_nt_kernel": 1, "gemm_nn_attr_kernel": 1, "ig_rows_kernel": 1},
        "radio": {"linear_nt_kernel": 2, "ig_bias_kernel": 1, "gemm_nn_kernel": 1, "gemm_nn_attr_seg_kernel": 1, "ig_rows_seg_kernel": 1},
        "omic": {"ig_omic_z_kernel": 1, "ig_omic_attr_kernel": 1}}


def _expected(mode, windows=1, folds=1):
    want = {n: windows for n in TAIL_WINDOW}
    for b in tc.order(mode):
        for n, cnt in ONCE[b].items():
            want[n] = want.get(n, 0) + cnt
        for n in (OMIC_WINDOW if b == "omic" else STACK_WINDOW):
            want[n] = want.get(n, 0) + (folds if "fold" in n else windows)
    return want


def _no_weight_gradient(k):
    assert not any(n in k for n in ("kron_dense_dw_group_kernel", "xgate_dw_group_kernel", "add_into_kernel", "ig_head_kernel",
                                    "dense_dw_kernel")), sorted(k)
    assert not any("tn_kernel" in n or "reduce" in n for n in k), sorted(k)


@pytest.mark.parametrize("name", ["t_rpo_shipped_tail", "t_rp_remainders_k1", "t_ro_one_row", "t_po_omic_first_k32"])
def test_launch_list_per_mode(name):
    """Per mode: each present branch's once-per-call and window launches as in the concat call, SEVEN tail launches per window
    where that call has its one head launch, and no weight-gradient, TN, add-into or reduce launch."""
    c = tc.BY_NAME[name]
    k = {n: v[0] for n, v in _traced(name).items()}
    print(name, sorted(k.items()))
    assert k == _expected(c.mode), name
    assert sum(k[n] for n in TAIL_WINDOW) == 7
    _no_weight_gradient(k)


def test_launch_list_over_several_windows():
    k = {n: v[0] for n, v in _traced("t_po_one_step_windows").items()}
    assert k == _expected("path_omic", windows=3, folds=1), sorted(k.items())
    _no_weight_gradient(k)
    # 64 nodes in a window of 64, the riders alone in the second: nothing to fold there
    k = {n: v[0] for n, v in _traced("t_rp_riders_alone").items()}
    assert k == _expected("radio_path", windows=2, folds=1), sorted(k.items())
    # 20 + 2 in windows of 17: one patient past the dkr launch's group of 16
    k = {n: v[0] for n, v in _traced("t_po_window_17").items()}
    assert k == _expected("path_omic", windows=2, folds=2), sorted(k.items())
    assert sum(k[n] for n in TAIL_WINDOW) == 14


def _raw(name, fill, want_attr):
    """The raw call on a workspace (with a guard band of 64 words on either side) and outputs filled with `fill` first, with
    the head's optional outputs and, for an absent branch, output buffers it must not touch."""
    from multimodalfusion_amd import _lib, ops
    c, branches, Wk, bk, (xweights, Wc0, bc0) = _operands(name)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature(c.method, c.n_steps))
    fp = C.POINTER(C.c_float)
    mm = _lib.MmIgDesc(n_steps=c.n_steps, window_steps=c.window_steps, alpha=a.ctypes.data_as(fp), weight=w.ctypes.data_as(fp))
    full = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=DEV)
    keep, bufs, F = [], {}, 0
    q = dict(Np=0, Lp=0, Hp=0, Dp=0, gp=0, Nr=0, nseg=0, kseg=0, Hr=0, Dr=0, gr=0, Gin=0, W0=0, We=0)
    for b in branches:
        if b[0] == "path":
            x, (stack, _, H, D) = b[1], ops._stack_operands(b[2], b[1].shape[1], None, "bag")
            N, L = x.shape
            d = ops._amil_desc(stack, N, L, H, D, b[3], 0.0, 0.0, 0, None)
            bufs["path"] = (full(N + 4), full(N + 4), full(N, L))
            mm.path, mm.path_x, mm.path_col = C.pointer(d), x.data_ptr(), F
            q.update(Np=N, Lp=L, Hp=H, Dp=D, gp=d.gated)
            keep += [d, stack]
            F += H
        elif b[0] == "radio":
            xs, N, nseg, kseg, rd = ops._radio_operands(b[1], b[2], b[3], "pass")
            stack, _, H, D = ops._stack_operands(b[4], kseg, None, "bags")
            d = ops._amil_desc(stack, N, kseg, H, D, b[5], 0.0, 0.0, 0, None)
            bufs["radio"] = (full(nseg * N + 4), full(nseg * N + 4), full(nseg, N, kseg))
            mm.radio, mm.rd, mm.radio_col = C.pointer(d), C.pointer(rd), F
            q.update(Nr=N, nseg=nseg, kseg=kseg, Hr=H, Dr=D, gr=d.gated)
            keep += [d, rd, xs, stack]
            F += H
        else:
            _, x, W0, b0, W1, b1 = b
            bufs["omic"] = (full(x.numel() + 4),)
            mm.omic_x, mm.omic_W0, mm.omic_b0, mm.omic_W1, mm.omic_b1 = (t.data_ptr() for t in (x, W0, b0, W1, b1))
            mm.omic_Gin, mm.omic_W0n, mm.omic_We, mm.omic_col = x.numel(), W0.shape[0], W1.shape[0], F
            q.update(Gin=x.numel(), W0=W0.shape[0], We=W1.shape[0])
            F += W1.shape[0]
    absent = {b: (full(64), full(64), full(64)) for b in ("path", "radio", "omic") if b not in bufs}
    for b, v in {**bufs, **absent}.items():
        if b == "omic":
            mm.omic_attr = v[0].data_ptr()
        else:
            setattr(mm, b + "_row_sum", v[0].data_ptr())
            setattr(mm, b + "_row_abs", v[1].data_ptr())
            setattr(mm, b + "_attr", v[2].data_ptr() if want_attr or b in absent else None)
    m = len(branches)
    xw, xkeep, (sdim, mmhid1, mmhid2, nhid) = ops._xfusion_operands(m, 1, F // m, xweights, Wc0, bc0, "test")
    K, n = c.K, c.n_steps
    l = _lib.lib()
    nbytes = l.mmf_mm_ig_tensor_workspace_bytes(*q.values(), n, c.window_steps, F // m, sdim, mmhid1, mmhid2, nhid)
    assert nbytes > 0 and nbytes % 256 == 0
    G = 64
    ws = full(nbytes // 4 + 2 * G)
    risks, head = full(2 + n + 4), full(3 * K + 1 + 4)
    yhat = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    mm.risk_x, mm.risk_base, mm.step_risk = risks[0:1].data_ptr(), risks[1:2].data_ptr(), risks[2:].data_ptr()
    sh = _lib.SurvHead(Wk=_lib.ptr(Wk), bk=_lib.ptr(bk), K=K, logits=head[:K].data_ptr(), hazards=head[K:2 * K].data_ptr(),
                       S=head[2 * K:3 * K].data_ptr(), Y_hat=yhat.data_ptr(), risk=head[3 * K:].data_ptr())
    _lib.check(l.mmf_mm_ig_tensor(C.byref(mm), C.byref(xw), ws[G:].data_ptr(), nbytes, C.byref(sh), _lib.stream_ptr()),
               "mmf_mm_ig_tensor")
    torch.cuda.synchronize()
    out = dict(risks=_np(risks[:2 + n]), head=_np(head[:3 * K + 1]), Y_hat=int(yhat[0]),
               guard=np.concatenate([_np(risks[2 + n:]), _np(head[3 * K + 1:]), _np(ws[:G]), _np(ws[G + nbytes // 4:])]
                                    + [_np(v[i][-4:]) for b, v in bufs.items() for i in range(min(2, len(v)))]),
               absent=np.concatenate([_np(t) for v in absent.values() for t in v]) if absent else np.zeros(0))
    for b, v in bufs.items():
        out[b] = [_np(v[0][:-4])] if b == "omic" else [_np(v[0][:-4]), _np(v[1][:-4]), _np(v[2])]
    return out


@pytest.mark.parametrize("name", ["t_rpo_shipped_tail", "t_rp_remainders_k1", "t_ro_one_row", "t_po_omic_first_k32",
                                  "t_po_window_17", "t_rp_widest_row"])
def test_poisoned_workspace_and_outputs_are_overwritten(name):
    """NaN canaries in the workspace, around it and in every output: the outputs come back finite, whole, and bit for bit
    what a zero-filled workspace gives -- nothing is read before the call writes it (the seed table is read and never used)
    -- the guard bands and the words behind the outputs stay, and the outputs of an absent branch keep their poison."""
    c = tc.BY_NAME[name]
    o = tc.oracle(name)
    nan, zero = _raw(name, float("nan"), True), _raw(name, 0.0, True)
    for b in tc.order(c.mode):
        for i, (x, y) in enumerate(zip(nan[b], zero[b])):
            assert np.isfinite(x).all(), (b, i)
            np.testing.assert_array_equal(x, y, err_msg=f"{b} {i}")
    got = {b: (nan[b][0] if b == "omic" else nan[b][2].reshape(o.attr[b].shape)) for b in tc.order(c.mode)}
    rs = {b: (nan[b][0] if b == "omic" else nan[b][0].reshape(o.row_sum[b].shape)) for b in got}
    ra = {b: (np.abs(nan[b][0]) if b == "omic" else nan[b][1].reshape(o.row_abs[b].shape)) for b in got}
    assert tc.match(o, got, rs, ra)[0] is not None, name
    for what in ("risks", "head"):
        assert np.isfinite(nan[what]).all(), what
        np.testing.assert_array_equal(nan[what], zero[what], err_msg=what)
    assert np.isnan(nan["guard"]).all() and (zero["guard"] == 0).all() and nan["Y_hat"] == zero["Y_hat"]
    assert np.isnan(nan["absent"]).all() and (zero["absent"] == 0).all()
    assert (nan["absent"].size > 0) == (len(tc.order(c.mode)) < 3)
    K = c.K
    logits, hz, S, risk = nan["head"][:K], nan["head"][K:2 * K], nan["head"][2 * K:3 * K], nan["head"][3 * K]
    np.testing.assert_allclose(logits, o.logits, rtol=0, atol=1e-4)
    np.testing.assert_allclose(hz, o.hazards, rtol=0, atol=1e-4)
    np.testing.assert_allclose(S, o.S, rtol=0, atol=1e-4)
    assert risk == nan["risks"][0] and abs(risk - o.risk) <= 1e-4
    srt = np.sort(o.logits)
    if K == 1 or srt[-1] - srt[-2] > 2e-4:
        assert nan["Y_hat"] == o.Y_hat


@pytest.mark.parametrize("name", ["tc_rpo_small_gated", "tc_po_small_ungated", "t_rpo_shipped_tail"])
def test_head_outputs_and_step_risks_are_the_models(name):
    """hazards / S / Y_hat at alpha = 1 against model(**features) at test_gpu_mm_ig's tolerance for the same comparison, and
    step_risk[k] against the model's forward on alpha_k * the inputs."""
    from multimodalfusion_amd import ops
    c, model, feats = _model(name)
    got = _raw(name, float("nan"), False)
    with torch.no_grad():
        hz, S, Y_hat, _ = model(**feats)
        a = ops.ig_quadrature(c.method, c.n_steps)[0].astype(np.float32)
        steps = [float(-model(**{k: v * float(ak) for k, v in feats.items()})[1].sum()) for ak in a]
    torch.cuda.synchronize()
    K = c.K
    np.testing.assert_allclose(got["head"][K:2 * K], _np(hz).reshape(-1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["head"][2 * K:3 * K], _np(S).reshape(-1), rtol=0, atol=1e-5)
    assert abs(got["head"][3 * K] + float(S.sum())) <= 1e-5 and got["Y_hat"] == int(Y_hat.reshape(-1)[0])
    err = np.abs(got["risks"][2:] - np.asarray(steps)).max()
    print(f"{name} step_risk against the model's forward: max err {err:.3e}")
    assert err <= 1e-5


def test_surface_refusals_and_eval_mode_is_restored():
    from multimodalfusion_amd import _lib, infer
    c, model, feats = _model("tc_po_small_ungated")
    model.train()
    with pytest.raises(RuntimeError):
        model.integrated_gradients_tensor(**feats)
    model.eval()
    with pytest.raises(NotImplementedError):
        model.integrated_gradients(**feats)
    with pytest.raises(NotImplementedError):
        model.integrated_gradients_tensor(**{**feats, "path_features": feats["path_features"].to(torch.bfloat16)})
    with pytest.raises(_lib.MmfError):
        model.integrated_gradients_tensor(path_features=feats["path_features"])
    model.train()
    cpu = {k: v.cpu() for k, v in feats.items()}
    out = infer.attribute_modalities(model, cpu, n_steps=4)               # eval for the call, then restored
    assert model.training and out.patch_abs.shape == (33,) and out.gene_attr.shape == (80,) and out.attr is None
    assert out.inst_abs is None and abs(float(out.share["path"]) + float(out.share["omic"]) - 1.0) <= 1e-6
