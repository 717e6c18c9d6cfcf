"""GPU parity of the multimodal head's grouped forward-only pass, both fusions (MM_MIL_Attention_fc_surv.forward_group over
include/mmf_amil.h: mmf_amil_infer_group / mmf_radio_infer_group without a head, mmf_dense_forward on a B = G batch,
mmf_xfusion_infer_group, mmf_surv_head_infer_group).  Per patient, hazards / S / Y_hat / both score vectors / loss / risk
/ the fused embedding against the fp64 oracle of that patient alone; the grouped pass against the per-patient route it
replaces; position independence of the new kernels to the bit; the new kernels alone against fp64 numpy; the refusals;
and validate_survival / summary_survival with and without group=True.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import inputs as gen
from oracle import torch_port as tp
from test_gpu_path import DEV, _load, _t, compare
from test_gpu_poison import poison  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

FUSIONS = ("concat", "tensor")
SIXTY_FOUR_P = [1 + (53 * g) % 400 for g in range(64)]
SIXTY_FOUR_R = [1 + (37 * g) % 90 for g in range(64)]
OBSERVED = {}                                  # tag -> largest error seen, printed by each test (pytest -s)


def _note(tag, err):
    OBSERVED[tag] = max(OBSERVED.get(tag, 0.0), float(err))


def _base(mode, gate_path, gate_radio, K, fusion, **kw):
    base = dict(mode=mode, gate_path=gate_path, gate_radio=gate_radio, K=K, fusion=fusion, G=80, alpha=0.3, bias_std=0.05,
                seed=4343, x_seed=510, train=False, dropout=False)
    base.update(kw)
    return base


def _metas(base, path_sizes, radio_sizes):
    return [dict(base, Np=Np, nr=nr, x_seed=base["x_seed"] + 101 * g, y=(g + 1) % base["K"], c=g % 2)
            for g, (Np, nr) in enumerate(zip(path_sizes, radio_sizes))]


def _model(m):
    from multimodalfusion_amd.models import MM_MIL_Attention_fc_surv
    sd = cases.mm_inputs(m)[0]
    return _load(MM_MIL_Attention_fc_surv(input_dim=m["G"], radio_fusion="concat", fusion=m["fusion"], gate=True,
                                          gate_path=m["gate_path"], gate_omic=True, gate_radio=m["gate_radio"],
                                          dropout=False, n_classes=m["K"], mode=m["mode"]), sd).eval()


def _patient(m):
    _, xs, xp, xo = cases.mm_inputs(m)
    kw = {k: _t(x) for k, x in zip(cases.MODS, xs)}
    kw["path_features"] = _t(xp)
    kw["genomic_features"] = _t(xo)
    return kw


def _stacked(patients):
    path = (torch.cat([p["path_features"] for p in patients]), [int(p["path_features"].shape[0]) for p in patients])
    radio = (torch.stack([torch.cat([p[m] for p in patients]) for m in cases.MODS]),
             [int(p["T1"].shape[0]) for p in patients])
    omic = torch.stack([p["genomic_features"] for p in patients])
    return path, radio, omic


def _labels(metas):
    return torch.tensor([m["y"] for m in metas]), torch.tensor([float(m["c"]) for m in metas])


@functools.lru_cache(maxsize=None)
def _oracle(key):
    """The fp64 oracle of one patient alone, once per patient of the module: cases.run_mm, and the fused embedding MM the
    same torch port returns (run_mm drops it)."""
    m = dict(key)
    ref = cases.run_mm(m)
    sd_np, xs, xp, xo = cases.mm_inputs(m)
    sd = tp.to_torch(sd_np, torch.float64)
    T = lambda a: torch.as_tensor(a).to(torch.float64)
    with torch.no_grad():
        MM = tp.mm_forward(sd, [T(x) for x in xs], T(xp), T(xo), fusion=m["fusion"], gate_path=m["gate_path"],
                           gate_radio=m["gate_radio"], dropout=False, mode=m["mode"])[4]
    return dict(ref, MM=MM.detach().numpy(), grads={})


def oracle_patient(m):
    return _oracle(tuple(sorted(m.items())))


def run_group(metas, model=None, patients=None):
    model = _model(metas[0]) if model is None else model
    patients = [_patient(m) for m in metas] if patients is None else patients
    Y, c = _labels(metas)
    hz, S, Yh, A, loss, risk = model.forward_group(patients, Y, c, alpha=metas[0]["alpha"])
    feats = model.forward_group(patients, return_features=True)
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(),
                A={k: [a.cpu().numpy() for a in v] for k, v in A.items()}, loss=loss.cpu().numpy(),
                risk=risk.cpu().numpy(), feats=feats.cpu().numpy())


def check_group(res, metas):
    keys = {"radiology": "radio", "pathology": "path"}
    for g, m in enumerate(metas):
        ref = oracle_patient(m)
        assert set(res["A"]) == set(ref["A_raw"]) == {k for k, b in keys.items() if b in m["mode"]}
        one = dict(hazards=res["hazards"][g:g + 1], S=res["S"][g:g + 1], loss=float(res["loss"][g]), grads={},
                   A_raw={k: res["A"][k][g] for k in ref["A_raw"]})
        _note("oracle hazards", np.abs(one["hazards"] - ref["hazards"]).max())
        _note("oracle S", np.abs(one["S"] - ref["S"]).max())
        _note("oracle loss", abs(one["loss"] - float(ref["loss"])))
        for k in ref["A_raw"]:
            _note("oracle A_raw", np.abs(one["A_raw"][k] - ref["A_raw"][k]).max())
        _note("oracle feats", np.abs(res["feats"][g:g + 1] - ref["MM"]).max())
        compare(one, ref, f"patient {g}")                                       # A_raw, hazards, S 1e-4; loss 1e-5
        assert int(res["Y_hat"][g]) == int(np.asarray(ref["Y_hat"]).reshape(-1)[0]), f"patient {g}"
        assert abs(float(res["risk"][g]) + float(res["S"][g].sum())) < 1e-5, f"patient {g}"
        np.testing.assert_allclose(res["feats"][g:g + 1], ref["MM"], rtol=0, atol=1e-4, err_msg=f"patient {g}")
    print("observed maxima:", {k: f"{v:.2e}" for k, v in sorted(OBSERVED.items())})


# mode, gate_path, gate_radio, K, pathology sizes, radio sizes, pre-stacked triple
CASES = [
    ("radio_path_omic", True, True, 4, [1, 5, 64, 130], [1, 17, 3, 40], False),
    ("radio_path_omic", False, False, 1, SIXTY_FOUR_P, SIXTY_FOUR_R, True),
    ("radio_path", True, False, 32, [300, 50], [20, 64], True),
    ("path_omic", False, True, 1, [5], [1], False),
    ("radio_omic", True, True, 4, [1] * 9, SIXTY_FOUR_R[:9], False),
    ("path_omic", True, True, 32, SIXTY_FOUR_P[:9], [1] * 9, True),
]


@pytest.mark.parametrize("fusion", FUSIONS)
@pytest.mark.parametrize("mode,gate_path,gate_radio,K,psizes,rsizes,stacked", CASES)
def test_group_matches_oracle_per_patient(mode, gate_path, gate_radio, K, psizes, rsizes, stacked, fusion):
    metas = _metas(_base(mode, gate_path, gate_radio, K, fusion), psizes, rsizes)
    patients = [_patient(m) for m in metas]
    check_group(run_group(metas, patients=_stacked(patients) if stacked else patients), metas)


@pytest.mark.parametrize("fusion", FUSIONS)
def test_pre_stacked_window_equals_the_list_form_and_a_repeat_is_bit_identical(fusion):
    metas = _metas(_base("radio_path_omic", True, True, 4, fusion, seed=91, x_seed=92), [65, 130, 7], [12, 300, 1])
    model = _model(metas[0])
    patients = [_patient(m) for m in metas]
    a = run_group(metas, model=model, patients=patients)
    for other in (run_group(metas, model=model, patients=patients), run_group(metas, model=model, patients=_stacked(patients))):
        for k in ("hazards", "S", "loss", "risk", "Y_hat", "feats"):
            assert np.array_equal(other[k], a[k]), k
        for k in a["A"]:
            assert all(np.array_equal(x, y) for x, y in zip(other["A"][k], a["A"][k])), k


@pytest.mark.parametrize("fusion", FUSIONS)
@pytest.mark.parametrize("mode,gate_path,gate_radio,K,psizes,rsizes,stacked", [CASES[0], CASES[1], CASES[2], CASES[5]])
def test_group_against_the_per_patient_route(mode, gate_path, gate_radio, K, psizes, rsizes, stacked, fusion):
    """The same patients through model(**kw) under no_grad + NLLSurvLoss: both routes are inside the bars of the same
    oracle, so they agree within twice those bars."""
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    metas = _metas(_base(mode, gate_path, gate_radio, K, fusion, alpha=0.1, seed=78, x_seed=610), psizes, rsizes)
    model = _model(metas[0])
    patients = [_patient(m) for m in metas]
    res = run_group(metas, model=model, patients=patients)
    loss_fn = NLLSurvLoss(alpha=metas[0]["alpha"])
    with torch.no_grad():
        for g, (m, kw) in enumerate(zip(metas, patients)):
            hz, S, Yh, A = model(**kw)
            loss = loss_fn(hazards=hz, S=S, Y=torch.tensor([m["y"]], device=DEV), c=torch.tensor([float(m["c"])], device=DEV))
            feats = model(**kw, return_features=True)
            errs = dict(hazards=np.abs(res["hazards"][g:g + 1] - hz.cpu().numpy()).max(),
                        S=np.abs(res["S"][g:g + 1] - S.cpu().numpy()).max(),
                        loss=abs(float(res["loss"][g]) - float(loss)),
                        feats=np.abs(res["feats"][g:g + 1] - feats.cpu().numpy()).max())
            for k, v in A.items():
                errs["A_raw"] = max(errs.get("A_raw", 0.0), np.abs(res["A"][k][g] - v.cpu().numpy()).max())
            for k, v in errs.items():
                _note("route " + k, v)
                assert v <= (2e-5 if k == "loss" else 2e-4), (g, k, v)
            assert abs(float(res["risk"][g]) + float(S.sum())) <= 2e-5, g
            assert int(res["Y_hat"][g]) == int(Yh), g
    print("observed maxima:", {k: f"{v:.2e}" for k, v in sorted(OBSERVED.items())})


# ---- position independence of the new kernels, on the raw entry points ---------------------------------------------------
def _xfusion_operands(m, G, seed=7, mmhid=512, nhid=256, dim=256):
    rs = lambda i, shape, std: gen.normal(seed + i, shape, stream=i, std=std)
    vs = [rs(i, (G, dim), 1.0) for i in range(m)]
    w = []
    for i in range(m):
        w += [rs(10 + i, (16, dim), 1 / 16.0), rs(20 + i, (16,), 0.1), rs(30 + i, (16, m * dim), 1 / np.sqrt(m * dim)),
              rs(40 + i, (16,), 0.1), rs(50 + i, (16, 16), 0.25), rs(60 + i, (16,), 0.1)]
    K1 = 17 ** m
    w += [rs(70, (mmhid, K1), 1 / np.sqrt(K1)), rs(71, (mmhid,), 0.1), rs(72, (mmhid, mmhid + m * dim), 1 / np.sqrt(mmhid + m * dim)),
          rs(73, (mmhid,), 0.1)]
    return vs, w, rs(74, (nhid, mmhid), 1 / np.sqrt(mmhid)), rs(75, (nhid,), 0.1)


def _xfusion_fp64(vs, w, Wc0, bc0):
    """XlinearFusion (gate, skip) + classifier[0] in numpy fp64 -> (o [m x G x 16], e1, MM, hid)."""
    m = len(vs)
    vs = [np.asarray(v, np.float64) for v in vs]
    w = [np.asarray(a, np.float64) for a in w]
    cat = np.concatenate(vs, 1)
    os_ = []
    for i in range(m):
        Wh, bh, Wz, bz, Wo, bo = w[6 * i:6 * i + 6]
        h = np.maximum(vs[i] @ Wh.T + bh, 0)
        z = cat @ Wz.T + bz
        os_.append(np.maximum((h / (1 + np.exp(-z))) @ Wo.T + bo, 0))
    G = vs[0].shape[0]
    ones = np.ones((G, 1))
    kr = np.concatenate([os_[0], ones], 1)
    for o in os_[1:]:
        kr = (kr[:, :, None] * np.concatenate([o, ones], 1)[:, None, :]).reshape(G, -1)
    We1, be1, We2, be2 = w[6 * m:]
    e1 = np.maximum(kr @ We1.T + be1, 0)
    MM = np.maximum(np.concatenate([e1] + vs, 1) @ We2.T + be2, 0)
    hid = np.maximum(MM @ np.asarray(Wc0, np.float64).T + np.asarray(bc0, np.float64), 0)
    return np.stack(os_), e1, MM, hid


@pytest.mark.parametrize("m", [2, 3])
def test_xfusion_rows_do_not_depend_on_the_window(m, poison):  # noqa: F811
    """ops.xfusion_infer_group on 64 patients against the same call on one of them alone: bit equality, on poisoned
    outputs and workspace."""
    from multimodalfusion_amd import ops
    vs, w, Wc0, bc0 = _xfusion_operands(m, 64)
    tv, tw = [_t(v) for v in vs], [_t(a) for a in w]
    MM, hid = poison.run("nan", ops.xfusion_infer_group, tv, tw, _t(Wc0), _t(bc0))
    assert bool(torch.isfinite(MM).all()) and bool(torch.isfinite(hid).all())
    for g in (0, 7, 8, 63):
        MM1, hid1 = poison.run("nan", ops.xfusion_infer_group, [v[g:g + 1] for v in tv], tw, _t(Wc0), _t(bc0))
        assert torch.equal(MM1, MM[g:g + 1]) and torch.equal(hid1, hid[g:g + 1]), g
    MM9, hid9 = ops.xfusion_infer_group([v[3:12] for v in tv], tw, _t(Wc0), _t(bc0))      # another window size and offset
    assert torch.equal(MM9, MM[3:12]) and torch.equal(hid9, hid[3:12])


@pytest.mark.parametrize("widths,K,G", [((256, 256, 256), 4, 64), ((256, 256), 32, 9), ((100, 7, 1), 1, 3), ((1024,), 17, 1)])
def test_head_infer_group_equals_the_training_heads_forward(widths, K, G, poison):  # noqa: F811
    """ops.surv_head_infer_group on separate segments against ops.surv_head_nll_step_group's forward outputs on the
    concatenated [G x F] matrix: the same head_tail body, so bit equality."""
    from multimodalfusion_amd import ops
    F = sum(widths)
    segs = [_t(gen.normal(10 + i, (G, wd), stream=wd)) for i, wd in enumerate(widths)]
    Wk, bk = _t(gen.normal(11, (K, F), stream=K, std=1.0 / np.sqrt(F))), _t(gen.normal(12, (K,), stream=3, std=0.1))
    Y, c = torch.tensor([(3 * g + 1) % K for g in range(G)]), torch.tensor([float(g % 2) for g in range(G)])
    hz, S, Yh, loss, risk = poison.run("nan", ops.surv_head_infer_group, segs, Wk, bk, Y, c, 0.3)
    dWk, dbk = torch.empty_like(Wk), torch.empty_like(bk)
    rhz, rS, rYh, rloss, rrisk, _ = ops.surv_head_nll_step_group(torch.cat(segs, 1), Wk, bk, Y, c, 0.3, dWk, dbk)
    torch.cuda.synchronize()
    for got, ref, name in ((hz, rhz, "hazards"), (S, rS, "S"), (Yh, rYh, "Y_hat"), (loss, rloss, "loss"), (risk, rrisk, "risk")):
        assert torch.equal(got, ref), name
    hz2, S2, Yh2, loss2, risk2 = ops.surv_head_infer_group(segs, Wk, bk)                  # no labels: no loss
    assert loss2 is None and torch.equal(hz2, hz) and torch.equal(S2, S) and torch.equal(risk2, risk)


# ---- the new kernels alone against fp64 numpy -------------------------------------------------------------------------
@pytest.mark.parametrize("m,G", [(2, 1), (2, 64), (3, 1), (3, 9), (3, 64)])
def test_xfusion_kernels_against_fp64(m, G):
    """The gating stage, the fused Kronecker . encoder1 contraction, encoder2's skip read and classifier[0], at the bars of
    test_gpu_omic_mm.py's one-patient kernels (atol 2e-5, rtol 1e-5).  A second weight set keeps only the last 49 columns of
    encoder1's weight: the row tail (the partly filled last chunk of a 17^m-wide row) alone then carries the result."""
    from multimodalfusion_amd import ops
    for tail_only in (False, True):
        vs, w, Wc0, bc0 = _xfusion_operands(m, G, seed=31 + m)
        if tail_only:
            We1 = np.array(w[6 * m], copy=True)
            We1[:, :-49] = 0
            We1[:, -49:] *= 8                      # keep encoder1's pre-activations of order one
            w[6 * m] = We1
        MM, hid = ops.xfusion_infer_group([_t(v) for v in vs], [_t(a) for a in w], _t(Wc0), _t(bc0))
        torch.cuda.synchronize()
        _, e1, rMM, rhid = _xfusion_fp64(vs, w, Wc0, bc0)
        assert (e1 > 0).mean() > 0.1               # the contraction is not hidden behind the ReLU
        np.testing.assert_allclose(MM.cpu().numpy(), rMM, atol=2e-5, rtol=1e-5)
        np.testing.assert_allclose(hid.cpu().numpy(), rhid, atol=2e-5, rtol=1e-5)


def test_encoder2_reads_every_part_of_the_skip_connection():
    """Each v_i reaches MM through encoder2's skip columns alone when encoder1 and the gating stage are silenced."""
    from multimodalfusion_amd import ops
    m, G = 3, 5
    vs, w, Wc0, bc0 = _xfusion_operands(m, G, seed=44)
    w[6 * m] = np.zeros_like(w[6 * m])             # encoder1's weight: e1 = relu(be1)
    MM, _ = ops.xfusion_infer_group([_t(v) for v in vs], [_t(a) for a in w], _t(Wc0), _t(bc0))
    base = _xfusion_fp64(vs, w, Wc0, bc0)[2]
    np.testing.assert_allclose(MM.cpu().numpy(), base, atol=2e-5, rtol=1e-5)
    for i in range(m):                             # moving v_i alone moves MM as the fp64 skip read says
        vs2 = [np.array(v, copy=True) for v in vs]
        vs2[i][:, 200:] += 1.0
        w2 = list(w)
        for j in range(m):                         # the gates see v_cat: silence them so that only the skip read moves
            w2[6 * j + 2] = np.zeros_like(w[6 * j + 2])
            w2[6 * j] = np.zeros_like(w[6 * j])
        MM2, _ = ops.xfusion_infer_group([_t(v) for v in vs2], [_t(a) for a in w2], _t(Wc0), _t(bc0))
        ref2 = _xfusion_fp64(vs2, w2, Wc0, bc0)[2]
        np.testing.assert_allclose(MM2.cpu().numpy(), ref2, atol=2e-5, rtol=1e-5)
        assert np.abs(ref2 - _xfusion_fp64(vs, w2, Wc0, bc0)[2]).max() > 1e-2, i


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", FUSIONS)
def test_rejects_bad_calls_before_any_launch(fusion, monkeypatch):
    from multimodalfusion_amd import _lib, ops
    metas = _metas(_base("radio_path_omic", True, True, 4, fusion, seed=91, x_seed=92), [64, 64], [8, 8])
    model = _model(metas[0])
    patients = [_patient(m) for m in metas]
    Y, c = _labels(metas)
    launches = []
    real = ops.stream_ptr
    monkeypatch.setattr(ops, "stream_ptr", lambda: launches.append(1) or real())     # every C-ABI launch asks for the stream

    def refused(exc, pts, Y=Y, c=c, model=model):
        n = len(launches)
        with pytest.raises(exc):
            model.forward_group(pts, Y, c)
        assert len(launches) == n, "a refused call launched something"

    bf = [dict(p, path_features=p["path_features"].to(torch.bfloat16)) for p in patients]
    refused((TypeError, _lib.MmfError), bf)                                  # bf16 bags
    refused(_lib.MmfError, [patients[0]] * 65, Y=[0] * 65, c=[0.0] * 65)     # G = 65
    empty = [patients[0], dict(patients[1], path_features=patients[1]["path_features"][:0])]
    refused(_lib.MmfError, empty)                                            # an empty bag
    path, radio, omic = _stacked(patients)
    refused(_lib.MmfError, (path, radio, omic[:1]))                          # patient counts differ between branches
    refused(_lib.MmfError, ((path[0], [128]), radio, omic))
    refused(_lib.MmfError, patients, model=_model(dict(metas[0], K=33)))     # K = 33
    prev = ops.set_gemm(1)
    try:
        refused(_lib.MmfError, patients)                                     # bf16x3 GEMMs
    finally:
        ops.set_gemm(prev)
    model.train()
    refused(RuntimeError, patients)                                          # training mode
    model.eval()
    hz, *_ = model.forward_group(patients, Y, c)                             # still fine afterwards
    torch.cuda.synchronize()
    assert launches and bool(torch.isfinite(hz).all())


# ---- the evaluation loops ---------------------------------------------------------------------------------------------
N_LOADER, ALONE_AT = 70, 20


def _loader(K):
    rs = np.random.RandomState(3)
    out = []
    for i in range(N_LOADER):
        n, r = int(rs.randint(1, 90)), int(rs.randint(1, 30))
        path = torch.as_tensor(gen.bag(700 + i, n, stream=100))
        radio = {k: torch.as_tensor(gen.bag(700 + i, r, stream=7 * j)) for j, k in enumerate(cases.MODS)}
        if i == ALONE_AT:
            path = path.to(torch.bfloat16)             # the grouped pass does not take it: a flush in mid pass
        out.append((radio, path, torch.as_tensor(gen.normal(700 + i, (1, 80), stream=200)), torch.tensor([int(rs.randint(0, K))]),
                    np.array([float(rs.uniform(1, 50))]), torch.tensor([float(rs.randint(0, 2))])))
    return out


class _Recorder:
    def __init__(self):
        self.calls, self.scalars = [], {}
        self.early_stop = False

    def __call__(self, epoch, val_loss, model):
        self.calls.append((epoch, val_loss))

    def add_scalar(self, k, v, step):
        self.scalars[k] = v


@pytest.mark.parametrize("fusion", FUSIONS)
def test_grouped_validation_and_summary_match_the_per_patient_loops(fusion, monkeypatch):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    from multimodalfusion_amd.utils.utils import l1_reg_all
    model = _model(_base("radio_path_omic", True, True, 4, fusion, seed=9, Np=1, nr=1))
    loader = _loader(4)
    sizes, h0 = [], ops.surv_head_infer_group

    def counted(segs, *a, **k):
        sizes.append(int(segs[0].shape[0]))
        return h0(segs, *a, **k)

    stack0, stacked = torch.stack, []

    def spy(ts, *a, **k):
        out = stack0(ts, *a, **k)
        stacked.append(out.detach().float().cpu().numpy().copy())
        return out

    regs = []
    reg_fn = lambda m: regs.append(1) or l1_reg_all(m)
    runs = []
    for group in (False, True):
        es, wr = _Recorder(), _Recorder()
        monkeypatch.setattr(ops, "surv_head_infer_group", counted)
        monkeypatch.setattr(torch, "stack", spy)
        core_utils.validate_survival(0, 3, model, loader, 4, "radio_path_omic", early_stopping=es, writer=wr,
                                     loss_fn=NLLSurvLoss(alpha=0.15), reg_fn=reg_fn, lambda_reg=1e-5, group=group)
        monkeypatch.setattr(torch, "stack", stack0)
        res, cidx = core_utils.summary_survival(model, loader, 4, "radio_path_omic", loss_fn=NLLSurvLoss(alpha=0.15),
                                                group=group)
        runs.append((es, wr, res, cidx, stacked[-2], len(regs)))
    # two passes, each: 20 patients, the bf16 one alone, 49 more = a full... 20, then 49 at the end
    assert sizes == [ALONE_AT, N_LOADER - ALONE_AT - 1] * 2
    (es0, wr0, res0, c0, loss0, nreg0), (es1, wr1, res1, c1, loss1, nreg1) = runs
    assert nreg0 == N_LOADER and nreg1 - nreg0 == 2              # once for the held patients, once for the one alone
    assert loss0.shape == loss1.shape == (N_LOADER,)
    np.testing.assert_allclose(loss1, loss0, rtol=0, atol=2e-5)  # per patient, in loader order
    assert abs(wr0.scalars["val/loss_surv"] - wr1.scalars["val/loss_surv"]) <= 2e-5
    assert abs(wr0.scalars["val/loss"] - wr1.scalars["val/loss"]) <= 2e-5
    assert wr0.scalars["val/c-index"] == wr1.scalars["val/c-index"]
    assert len(es0.calls) == len(es1.calls) == 1 and es0.calls[0][0] == es1.calls[0][0]
    assert abs(es0.calls[0][1] - es1.calls[0][1]) <= 2e-5
    assert list(res0["subject_id"]) == list(res1["subject_id"]) == list(range(N_LOADER))
    np.testing.assert_allclose(res1["risk"], res0["risk"], rtol=0, atol=2e-4)
    np.testing.assert_array_equal(res1["disc_label"], res0["disc_label"])
    np.testing.assert_array_equal(res1["censorship"], res0["censorship"])
    assert c0 == c1


def test_a_full_window_flushes_at_group_max(monkeypatch):
    """More than ops.GROUP_MAX eligible patients in a row: the first grouped call takes 64, the end of the pass the rest."""
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.utils import core_utils
    model = _model(_base("radio_path_omic", True, True, 4, "tensor", seed=9, Np=1, nr=1))
    loader = [b for i, b in enumerate(_loader(4)) if i != ALONE_AT]
    sizes, h0 = [], ops.surv_head_infer_group
    monkeypatch.setattr(ops, "surv_head_infer_group", lambda segs, *a, **k: sizes.append(int(segs[0].shape[0])) or h0(segs, *a, **k))
    a, ca = core_utils.summary_survival(model, loader, 4, "radio_path_omic", group=True)
    b, cb = core_utils.summary_survival(model, loader, 4, "radio_path_omic", group=False)
    assert sizes == [ops.GROUP_MAX, N_LOADER - 1 - ops.GROUP_MAX]
    np.testing.assert_allclose(a["risk"], b["risk"], rtol=0, atol=2e-4)
    assert ca == cb and list(a["subject_id"]) == list(b["subject_id"])
