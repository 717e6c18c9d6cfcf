"""GPU: the grouped forward-only pass (include/mmf_amil.h: mmf_amil_infer_group / mmf_radio_infer_group;
model.forward_group) -- G bags evaluated with fixed weights in one launch chain over their concatenated rows.  Each bag of
a ragged group (sizes across the 64- and 128-row boundaries) against the fp64 / bf16 oracle of that bag alone and against
the per-bag no_grad forward; the refusals of the contract; the grouped validation, summary, export and heat-map loops
against their per-bag forms."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import bf16_port
from oracle import cases
from oracle import inputs as gen
from oracle import torch_port as tp
from test_gpu_path import DEV, _load

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 128, 129, 999, 4097, 10000]


def _path_model(gated=True, size="small", K=4, seed=3):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    sd = gen.path_state_dict(seed=seed, gated=gated, size=size, n_classes=K, dropout=False, bias_std=0.02)
    return _load(MIL_Attention_fc_surv_path(gate_path=gated, model_size_wsi=size, dropout=False, n_classes=K), sd).eval(), sd


def _labels(G, K):
    return torch.tensor([(g + 1) % K for g in range(G)]), torch.tensor([float(g % 2) for g in range(G)])


def _per_bag(model, **feats):
    with torch.no_grad():
        hz, S, Yh, A = model(**feats)
        M = model(**feats, return_features=True)
    return hz, S, Yh, A, M


def _np(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("gated", [True, False])
def test_fp32_group_matches_the_oracle_and_the_per_bag_forward(gated, size, K):
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    model, sd = _path_model(gated, size, K)
    xs = [gen.bag(100 + g, n) for g, n in enumerate(SIZES)]
    bags = [torch.as_tensor(x).to(DEV) for x in xs]
    Y, c = _labels(len(SIZES), K)
    alpha = 0.15
    hz, S, Yh, A, loss, risk = model.forward_group(bags, Y, c, alpha=alpha)
    M = model.forward_group(bags, return_features=True)
    torch.cuda.synchronize()
    assert hz.shape == (len(SIZES), K) and M.shape[0] == len(SIZES) and len(A) == len(SIZES)
    sdt = tp.to_torch(sd, torch.float64, False)
    for g, x in enumerate(xs):
        tag = f"bag {g} (N = {SIZES[g]})"
        rh, rS, rY, rA, rM = tp.path_forward(sdt, torch.as_tensor(x).double(), gated, False, None)
        rl = tp.nll_loss(rh, rS, Y[g:g + 1], c[g:g + 1], alpha=alpha)
        np.testing.assert_allclose(_np(A[g]), rA.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        np.testing.assert_allclose(_np(hz[g:g + 1]), rh.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        np.testing.assert_allclose(_np(S[g:g + 1]), rS.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        assert abs(float(loss[g]) - float(rl)) <= 1e-5, (tag, float(loss[g]), float(rl))
        # the per-bag no_grad forward (mmf_amil_infer + the head), to fp32 rounding
        ph, pS, pY, pA, pM = _per_bag(model, path_features=bags[g])
        pl = NLLSurvLoss(alpha=alpha)(hazards=ph, S=pS, Y=Y[g:g + 1].to(DEV), c=c[g:g + 1].to(DEV))
        np.testing.assert_allclose(_np(A[g]), _np(pA), rtol=0, atol=1e-5, err_msg=tag)
        np.testing.assert_allclose(_np(M[g:g + 1]), _np(pM), rtol=0, atol=1e-5, err_msg=tag)
        np.testing.assert_allclose(_np(hz[g:g + 1]), _np(ph), rtol=0, atol=2e-6, err_msg=tag)
        np.testing.assert_allclose(_np(S[g:g + 1]), _np(pS), rtol=0, atol=2e-6, err_msg=tag)
        assert abs(float(risk[g]) + float(pS.sum())) <= 4e-6 and abs(float(loss[g]) - float(pl)) <= 2e-6, tag
        assert int(Yh[g, 0]) == int(pY[0, 0]) == int(rY[0, 0]), tag


def _bf16_oracle(sd, xq, gated, K):
    M, A_raw, _ = bf16_port.amil_bf16(sd, "attention_net_WSI", xq, gated, False)
    logits = M @ bf16_port._t(sd["classifier.weight"]).T + bf16_port._t(sd["classifier.bias"])
    hz, S, Yh = tp.surv_head(logits)
    return hz, S, A_raw, M


def _check_bf16(got, want, tag):
    """Against the bf16 oracle: test_gpu_bf16.py's bars."""
    for name, a, b, tol in zip(("hazards", "A_raw", "M"), got, want, (2e-3, 5e-3, 5e-3)):
        a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
        np.testing.assert_allclose(a, b, rtol=0, atol=tol, err_msg=f"{tag} {name}")
        if name == "A_raw" and a.size >= 1000:      # outliers are rare bf16 rounding flips of h (one is 1 % of 100 rows)
            assert float(np.quantile(np.abs(a - b), 0.99)) <= 2e-4, tag


def _check_per_bag(got, want, tag):
    """Against the per-bag bf16 forward: the same bf16 kernels, so the fp32 test's bars."""
    for name, a, b, tol in zip(("hazards", "A_raw", "M"), got, want, (2e-6, 1e-5, 1e-5)):
        np.testing.assert_allclose(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1), rtol=0, atol=tol,
                                   err_msg=f"{tag} {name}")


# the heads whose one-bag bf16 route is the unfused kernels (ops.infer_group_takes_bf16): the grouped pass takes their bags
BF16_HEADS = [(False, "small"), (True, "big"), (False, "big")]


@pytest.mark.parametrize("gated,size", BF16_HEADS)
def test_bf16_group_matches_the_bf16_oracle_and_the_per_bag_forward(gated, size):
    model, sd = _path_model(gated, size, K=4, seed=5)
    sizes = SIZES[:-1]
    xq = [bf16_port.rb(bf16_port._t(gen.bag(200 + g, n))).numpy() for g, n in enumerate(sizes)]
    bags = [torch.as_tensor(x).float().to(torch.bfloat16).to(DEV) for x in xq]
    Y, c = _labels(len(sizes), 4)
    hz, S, Yh, A, loss, risk = model.forward_group(bags, Y, c, alpha=0.15)
    M = model.forward_group(bags, return_features=True)
    for g in range(len(sizes)):
        tag = f"{gated}/{size} bag {g} (N = {sizes[g]})"
        rh, rS, rA, rM = _bf16_oracle(sd, xq[g], gated, 4)
        _check_bf16((_np(hz[g]), _np(A[g]), _np(M[g])), (rh.numpy(), rA.numpy(), rM.numpy()), tag + " vs oracle")
        ph, pS, pY, pA, pM = _per_bag(model, path_features=bags[g])
        _check_per_bag((_np(hz[g]), _np(A[g]), _np(M[g])), (_np(ph), _np(pA), _np(pM)), tag + " vs per-bag")
        pl = tp.nll_loss(ph.double().cpu(), pS.double().cpu(), Y[g:g + 1], c[g:g + 1], alpha=0.15)
        assert abs(float(loss[g]) - float(pl)) <= 2e-6 and abs(float(risk[g]) + float(pS.sum())) <= 4e-6, tag


def test_bf16_window_with_a_41k_row_bag():
    """A 41,000-row bf16 bag beside small ones: most of the window's pooling partials belong to one bag."""
    model, sd = _path_model(False, "small", K=4, seed=6)
    sizes = [129, 41000, 64]
    xq = [bf16_port.rb(bf16_port._t(gen.bag(300 + g, n))).numpy() for g, n in enumerate(sizes)]
    bags = [torch.as_tensor(x).float().to(torch.bfloat16).to(DEV) for x in xq]
    hz, S, Yh, A, loss, risk = model.forward_group(bags)
    M = model.forward_group(bags, return_features=True)
    for g in range(len(sizes)):
        rh, rS, rA, rM = _bf16_oracle(sd, xq[g], False, 4)
        _check_bf16((_np(hz[g]), _np(A[g]), _np(M[g])), (rh.numpy(), rA.numpy(), rM.numpy()), f"bag {g}")
        ph, pS, pY, pA, pM = _per_bag(model, path_features=bags[g])
        _check_per_bag((_np(hz[g]), _np(A[g]), _np(M[g])), (_np(ph), _np(pA), _np(pM)), f"bag {g} vs per-bag")


def test_bf16_windows_of_the_fused_head_are_refused():
    """The gated `small` head takes the fused bf16 forms one bag at a time: its bf16 windows return MMF_ERR_SHAPE."""
    from multimodalfusion_amd import _lib, ops
    model, _ = _path_model(True, "small")
    assert not ops.infer_group_takes_bf16(True, 256, 256) and ops.infer_group_takes_bf16(False, 256, 256)
    bags = [torch.zeros((64, 1024), dtype=torch.bfloat16, device=DEV)] * 2
    with pytest.raises(_lib.MmfError, match="code -2"):
        model.forward_group(bags)


def _radio_model(n_mod=4):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    sd = gen.radio_state_dict(seed=2, gated=True, n_classes=4, dropout=True, n_mod=n_mod, bias_std=0.02)
    return _load(MIL_Attention_fc_surv_radio(n_classes=4, modalities=list(cases.MODS[:n_mod])), sd).eval(), sd


def test_radio_group_four_modalities_matches_the_oracle():
    model, sd = _radio_model()
    sizes = [1, 63, 64, 65, 128, 129, 512, 999]
    bags = [{m: torch.as_tensor(gen.bag(400 + 10 * g + i, n)).to(DEV) for i, m in enumerate(cases.MODS)}
            for g, n in enumerate(sizes)]
    Y, c = _labels(len(sizes), 4)
    hz, S, Yh, A, loss, risk = model.forward_group(bags, Y, c, alpha=0.0)
    M = model.forward_group(bags, return_features=True)
    sdt = tp.to_torch(sd, torch.float64, False)
    for g, b in enumerate(bags):
        tag = f"bag {g} (N = {sizes[g]})"
        rh, rS, rY, rA, rM = tp.radio_forward(sdt, [b[m].double().cpu() for m in cases.MODS], True, True, None)
        rl = tp.nll_loss(rh, rS, Y[g:g + 1], c[g:g + 1], alpha=0.0)
        np.testing.assert_allclose(_np(A[g]), rA.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        np.testing.assert_allclose(_np(hz[g:g + 1]), rh.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        np.testing.assert_allclose(_np(S[g:g + 1]), rS.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        np.testing.assert_allclose(_np(M[g:g + 1]), rM.numpy(), rtol=0, atol=1e-4, err_msg=tag)
        assert abs(float(loss[g]) - float(rl)) <= 1e-5, tag
        ph, pS, pY, pA, pM = _per_bag(model, **b)
        np.testing.assert_allclose(_np(hz[g:g + 1]), _np(ph), rtol=0, atol=2e-6, err_msg=tag)
        np.testing.assert_allclose(_np(M[g:g + 1]), _np(pM), rtol=0, atol=1e-5, err_msg=tag)


def test_refusals_return_the_documented_codes():
    from multimodalfusion_amd import _lib, ops
    from multimodalfusion_amd.models.model_modules import stack_args
    model, _ = _path_model()
    model.train()
    with pytest.raises(RuntimeError):
        model.forward_group([torch.zeros((10, 1024), device=DEV)])
    model.eval()
    gated, stack, _, _ = stack_args(model.attention_net_WSI, False)
    stack = tuple(t.contiguous() for t in stack)
    x = torch.zeros((130, 1024), device=DEV)
    A = torch.empty((130,), device=DEV)
    M = torch.empty((65, 256), device=DEV)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=DEV)
    l = _lib.lib()

    def call(offsets, p_h=0.0, p_att=0.0):
        G = len(offsets) - 1
        offs = (C.c_int64 * len(offsets))(*offsets)
        grp = _lib.BagGroup(G=G, offsets=offs, seeds=None)
        d = ops._amil_desc(stack, offsets[-1], 1024, 256, 256, gated, p_h, p_att, 0, None)
        return l.mmf_amil_infer_group(C.byref(d), C.byref(grp), _lib.ptr(x), 0, _lib.ptr(ws), ws.numel(), None, None,
                                      _lib.ptr(M), _lib.ptr(A), _lib.stream_ptr())

    assert call([0, 64, 130]) == 0
    torch.cuda.synchronize()
    ARG, SHAPE = -1, -2
    assert l.mmf_strerror(ARG).startswith(b"invalid argument") and l.mmf_strerror(SHAPE).startswith(b"unsupported shape")
    assert call([0, 64, 130], p_h=0.25) == ARG                  # train mode
    assert call([0, 64, 130], p_att=0.25) == ARG
    assert call(list(range(66))) == SHAPE                       # G = 65
    assert call([0, 64, 64, 130]) == SHAPE                      # an empty bag
    with pytest.raises(_lib.MmfError):
        ops.amil_infer_group(x, [1] * 65 + [65], stack, gated, want_M=True)


def _loader(n_bags, K, seed=0, skip_at=(5,)):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n_bags):
        n = int(rs.randint(40, 700))
        path = torch.zeros((1, 1)) if i in skip_at else torch.as_tensor(gen.bag(500 + i, n))
        out.append(({}, path, torch.zeros((1, 4)), torch.tensor([int(rs.randint(0, K))]),
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


def test_grouped_validation_and_summary_match_the_per_bag_loops(monkeypatch):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    from multimodalfusion_amd.utils.utils import l1_reg_all
    model, _ = _path_model(K=4, seed=9)
    loader = _loader(ops.GROUP_MAX + 9, 4)
    calls = {"group": 0}
    g0 = ops.amil_infer_group

    def counted(*a, **k):
        calls["group"] += 1
        return g0(*a, **k)

    runs = []
    for group in (False, True):
        es, wr = _Recorder(), _Recorder()
        if group:
            monkeypatch.setattr(ops, "amil_infer_group", counted)
        core_utils.validate_survival(0, 3, model, loader, 4, "path", early_stopping=es, writer=wr,
                                     loss_fn=NLLSurvLoss(alpha=0.15), reg_fn=l1_reg_all, lambda_reg=1e-5, group=group)
        res, cidx = core_utils.summary_survival(model, loader, 4, "path", loss_fn=NLLSurvLoss(alpha=0.15), group=group)
        runs.append((es, wr, res, cidx))
    assert calls["group"] >= 4                       # > GROUP_MAX bags: two grouped calls per pass, two passes
    (es0, wr0, res0, c0), (es1, wr1, res1, c1) = runs
    assert abs(wr0.scalars["val/loss_surv"] - wr1.scalars["val/loss_surv"]) <= 1e-6
    assert abs(wr0.scalars["val/loss"] - wr1.scalars["val/loss"]) <= 1e-6
    assert wr0.scalars["val/c-index"] == wr1.scalars["val/c-index"]
    assert len(es0.calls) == len(es1.calls) == 1 and es0.calls[0][0] == es1.calls[0][0]
    assert abs(es0.calls[0][1] - es1.calls[0][1]) <= 1e-6
    assert list(res0["subject_id"]) == list(res1["subject_id"]) and len(res0["subject_id"]) == len(loader) - 1
    np.testing.assert_allclose(res1["risk"], res0["risk"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(res1["disc_label"], res0["disc_label"])
    assert c0 == c1


@pytest.mark.parametrize("gated,grouped", [(False, True), (True, False)])
def test_grouped_loops_on_bf16_bags(monkeypatch, gated, grouped):
    """bf16 bags: the ungated head's go through the grouped pass, the gated `small` head's (fused one-bag forms) keep the
    per-bag route -- either way the two loops agree."""
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    model, _ = _path_model(gated=gated, K=4, seed=11)
    loader = [(r, p.to(torch.bfloat16), *rest) for r, p, *rest in _loader(ops.GROUP_MAX + 3, 4, seed=2)]
    calls = {"group": 0}
    g0 = ops.amil_infer_group

    def counted(*a, **k):
        calls["group"] += 1
        return g0(*a, **k)

    runs = []
    for group in (False, True):
        es, wr = _Recorder(), _Recorder()
        if group:
            monkeypatch.setattr(ops, "amil_infer_group", counted)
        core_utils.validate_survival(0, 0, model, loader, 4, "path", early_stopping=es, writer=wr,
                                     loss_fn=NLLSurvLoss(alpha=0.15), group=group)
        runs.append((wr, *core_utils.summary_survival(model, loader, 4, "path", loss_fn=NLLSurvLoss(), group=group)))
    assert (calls["group"] > 0) == grouped, calls
    (wr0, res0, c0), (wr1, res1, c1) = runs
    assert abs(wr0.scalars["val/loss_surv"] - wr1.scalars["val/loss_surv"]) <= 1e-6
    assert wr0.scalars["val/c-index"] == wr1.scalars["val/c-index"] and c0 == c1
    assert list(res0["subject_id"]) == list(res1["subject_id"])
    np.testing.assert_allclose(res1["risk"], res0["risk"], rtol=0, atol=1e-6)


def test_grouped_validation_losses_per_bag(monkeypatch):
    """Each bag's loss value lands in its loader slot: the stacked losses of the two passes agree bag by bag."""
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    model, _ = _path_model(K=4, seed=10)
    loader = _loader(20, 4, seed=1, skip_at=(0, 7))
    got = []
    stack0 = torch.stack

    def spy(ts, *a, **k):
        out = stack0(ts, *a, **k)
        got.append(out.detach().float().cpu().numpy().copy())
        return out

    for group in (False, True):
        monkeypatch.setattr(torch, "stack", spy)
        core_utils.validate_survival(0, 0, model, loader, 4, "path", loss_fn=NLLSurvLoss(), group=group)
        monkeypatch.setattr(torch, "stack", stack0)
    losses0, losses1 = got[0], got[2]                # (losses, regs) per pass
    assert losses0.shape == losses1.shape == (18,)
    np.testing.assert_allclose(losses1, losses0, rtol=0, atol=1e-6)


def test_grouped_export_gives_the_per_subject_features():
    from multimodalfusion_amd.infer import extract_features_for_subjects
    path, _ = _path_model(seed=12)
    radio, _ = _radio_model()
    subjects = []
    for i in range(70):
        n = 30 + 17 * i
        p = torch.zeros((1, 1)) if i == 3 else torch.as_tensor(gen.bag(600 + i, n))
        r = {m: torch.as_tensor(gen.bag(700 + 4 * i + j, 20 + i)) for j, m in enumerate(cases.MODS)}
        subjects.append((f"s{i}", r, p, None))
    models = {"path": path, "radio": radio}
    want = list(extract_features_for_subjects(models, subjects))
    got = list(extract_features_for_subjects(models, subjects, group=True))
    assert [(s, m) for s, m, _ in got] == [(s, m) for s, m, _ in want]
    for (s, m, a), (_, _, b) in zip(got, want):
        assert a.shape == b.shape and a.device.type == "cpu"
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=1e-5, err_msg=f"{s}/{m}")


@pytest.mark.parametrize("size,dtype", [("small", torch.float32), ("big", torch.float32), ("small", torch.bfloat16)])
def test_grouped_patch_scoring_is_bit_identical_to_per_batch_scoring(size, dtype):
    """fp32 batches are grouped up to the row cap of the head (2,048 rows `small`, 1,024 `big`); bf16 batches keep one call
    each.  Either way the scores are the per-batch scores bit for bit."""
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.infer import score_patch_batches
    model, _ = _path_model(size=size, seed=8)
    x = torch.as_tensor(gen.bag(41, 512 * 9 + 77)).to(dtype)
    batches = [x[i:i + 512] for i in range(0, x.shape[0], 512)]
    want = list(score_patch_batches(model, batches))
    calls = {"group": 0}
    g0 = ops.amil_infer_group

    def counted(*a, **k):
        calls["group"] += 1
        return g0(*a, **k)

    ops_group = ops.amil_infer_group
    ops.amil_infer_group = counted
    try:
        got = list(score_patch_batches(model, batches, group=True))
    finally:
        ops.amil_infer_group = ops_group
    assert calls["group"] == ({"small": 3, "big": 5}[size] if dtype == torch.float32 else 0), calls
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)
    ref = np.random.RandomState(0).normal(size=300).astype(np.float32)
    for a, b in zip(score_patch_batches(model, batches, ref_scores=ref, group=True),
                    score_patch_batches(model, batches, ref_scores=ref)):
        assert np.array_equal(a, b)
