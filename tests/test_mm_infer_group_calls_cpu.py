"""The C-ABI calls behind MM_MIL_Attention_fc_surv.forward_group, without a GPU (the recorder of test_ops_calls_cpu stands
in for the library): for both fusions the order on the one stream -- radio stack, pathology stack, omic SNN, (tensor: the
fusion call,) the hazard head -- with the stacks run headless into their own [G x 256] embeddings, which the head (concat)
or the fusion call (tensor) reads where they lie; no Kronecker / gating / per-patient call; a refused call makes no C-ABI
call at all; and validate_survival / summary_survival(group=True) hold multimodal patients and flush them at
ops.GROUP_MAX patients, at a patient the grouped pass does not take, and at the end of the pass."""
import numpy as np
import pytest
import torch

from multimodalfusion_amd import _lib, ops
from test_ops_calls_cpu import STREAM, rec  # noqa: F401  (fixture)

MODS = ["T1", "T2", "T1Gd", "FLAIR"]
PATH, RADIO = [5, 1, 9], [2, 7, 3]
PER_PATIENT = ("mmf_amil_infer", "mmf_amil_bf16_infer", "mmf_amil_forward", "mmf_amil_head_forward", "mmf_linear_forward",
               "mmf_surv_head_forward", "mmf_kron_forward", "mmf_xreduce_forward", "mmf_gate_mul_forward", "mmf_nll_surv")


def _model(mode="radio_path_omic", fusion="concat", K=4):
    from multimodalfusion_amd.models import MM_MIL_Attention_fc_surv
    torch.manual_seed(0)
    return MM_MIL_Attention_fc_surv(input_dim=80, radio_fusion="concat", fusion=fusion, gate=True, gate_path=True,
                                    gate_omic=True, gate_radio=False, dropout=True, n_classes=K, mode=mode).eval()


def _patients(path=PATH, radio=RADIO):
    return [dict({m: torch.randn(r, 1024) for m in MODS}, path_features=torch.randn(n, 1024),
                 genomic_features=torch.randn(80)) for n, r in zip(path, radio)]


def _calls(rec, name):  # noqa: F811
    log, sizes = rec.log()
    return [a for n, a, _ in log if n == name], sizes


def test_concat_call_order_and_the_head_reads_the_embeddings_in_place(rec):  # noqa: F811
    model = _model()
    out = model.forward_group(_patients(), [0, 1, 2], [0.0, 1.0, 0.0], alpha=0.2)
    assert rec.names == ["mmf_radio_group_infer_workspace_bytes", "mmf_radio_infer_group",
                         "mmf_amil_group_infer_workspace_bytes", "mmf_amil_infer_group",
                         "mmf_dense_forward", "mmf_dense_forward", "mmf_surv_head_infer_group"]
    (rf,), sizes = _calls(rec, "mmf_radio_infer_group")
    (pf,), _ = _calls(rec, "mmf_amil_infer_group")
    (d0, d1), _ = _calls(rec, "mmf_dense_forward")
    (hd,), _ = _calls(rec, "mmf_surv_head_infer_group")
    # the stacks: ragged tables, eval descriptors, no head and no target, M [3 x 256] of their own
    assert rf[1] == {"G": 3, "offsets": [0, 2, 9, 12], "seeds": None}
    assert pf[1] == {"G": 3, "offsets": [0, 5, 6, 15], "seeds": None}
    assert (rf[0]["p_h"], rf[0]["p_att"], rf[0]["gated"], pf[0]["gated"], pf[0]["gemm"]) == (0.0, 0.0, 0, 1, 0)
    assert rf[5] is None and rf[6] is None and pf[6] is None and pf[7] is None
    M_r, M_p = rf[7], pf[8]
    assert sizes[M_r] == sizes[M_p] == 3 * 256 * 4 and M_r != M_p
    # the omic SNN: one B = 3 batch per block, SELU, no dropout, sites 0 and 1
    assert (d0[3], d0[4], d0[5], d0[6], d0[7], d0[8]) == (3, 80, 256, ops.ACT["selu"], 0, 0.0)
    assert (d1[3], d1[4], d1[5], d1[10]) == (3, 256, 256, 1) and d1[0] == d0[12]
    # the head: the three embeddings as segments in the model's order, G = 3, the loss with alpha
    assert hd[0] == [M_r, M_p, d1[12]] and hd[1] == [256, 256, 256] and (hd[2], hd[3]) == (3, 3)
    assert hd[4]["K"] == 4 and abs(hd[5]["alpha"] - 0.2) < 1e-7 and hd[5]["dWk"] is None and hd[6] == STREAM
    hz, S, Y_hat, A_raw, loss, risk = out
    assert hz.shape == (3, 4) and S.shape == (3, 4) and Y_hat.shape == (3,) and loss.shape == (3,) and risk.shape == (3,)
    assert [a.shape[1] for a in A_raw["radiology"]] == RADIO and [a.shape[1] for a in A_raw["pathology"]] == PATH
    assert not any(t.requires_grad for t in (hz, S, loss, risk))


def test_tensor_call_order_and_the_fusion_call_reads_the_embeddings_in_place(rec):  # noqa: F811
    model = _model(fusion="tensor")
    out = model.forward_group(_patients())
    assert rec.names == ["mmf_radio_group_infer_workspace_bytes", "mmf_radio_infer_group",
                         "mmf_amil_group_infer_workspace_bytes", "mmf_amil_infer_group",
                         "mmf_dense_forward", "mmf_dense_forward",
                         "mmf_xfusion_group_infer_workspace_bytes", "mmf_xfusion_infer_group", "mmf_surv_head_infer_group"]
    (rf,), sizes = _calls(rec, "mmf_radio_infer_group")
    (pf,), _ = _calls(rec, "mmf_amil_infer_group")
    (_, d1), _ = _calls(rec, "mmf_dense_forward")
    (q,), _ = _calls(rec, "mmf_xfusion_group_infer_workspace_bytes")
    (xf,), _ = _calls(rec, "mmf_xfusion_infer_group")
    (hd,), _ = _calls(rec, "mmf_surv_head_infer_group")
    assert q == [3, 16, 512, 3]
    w = xf[0]
    assert (w["m"], w["dim"], w["sdim"], w["mmhid1"], w["mmhid2"], w["nhid"]) == (3, 256, 16, 512, 512, 256)
    assert xf[1] == [rf[7], pf[8], d1[12]] and xf[2] == 3 and xf[-1] == STREAM
    ws, nbytes, MM, hid = xf[3], xf[4], xf[5], xf[6]
    assert nbytes == [r for n, _, r in rec.calls if n == "mmf_xfusion_group_infer_workspace_bytes"][0] == sizes[ws]
    assert sizes[MM] == 3 * 512 * 4 and sizes[hid] == 3 * 256 * 4
    # every weight is its own storage of the right size
    assert sizes[w["We1"]] == 512 * 17 ** 3 * 4 and sizes[w["We2"]] == 512 * (512 + 768) * 4 and sizes[w["Wc0"]] == 256 * 512 * 4
    assert [sizes[p] for p in w["Wz"]] == [16 * 768 * 4] * 3 and [sizes[p] for p in w["Wh"]] == [16 * 256 * 4] * 3
    # the head on hid alone, with classifier[3]; no labels: no target
    assert hd[0] == [hid] and hd[1] == [256] and (hd[2], hd[3]) == (1, 3) and hd[4]["K"] == 4 and hd[5] is None
    assert sizes[hd[4]["Wk"]] == 4 * 256 * 4
    assert out[4] is None and out[0].shape == (3, 4)


@pytest.mark.parametrize("fusion", ["concat", "tensor"])
def test_two_branch_mode_runs_its_branches_only(fusion, rec):  # noqa: F811
    model = _model("path_omic", fusion)
    model.forward_group(_patients(), [0, 1, 2], [0.0, 1.0, 0.0])
    want = ["mmf_amil_infer_group", "mmf_dense_forward", "mmf_dense_forward"]
    want += ["mmf_xfusion_infer_group"] if fusion == "tensor" else []
    assert [n for n in rec.names if not n.endswith("_workspace_bytes")] == want + ["mmf_surv_head_infer_group"]
    (pf,), _ = _calls(rec, "mmf_amil_infer_group")
    (_, d1), _ = _calls(rec, "mmf_dense_forward")
    # omic first in path_omic: the reference's order of the concatenation (model_mm_attention_mil.py:178-182)
    if fusion == "tensor":
        (xf,), _ = _calls(rec, "mmf_xfusion_infer_group")
        assert xf[0]["m"] == 2 and xf[1] == [d1[12], pf[8]]
    else:
        (hd,), _ = _calls(rec, "mmf_surv_head_infer_group")
        assert hd[0] == [d1[12], pf[8]] and hd[1] == [256, 256] and hd[2] == 2


@pytest.mark.parametrize("fusion", ["concat", "tensor"])
def test_return_features_and_the_pre_stacked_window(fusion, rec):  # noqa: F811
    model = _model(fusion=fusion)
    window = ((torch.randn(15, 1024), PATH), (torch.randn(4, 12, 1024), RADIO), torch.randn(3, 80))
    feats = model.forward_group(window, return_features=True)
    assert feats.shape == ((3, 512) if fusion == "tensor" else (3, 768))
    assert "mmf_surv_head_infer_group" not in rec.names and not [n for n in rec.names if n in PER_PATIENT]
    assert ("mmf_xfusion_infer_group" in rec.names) == (fusion == "tensor")


@pytest.mark.parametrize("fusion", ["concat", "tensor"])
def test_refused_calls_make_no_abi_call(fusion, rec, monkeypatch):  # noqa: F811
    model = _model(fusion=fusion)
    pts = _patients()
    Y, c = [0, 1, 2], [0.0, 1.0, 0.0]
    bad = [
        ([dict(p, path_features=p["path_features"].to(torch.bfloat16)) for p in pts], Y, c),      # bf16 bags
        ([pts[0]] * 65, [0] * 65, [0.0] * 65),                                                     # G = 65
        ([pts[0], dict(pts[1], path_features=pts[1]["path_features"][:0])], Y[:2], c[:2]),         # an empty bag
        (((torch.randn(15, 1024), PATH), (torch.randn(4, 12, 1024), RADIO), torch.randn(2, 80)), Y, c),   # counts differ
        (pts, Y[:2], c[:2]),                                                                       # labels for two
    ]
    for args in bad:
        with pytest.raises((TypeError, _lib.MmfError)):
            model.forward_group(*args)
    with pytest.raises(_lib.MmfError):
        _model(fusion=fusion, K=33).forward_group(pts, Y, c)
    monkeypatch.setattr(ops, "_gemm", 1)
    with pytest.raises(_lib.MmfError):
        model.forward_group(pts, Y, c)
    monkeypatch.setattr(ops, "_gemm", 0)
    with pytest.raises(RuntimeError):
        model.train().forward_group(pts, Y, c)                                                     # training mode
    assert rec.calls == []
    model.eval().forward_group(pts, Y, c)                # a valid call afterwards still works
    assert "mmf_surv_head_infer_group" in rec.names


# ---- the evaluation loops -------------------------------------------------------------------------------------------
N_LOADER, BF16_AT = 70, 66


def _loader():
    g = torch.Generator().manual_seed(5)
    out = []
    for i in range(N_LOADER):
        n, r = 1 + i % 3, 1 + i % 2
        x = torch.randn(n, 1024, generator=g)
        out.append(({m: torch.randn(r, 1024, generator=g) for m in MODS}, x.to(torch.bfloat16) if i == BF16_AT else x,
                    torch.randn(1, 80, generator=g), torch.tensor([i % 4]), np.array([float(10 + i)]),
                    torch.tensor([float(i % 3 == 0)])))
    return out


def _validate(rec, monkeypatch, fusion, group, which="validate"):  # noqa: F811
    """validate_survival / summary_survival over 70 multimodal patients (patient 66 has a bf16 pathology bag) with the
    recorder as the library: the values are whatever the zeroed outputs hold, the calls are what is checked."""
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    monkeypatch.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **k))      # finite losses and risks for the statistics
    model = _model(fusion=fusion)
    regs = []
    reg_fn = lambda m: regs.append(1) or torch.zeros(())
    if which == "validate":
        core_utils.validate_survival(0, 0, model, _loader(), 4, "radio_path_omic", loss_fn=NLLSurvLoss(alpha=0.2),
                                     reg_fn=reg_fn, lambda_reg=1e-4, group=group)
    else:
        core_utils.summary_survival(model, _loader(), 4, "radio_path_omic", loss_fn=NLLSurvLoss(alpha=0.2), group=group)
    return [(n, a) for n, a, _ in rec.calls], len(regs)


@pytest.mark.parametrize("which", ["validate", "summary"])
@pytest.mark.parametrize("fusion", ["concat", "tensor"])
def test_loops_hold_multimodal_patients_and_flush_at_64_at_a_bf16_patient_and_at_the_end(fusion, which, rec, monkeypatch):  # noqa: F811
    calls, n_reg = _validate(rec, monkeypatch, fusion, True, which)
    heads = [a for n, a in calls if n == "mmf_surv_head_infer_group"]
    assert [a[3] for a in heads] == [64, 2, 3]                 # full, before the bf16 patient, the rest at the end
    # the stock NLLSurvLoss value comes from the kernel, with the per-patient branch's alpha = 0
    assert all((a[5] is not None and a[5]["alpha"] == 0.0) if which == "validate" else a[5] is None for a in heads)
    assert [n for n, _ in calls].count("mmf_xfusion_infer_group") == (3 if fusion == "tensor" else 0)
    # the held rows: each call's tables are the patients' sizes, in loader order
    order = [i for i in range(N_LOADER) if i != BF16_AT]
    sizes_p = [b - a for n, ar in calls if n == "mmf_amil_infer_group" for a, b in zip(ar[1]["offsets"], ar[1]["offsets"][1:])]
    sizes_r = [b - a for n, ar in calls if n == "mmf_radio_infer_group" for a, b in zip(ar[1]["offsets"], ar[1]["offsets"][1:])]
    assert sizes_p == [1 + i % 3 for i in order] and sizes_r == [1 + i % 2 for i in order]
    # the bf16 patient alone, on the one-bag route, between the second and the third grouped call
    names = [n for n, _ in calls]
    assert names.count("mmf_amil_bf16_infer") == 1 and names.count("mmf_amil_infer") == 1 and names.count("mmf_linear_forward") == 1
    at = names.index("mmf_amil_bf16_infer")
    assert names[:at].count("mmf_surv_head_infer_group") == 2
    if which == "validate":
        assert n_reg == 2                                      # once for the grouped patients, once for the one alone


@pytest.mark.parametrize("fusion", ["concat", "tensor"])
def test_without_group_the_calls_are_the_per_patient_calls(fusion, rec, monkeypatch):  # noqa: F811
    calls, n_reg = _validate(rec, monkeypatch, fusion, False)
    names = [n for n, _ in calls if not n.endswith("_workspace_bytes")]
    assert not [n for n in names if "group" in n] and n_reg == N_LOADER
    tail = ["mmf_xreduce_forward", "mmf_kron_forward", "mmf_dense_forward", "mmf_dense_forward", "mmf_dense_forward",
            "mmf_surv_head_forward"] if fusion == "tensor" else ["mmf_surv_head_forward"]
    one = lambda bf16: ["mmf_linear_forward", "mmf_amil_infer", "mmf_amil_bf16_infer" if bf16 else "mmf_amil_infer",
                        "mmf_dense_forward", "mmf_dense_forward"] + tail + ["mmf_nll_surv"]
    assert names == [n for i in range(N_LOADER) for n in one(i == BF16_AT)]
