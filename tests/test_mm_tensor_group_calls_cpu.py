"""The C-ABI calls behind MM_MIL_Attention_fc_surv.nll_step_group_tensor, without a GPU (the recorder of
test_ops_calls_cpu stands in for the library): their order on the one stream -- radio forward, pathology forward, omic
forward, fusion forward, head, fusion backward, pathology backward, omic backward, radio backward --, that no per-patient
fusion or stack call is made, the per-patient seeds (drawn in nll_step's order: radio, path, omic, fusion), the row_base and
the two probabilities handed to the fusion calls, every branch writing its own columns of encoder2's input matrix, that a
refused call makes no C-ABI call at all, and the training loop's opt-in (model.mmf_group_tensor)."""
import pytest
import torch

from multimodalfusion_amd import _lib, ops
from test_mm_group_calls_cpu import MODS, PATH, RADIO, _loop, _model, _patients
from test_ops_calls_cpu import STREAM, rec  # noqa: F401  (fixture)

FWD, BWD = "mmf_xfusion_group_forward", "mmf_xfusion_group_backward"
FUSION_PER_PATIENT = ("mmf_kron_", "mmf_xreduce_", "mmf_gate_mul_")       # the one-patient fusion tail's entry points
ONE_PATIENT = {"mmf_amil_forward", "mmf_amil_backward", "mmf_amil_head_forward", "mmf_amil_nll_step", "mmf_linear_forward",
               "mmf_linear_backward", "mmf_dense_forward", "mmf_dense_backward", "mmf_surv_head_nll_step"}


def _no_per_patient_calls(names):
    for n in names:
        assert not n.startswith(FUSION_PER_PATIENT) and n not in ONE_PATIENT, n


def test_call_order_seeds_masks_and_feature_columns(rec, monkeypatch):  # noqa: F811
    seeds = iter(range(100, 200))
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: next(seeds))
    model = _model(fusion="tensor")
    out = model.nll_step_group_tensor(_patients(), [0, 1, 2], [0.0, 1.0, 0.0], alpha=0.2, loss_scale=0.25)
    log, sizes = rec.log()
    names = [n for n, _, _ in log]
    assert names == ["mmf_radio_group_workspace_bytes", "mmf_radio_group_forward",
                     "mmf_amil_group_workspace_bytes", "mmf_amil_group_forward",
                     "mmf_dense_forward_rows", "mmf_dense_forward_rows",
                     "mmf_xfusion_group_workspace_bytes", FWD,
                     "mmf_surv_head_group_workspace_bytes", "mmf_surv_head_nll_step_group",
                     BWD,
                     "mmf_amil_group_backward", "mmf_dense_backward_rows", "mmf_dense_backward_rows",
                     "mmf_radio_group_backward"]
    _no_per_patient_calls(names)
    call = {}
    for n, a, r in log:
        call.setdefault(n, []).append((a, r))
    rf, pf = call["mmf_radio_group_forward"][0][0], call["mmf_amil_group_forward"][0][0]
    rb, pb = call["mmf_radio_group_backward"][0][0], call["mmf_amil_group_backward"][0][0]
    # the seeds of patient g are draws 4g (radio), 4g + 1 (path), 4g + 2 (omic), 4g + 3 (fusion)
    assert rf[1] == {"G": 3, "offsets": [0, 2, 9, 12], "seeds": [100, 104, 108]}
    assert pf[1] == {"G": 3, "offsets": [0, 5, 6, 15], "seeds": [101, 105, 109]}
    bases = {tuple(int(v) & 0xFFFFFFFF for v in t.tolist()): p for p, t in rec.tensors.items() if t.dtype == torch.int32}
    inv = lambda ss: tuple((s * ops._HASH_MUL_INV) & 0xFFFFFFFF for s in ss)
    assert set(bases) == {inv((102, 106, 110)), inv((103, 107, 111))}
    (fq, fbytes), = call["mmf_xfusion_group_workspace_bytes"]
    assert fq == [3, 256, 16, 512, 512, 256, 3]
    (xf, _), = call[FWD]
    (xb, _), = call[BWD]
    w, x2, G, p, pc, base, word, ws, nb, MM, hid, stream = xf
    assert (G, p, pc, word, stream) == (3, 0.25, 0.25, None, STREAM)
    raw_fwd = [a for n, a, _ in rec.calls if n == FWD][0]
    assert raw_fwd[5] == bases[inv((103, 107, 111))]                  # row_base = seed . _HASH_MUL_INV of the FUSION seeds
    d0, d1 = (a for a, _ in call["mmf_dense_forward_rows"])
    raw_d0 = [a for n, a, _ in rec.calls if n == "mmf_dense_forward_rows"][0]
    assert raw_d0[11] == bases[inv((102, 106, 110))]                  # ... and of the omic seeds for the omic batch
    assert nb == fbytes and sizes[ws] == fbytes
    assert (w["m"], w["dim"], w["sdim"], w["mmhid1"], w["mmhid2"], w["nhid"]) == (3, 256, 16, 512, 512, 256)
    # one [3 x 1280] matrix: encoder1's 512 columns, then radio, pathology, omic; the stacks write through ldm = 1280
    K2 = 512 + 3 * 256
    assert sizes[x2] == 3 * K2 * 4
    assert (rf[5], rf[6]) == (f"{x2}+{512 * 4}", K2) and (pf[5], pf[6]) == (f"{x2}+{768 * 4}", K2)
    assert (d1[12], d1[13]) == (f"{x2}+{1024 * 4}", K2) and d0[13] == 256
    # the head: classifier[3] on hid [3 x 256]
    head = call["mmf_surv_head_nll_step_group"][0][0]
    assert (head[0], head[1], head[2], head[3]) == (hid, 256, 256, 3) and head[4]["K"] == 4
    assert head[5]["loss_scale"] == 0.25 and head[5]["accumulate"] == 0
    dhid = head[6]
    # the backward: the forward's operands and workspace, dhid from the head, fresh gradients written
    bw, bx2, bG, bp, bpc, bbase, bword, bMM, bhid, bdhid, ldd, bws, bnb, dx2, grads, acc, bstream = xb
    assert (bx2, bG, bp, bpc, bbase, bword, bMM, bhid) == (x2, G, p, pc, base, word, MM, hid)
    assert (bdhid, ldd, bws, bnb, acc, bstream) == (dhid, 256, ws, nb, 0, STREAM) and bw == w
    assert sizes[dx2] == 3 * K2 * 4
    ptrs = [v for k in ("dWh", "dbh", "dWz", "dbz", "dWo", "dbo") for v in grads[k]] + \
        [grads[k] for k in ("dWe1", "dbe1", "dWe2", "dbe2", "dWc0", "dbc0")]
    assert None not in ptrs and len(set(ptrs)) == 24
    assert sizes[grads["dWe1"]] == 512 * 17 ** 3 * 4
    # the branches' backward halves read their columns of dx2
    assert (rb[5], rb[6]) == (f"{dx2}+{512 * 4}", K2) and (pb[5], pb[6]) == (f"{dx2}+{768 * 4}", K2)
    b1, b0 = (a for a, _ in call["mmf_dense_backward_rows"])
    assert (b1[0], b1[1], b1[2], b1[3]) == (f"{dx2}+{1024 * 4}", K2, f"{x2}+{1024 * 4}", K2)
    hz, S, Y_hat, A_raw, loss, risk = out
    assert hz.shape == (3, 4) and Y_hat.shape == (3,) and loss.shape == (3,) and risk.shape == (3,)
    assert [a.shape[1] for a in A_raw["radiology"]] == RADIO and [a.shape[1] for a in A_raw["pathology"]] == PATH
    assert all(p.grad is not None for p in model.parameters())


def test_eval_mode_passes_zero_probabilities_and_draws_no_seed(rec, monkeypatch):  # noqa: F811
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: pytest.fail("eval mode drew a dropout seed"))
    model = _model(fusion="tensor").eval()
    model.nll_step_group_tensor(_patients(), [0, 1, 2], [0.0, 1.0, 0.0])
    xf = [a for n, a, _ in rec.calls if n == FWD][0]
    xb = [a for n, a, _ in rec.calls if n == BWD][0]
    assert (xf[3], xf[4]) == (0.0, 0.0) and (xb[3], xb[4]) == (0.0, 0.0)
    (base,) = {p for p, t in rec.tensors.items() if t.dtype == torch.int32 and p == xf[5]}
    assert rec.tensors[base].tolist() == [0, 0, 0]


@pytest.mark.parametrize("mode,want,order", [
    ("radio_path", ["mmf_radio_group_forward", "mmf_amil_group_forward", FWD, "mmf_surv_head_nll_step_group", BWD,
                    "mmf_amil_group_backward", "mmf_radio_group_backward"], ["radio", "path"]),
    ("path_omic", ["mmf_amil_group_forward", "mmf_dense_forward_rows", "mmf_dense_forward_rows", FWD,
                   "mmf_surv_head_nll_step_group", BWD, "mmf_amil_group_backward", "mmf_dense_backward_rows",
                   "mmf_dense_backward_rows"], ["omic", "path"]),
    ("radio_omic", ["mmf_radio_group_forward", "mmf_dense_forward_rows", "mmf_dense_forward_rows", FWD,
                    "mmf_surv_head_nll_step_group", BWD, "mmf_dense_backward_rows", "mmf_dense_backward_rows",
                    "mmf_radio_group_backward"], ["radio", "omic"]),
])
def test_modes_run_their_branches_only(mode, want, order, rec):  # noqa: F811
    model = _model(mode, fusion="tensor")
    model.nll_step_group_tensor(_patients(), [0, 1, 2], [0.0, 1.0, 0.0])
    assert [n for n in rec.names if not n.endswith("_workspace_bytes")] == want
    xf = [a for n, a, _ in rec.calls if n == FWD][0]
    assert xf[0]["m"] == 2
    x2, K2 = xf[1], 512 + 2 * 256
    at = {"radio": [a for n, a, _ in rec.calls if n == "mmf_radio_group_forward"],
          "path": [a for n, a, _ in rec.calls if n == "mmf_amil_group_forward"],
          "omic": [a for n, a, _ in rec.calls if n == "mmf_dense_forward_rows"][1:]}
    for i, k in enumerate(order):          # branch k writes modality slot i of _concat_order() (omic first in path_omic)
        a = at[k][0]
        where, ld = (a[12], a[13]) if k == "omic" else (a[5], a[6])
        assert (where, ld) == (x2 + (512 + 256 * i) * 4, K2), k


def test_refused_calls_make_no_abi_call(rec, monkeypatch):  # noqa: F811
    model = _model(fusion="tensor")
    pts = _patients()
    Y, c = [0, 1, 2], [0.0, 1.0, 0.0]
    with pytest.raises(NotImplementedError):
        _model(fusion="concat").nll_step_group_tensor(pts, Y, c)                                  # the concat head
    noskip = _model(fusion="tensor")
    noskip.mm.skip = 0
    with pytest.raises(NotImplementedError):
        noskip.nll_step_group_tensor(pts, Y, c)                                                    # what nll_step refuses
    bad = [
        ([dict(p, path_features=p["path_features"].to(torch.bfloat16)) for p in pts], Y, c),      # bf16 bags
        ([pts[0]] * 65, [0] * 65, [0.0] * 65),                                                     # G = 65
        ([pts[0], dict(pts[1], path_features=pts[1]["path_features"][:0])], Y[:2], c[:2]),         # an empty bag
        (((torch.randn(15, 1024), PATH), (torch.randn(4, 12, 1024), RADIO), torch.randn(2, 80)), Y, c),   # counts differ
        (pts, Y[:2], c[:2]),                                                                       # labels for two
    ]
    for args in bad:
        with pytest.raises((TypeError, _lib.MmfError)):
            model.nll_step_group_tensor(*args)
    with pytest.raises(_lib.MmfError):
        model.nll_step_group_tensor(pts, Y, c, seeds={"radio": [1, 2, 3], "path": [1, 2, 3], "omic": [1, 2, 3]})   # no fusion seeds
    with pytest.raises(_lib.MmfError):
        _model(fusion="tensor", K=33).nll_step_group_tensor(pts, Y, c)
    monkeypatch.setattr(ops, "_gemm", 1)
    with pytest.raises(_lib.MmfError):
        model.nll_step_group_tensor(pts, Y, c)
    assert rec.calls == []
    monkeypatch.setattr(ops, "_gemm", 0)
    model.nll_step_group_tensor(pts, Y, c)           # a valid call afterwards still works
    assert FWD in rec.names and BWD in rec.names


def _tensor_loop(rec, monkeypatch, opt_in, row_limits=None):  # noqa: F811
    import multimodalfusion_amd.models.model_mm_attention_mil as mod
    if opt_in:                        # _loop builds the model itself: every instance it makes opts in
        init = mod.MM_MIL_Attention_fc_surv.__init__

        def opted(self, *a, **k):
            init(self, *a, **k)
            self.mmf_group_tensor = True
        monkeypatch.setattr(mod.MM_MIL_Attention_fc_surv, "__init__", opted)
    return _loop(rec, monkeypatch, fusion="tensor", row_limits=row_limits)


@pytest.mark.parametrize("row_limits,want", [(None, [4, 1, 2, 2]), ((1000, 100000), [2, 2, 1, 2, 2]),
                                             ((100000, 100), [2, 2, 1, 2, 2])])
def test_loop_groups_tensor_windows_when_the_model_opts_in(row_limits, want, rec, monkeypatch):  # noqa: F811
    """gc = 4 over ten patients, patient 5 with a bf16 pathology bag: the held patients flush at the window's end, at a row
    limit, at the bf16 patient and at the end of the pass (GROUP_MAX: test_loop_flushes_a_full_tensor_group)."""
    calls = _tensor_loop(rec, monkeypatch, True, row_limits)
    fwd = [a for n, a in calls if n == FWD]
    assert [a[2] for a in fwd] == want and [a[2] for n, a in calls if n == BWD] == want
    heads = [a for n, a in calls if n == "mmf_surv_head_nll_step_group"]
    assert [a[3] for a in heads] == want and all(a[5]["loss_scale"] == 0.25 for a in heads)
    assert all((a[3], a[4]) == (0.25, 0.25) for a in fwd)
    assert [n for n, _ in calls].count("mmf_amil_bf16_forward") == 1          # the bf16 patient runs alone
    # seeds in arrival order: patient i draws 1000 + 4 i (radio), + 1 (path), + 2 (omic), + 3 (fusion), grouped or alone
    order = [0, 1, 2, 3, 4, 6, 7, 8, 9]
    got_r = [s for n, a in calls if n == "mmf_radio_group_forward" for s in a[1]["seeds"]]
    got_p = [s for n, a in calls if n == "mmf_amil_group_forward" for s in a[1]["seeds"]]
    assert got_r == [1000 + 4 * i for i in order] and got_p == [1001 + 4 * i for i in order]
    inv = lambda s: (s * ops._HASH_MUL_INV) & 0xFFFFFFFF
    got_f = [int(v) & 0xFFFFFFFF for a in fwd for v in rec.tensors[a[5]].tolist()]
    assert got_f == [inv(1003 + 4 * i) for i in order]
    sizes_p = [b - a for n, ar in calls if n == "mmf_amil_group_forward"
               for a, b in zip(ar[1]["offsets"], ar[1]["offsets"][1:])]
    assert sizes_p == [300, 41, 700, 128, 9, 512, 64, 77, 600]


def test_loop_without_the_attribute_makes_no_grouped_call(rec, monkeypatch):  # noqa: F811
    names = [n for n, _ in _tensor_loop(rec, monkeypatch, False)]
    assert not [n for n in names if "group" in n]


def test_loop_flushes_a_full_tensor_group(rec, monkeypatch):  # noqa: F811
    """70 eligible patients in one accumulation window (gc = 70): the group flushes at ops.GROUP_MAX, then at the end."""
    import numpy as np
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    monkeypatch.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **k))
    model = _model(fusion="tensor")
    model.mmf_group_tensor = True
    loader = [({m: torch.randn(2, 1024) for m in MODS}, torch.randn(3, 1024), torch.randn(1, 80), torch.tensor([i % 4]),
               np.array([float(10 + i)]), torch.tensor([float(i % 3 == 0)])) for i in range(70)]
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    core_utils.train_loop_survival(0, model, loader, opt, 4, "radio_path_omic", loss_fn=NLLSurvLoss(alpha=0.2), gc=70,
                                   group=True)
    assert [a[2] for n, a, _ in rec.calls if n == FWD] == [ops.GROUP_MAX, 70 - ops.GROUP_MAX]


def test_a_concat_models_seeds_stay_three(rec, monkeypatch):  # noqa: F811
    """The fourth seed is the tensor fusion's alone: a concat model's grouped call still gets {"radio", "path", "omic"}, and
    so does a tensor model's window only with "fusion" added."""
    seen = {}
    for fusion in ("concat", "tensor"):
        import multimodalfusion_amd.models.model_mm_attention_mil as mod
        name = "nll_step_group" if fusion == "concat" else "nll_step_group_tensor"
        real = getattr(mod.MM_MIL_Attention_fc_surv, name)

        def spy(self, *a, seeds=None, _real=real, _f=fusion, **k):
            seen.setdefault(_f, []).append(set(seeds))
            return _real(self, *a, seeds=seeds, **k)
        monkeypatch.setattr(mod.MM_MIL_Attention_fc_surv, name, spy)
    _loop(rec, monkeypatch, fusion="concat")
    _tensor_loop(rec, monkeypatch, True)
    assert seen["concat"] and all(s == {"radio", "path", "omic"} for s in seen["concat"])
    assert seen["tensor"] and all(s == {"radio", "path", "omic", "fusion"} for s in seen["tensor"])
