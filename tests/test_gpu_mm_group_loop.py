"""GPU: train_loop_survival(..., group=True) with the multimodal concat head -- each accumulation window's patients held on
the device (a pathology plane, the radio planes, the omic rows) and run as one grouped call (model.nll_step_group).  On a
ragged loader (gc = 4, dropout on, one patient with a bf16 pathology bag that flushes the group and runs alone, a
trailing partial window, a window split by the row limit) it gives the per-patient loop's losses and parameters after
every optimizer step; a tensor-fusion model under group=True keeps the per-patient route."""
import numpy as np
import pytest
import torch

from oracle import inputs as gen

pytestmark = pytest.mark.gpu

MODS = ["T1", "T2", "T1Gd", "FLAIR"]
PATH = [300, 41, 700, 128, 9, 250, 512, 64, 77, 600]
RADIO = [40, 8, 96, 1, 30, 64, 17, 50, 12, 72]
BF16_AT = 5                        # this patient's pathology bag is bf16: not grouped, flushes the held ones, runs alone


def _loader():
    loader = []
    for i, (n, r) in enumerate(zip(PATH, RADIO)):
        radio = {m: torch.as_tensor(gen.bag(700 + i, r, stream=7 * j)) for j, m in enumerate(MODS)}
        path = torch.as_tensor(gen.bag(900 + i, n, stream=100))
        if i == BF16_AT:
            path = path.to(torch.bfloat16)
        omic = torch.as_tensor(gen.normal(500 + i, (1, 80), stream=200))
        loader.append((radio, path, omic, torch.tensor([i % 4]), np.array([float(10 + i)]), torch.tensor([float(i % 3 == 0)])))
    return loader


def _run(group, monkeypatch, fusion="concat", row_limits=None):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import MM_MIL_Attention_fc_surv
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    sd = gen.mm_state_dict(seed=616, input_dim=80, fusion=fusion, gate_path=True, gate_radio=True, dropout=True,
                           n_classes=4, mode="radio_path_omic", n_mod=4, bias_std=0.05)
    model = MM_MIL_Attention_fc_surv(input_dim=80, radio_fusion="concat", fusion=fusion, gate=True, gate_path=True,
                                     gate_omic=True, gate_radio=True, dropout=True, n_classes=4, mode="radio_path_omic")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    model.relocate()
    seeds = iter(range(8001, 8200))
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: next(seeds))
    if row_limits is not None:
        monkeypatch.setattr(ops, "mm_group_row_limits", lambda **kw: row_limits)
    calls = {"group": [], "single": 0}
    g0, s0 = model.nll_step_group, model.nll_step

    def g(window, *a, **k):
        calls["group"].append(len(window[2]))
        return g0(window, *a, **k)

    def s(*a, **k):
        calls["single"] += 1
        return s0(*a, **k)

    model.nll_step_group, model.nll_step = g, s
    # SGD, as the pathology and radiology grouped loop tests: its update is linear in the gradient, so the parameter bar
    # below bounds the routes' gradient difference.  Adam's g / (sqrt(v) + eps) is not: where a gradient element nearly
    # cancels, fp32 rounding alone moves the first step by a sizeable share of lr.  On this loader's first window the
    # fp64 and fp32 evaluations of the SAME formulas on the CPU (gradients equal to 3e-7 of the tensor's max) end 5.8e-5
    # apart in reduce_dim.weight after one Adam(lr = 1e-3) step, past the 5.2e-5 bar; after one SGD(lr = 0.05) step they
    # are at 3e-4 of the bar.  The grouped and per-patient routes differ by fp32 rounding by construction (other tile
    # plans), so under Adam the bar would measure the optimizer's conditioning, not the routes.
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    snaps = []

    class Opt:
        def step(self):
            opt.step()
            snaps.append({k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})

        def zero_grad(self):
            opt.zero_grad()

    out = core_utils.train_loop_survival(0, model, _loader(), Opt(), 4, "radio_path_omic", loss_fn=NLLSurvLoss(alpha=0.2),
                                         gc=4, group=group)
    torch.cuda.synchronize()
    return out, snaps, calls


def _same(a, snaps_a, b, snaps_b):
    """The bars of test_gpu_mm_step.test_loop_takes_the_one_call_step_and_matches_the_autograd_route."""
    print("losses: max |grouped - per patient| / |per patient| =", float(np.abs(b["losses"] / a["losses"] - 1).max()))
    np.testing.assert_allclose(b["losses"], a["losses"], rtol=1e-5, atol=1e-6)
    assert len(snaps_a) == len(snaps_b) == 2
    for i, (sa, sb) in enumerate(zip(snaps_a, snaps_b)):
        worst = max((float(np.abs(sb[k] - v).max()) / (5e-5 + 2e-5 * float(np.abs(v).max())), k) for k, v in sa.items())
        print(f"step {i}: largest parameter difference as a share of its bar: {worst[0]:.3e} ({worst[1]})")
        for k, v in sa.items():
            d = float(np.abs(sb[k] - v).max())
            assert d <= 5e-5 + 2e-5 * float(np.abs(v).max()), (k, d)


@pytest.mark.parametrize("row_limits", [None, (1000, 100000), (100000, 100)])
def test_grouped_mm_loop_equals_the_per_patient_loop(row_limits, monkeypatch):
    a, snaps_a, calls_a = _run(False, monkeypatch)
    monkeypatch.undo()
    b, snaps_b, calls_b = _run(True, monkeypatch, row_limits=row_limits)
    assert calls_a["group"] == [] and calls_a["single"] == 10
    assert calls_b["group"], "grouped call was made"
    assert calls_b["single"] == 1                          # the bf16 patient alone
    # windows: positions 0-3; 4-7, where the bf16 patient at 5 flushes {4} and runs alone, then {6, 7}; trailing 8-9.
    # A 1,000-row pathology limit splits the first window after 300 + 41 (+ 700 > 1000); a 100-row radio limit after 40 + 8.
    want = {None: [4, 1, 2, 2], (1000, 100000): [2, 2, 1, 2, 2], (100000, 100): [2, 2, 1, 2, 2]}[row_limits]
    assert calls_b["group"] == want, calls_b
    _same(a, snaps_a, b, snaps_b)


def test_tensor_fusion_under_group_takes_the_per_patient_route(monkeypatch):
    out, snaps, calls = _run(True, monkeypatch, fusion="tensor")
    assert calls["group"] == [] and calls["single"] == 10
    assert len(snaps) == 2 and np.isfinite(out["losses"]).all()
