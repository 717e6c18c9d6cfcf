"""GPU: the omic head's one-launch training step (mmf_maxnet_cox_step: MaxNet forward + CoxSurvLoss + backward;
models/model_genomic.py:53-72, models/model_modules.py:64-68, utils/loss_utils.py:124-139) against the golden fixtures made
from the reference, the live fp64 oracle, and the composable path (model() -> CoxSurvLoss -> backward)."""
import numpy as np
import pytest
import torch

from conftest import check_summary
from oracle import cases
from test_gpu_path import DEV, _load, _t

pytestmark = pytest.mark.gpu
NAMES = ["fc_omic.0.0.weight", "fc_omic.0.0.bias", "fc_omic.1.0.weight", "fc_omic.1.0.bias", "classifier.weight", "classifier.bias"]


def _model(m, sd):
    from multimodalfusion_amd.models import MaxNet
    model = _load(MaxNet(input_dim=m["G"], model_size_omic="small", bag_loss="cox_surv", n_classes=m["K"]), sd)
    return model.train() if m["train"] else model.eval()


def _step(model, x, t, c, **kw):
    for p in model.parameters():
        p.grad = None
    risk, loss = model.cox_step(x, t, c, **kw)
    torch.cuda.synchronize()
    return risk.cpu().numpy(), float(loss), {k: p.grad.cpu().numpy().copy() for k, p in model.named_parameters()}


def _check(res, ref, name):
    risk, loss, grads = res
    assert abs(loss - float(ref["loss"])) <= 1e-5 * max(1.0, abs(float(ref["loss"]))), name
    np.testing.assert_allclose(risk, ref["hazards"], atol=1e-4, err_msg=name)
    for k, gr in ref["grads"].items():
        assert float(np.abs(grads[k] - gr).max()) <= 1e-5 + 1e-4 * float(np.abs(gr).max()), (name, k)


def test_cox_step_golden_cases(golden, monkeypatch):
    from multimodalfusion_amd import ops
    g = golden("omic")
    ran = 0
    for name, m in g.meta.items():
        if m["nll"]:
            continue
        sd, x, t, c, keeps = cases.omic_inputs(m)
        model = _model(m, sd)
        if m["train"]:
            monkeypatch.setattr(ops, "next_dropout_seed", lambda: m["mask_seed"])
        assert model.cox_step_ok(_t(x))
        res = _step(model, _t(x), torch.as_tensor(t), _t(c))
        _check(res, cases.run_omic(m), name)
        tag = name + "/f64"
        assert abs(res[1] - float(g[tag + "/loss"])) <= 1e-5 * max(1.0, abs(float(g[tag + "/loss"])))
        for k, gr in res[2].items():
            check_summary(g, f"{tag}/grad/{k}", gr, rtol=1e-4, atol=1e-5)
        assert int(ops.sync_words(DEV).abs().sum()) == 0          # both barriers' counters are back to zero
        ran += 1
    assert ran >= 3


@pytest.mark.parametrize("B,G,train", [(128, 36, True), (2, 80, False), (200, 186, True), (129, 36, False), (256, 256, True), (7, 1, False)])
def test_cox_step_matches_oracle_and_the_composable_path(B, G, train, monkeypatch):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.utils.loss_utils import CoxSurvLoss
    m = dict(B=B, G=G, nll=False, K=4, train=train, seed=500 + B, x_seed=600 + G, mask_seed=31, bias_std=0.05, alpha=0.0, y=0)
    sd, x, t, c, keeps = cases.omic_inputs(m)
    model = _model(m, sd)
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: m["mask_seed"])
    xt, ct = _t(x), _t(c)
    tdev = torch.as_tensor(t).to(DEV)                 # float64, device-resident: no per-step copy
    res = _step(model, xt, tdev, ct)
    _check(res, cases.run_omic(m), f"B={B} G={G}")
    # the same numbers as the composable path (three dense launches, Cox, three dense backward launches) to fp32 rounding
    for p in model.parameters():
        p.grad = None
    risk = model(genomic_features=xt)[0]
    loss = CoxSurvLoss()(risks=risk, times=torch.as_tensor(t), c=ct)
    loss.backward()
    np.testing.assert_allclose(res[0], risk.detach().cpu().numpy().reshape(-1), rtol=0, atol=2e-6)
    assert abs(res[1] - float(loss)) <= 2e-6 * max(1.0, abs(float(loss)))
    for k, p in model.named_parameters():
        gr = p.grad.cpu().numpy()
        assert float(np.abs(res[2][k] - gr).max()) <= 1e-7 + 2e-5 * float(np.abs(gr).max()), k
    # bit-reproducible, loss_scale and accumulate semantics
    res2 = _step(model, xt, tdev, ct)
    assert np.array_equal(res[0], res2[0]) and res[1] == res2[1] and all(np.array_equal(res[2][k], res2[2][k]) for k in res[2])
    half = _step(model, xt, tdev, ct, loss_scale=0.5)
    for k in res[2]:
        np.testing.assert_allclose(half[2][k], 0.5 * res[2][k], rtol=1e-6, atol=1e-12)
    model.cox_step(xt, tdev, ct, loss_scale=0.5)        # .grad exists: accumulated on top
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), res[2][k], rtol=2e-6, atol=1e-9)
    assert int(ops.sync_words(DEV).abs().sum()) == 0


def test_shapes_the_step_does_not_take():
    from multimodalfusion_amd.models import MaxNet
    big = MaxNet(input_dim=36, model_size_omic="big", bag_loss="cox_surv").to(DEV)
    assert not big.cox_step_ok(torch.zeros(8, 36, device=DEV))
    small = MaxNet(input_dim=300, bag_loss="cox_surv").to(DEV)
    assert not small.cox_step_ok(torch.zeros(8, 300, device=DEV))
    nll = MaxNet(input_dim=36, bag_loss="nll_surv").to(DEV)
    assert not nll.cox_step_ok(torch.zeros(8, 36, device=DEV))
    ok = MaxNet(input_dim=36, bag_loss="cox_surv").to(DEV)
    assert ok.cox_step_ok(torch.zeros(8, 36, device=DEV)) and not ok.cox_step_ok(torch.zeros(300, 36, device=DEV))


def test_training_loop_takes_the_one_launch_step(monkeypatch):
    """train_loop_survival on an omic model with CoxSurvLoss goes through MaxNet.cox_step and ends where the composable path
    ends: same parameters after two Adam steps (train mode, the dropout seed pinned so that both paths draw the same masks)."""
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models import MaxNet
    from multimodalfusion_amd.utils import core_utils as cu
    from multimodalfusion_amd.utils.loss_utils import CoxSurvLoss
    m = dict(B=64, G=36, nll=False, K=4, train=True, seed=77, x_seed=78, mask_seed=0, bias_std=0.05, alpha=0.0, y=0)
    sd, x, t, c, _ = cases.omic_inputs(m)
    batches = [({}, torch.zeros(1, 1), torch.as_tensor(x), torch.zeros(64), t, torch.as_tensor(c)) for _ in range(2)]
    outs = []
    for fused in (True, False):
        model = _load(MaxNet(input_dim=36, bag_loss="cox_surv"), sd)
        opt = torch.optim.Adam(model.parameters(), lr=2e-4, weight_decay=1e-5)
        calls = []
        monkeypatch.setattr(ops, "next_dropout_seed", lambda: 123)
        if fused:
            orig = MaxNet.cox_step
            monkeypatch.setattr(MaxNet, "cox_step", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
        else:
            monkeypatch.setattr(cu, "_bag_route", lambda *a: "autograd")
        cu.train_loop_survival(0, model, batches, opt, 4, "omic", loss_fn=CoxSurvLoss(), gc=1)
        monkeypatch.undo()
        assert bool(calls) == fused
        outs.append({k: p.detach().cpu().numpy().copy() for k, p in model.named_parameters()})
    # Adam's first steps move every element by ~lr whatever its gradient's size, so an element whose gradient is rounding
    # noise around zero may step the other way in the other path: all but a handful agree to 2e-6, none is off by more
    # than the two steps' 2 x 2 lr
    for k in outs[0]:
        d = np.abs(outs[0][k] - outs[1][k])
        assert float(d.max()) <= 8e-4 + 1e-6 and int((d > 2e-6).sum()) <= max(1, d.size // 1000), (k, float(d.max()), int((d > 2e-6).sum()))
