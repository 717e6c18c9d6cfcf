"""GPU parity of the attention scorer called on its own -- Attn_Net / Attn_Net_Gated .forward(x) -> (A, x)
(models/model_modules.py:70-110 of the reference; C ABI mmf_attn_net_forward / _backward) -- against the fp64 oracle
(oracle/torch_port.attn_net): scores 1e-4, every gradient (parameters and the input) 1e-5 + 1e-4 max|g|."""
import numpy as np
import pytest
import torch

from oracle import inputs as gen
from oracle import torch_port as tp
from test_gpu_path import DEV, _t

pytestmark = pytest.mark.gpu


def _case(N, L, D, gated, dropout, train, seed):
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.models.model_modules import Attn_Net, Attn_Net_Gated
    torch.manual_seed(seed)
    net = (Attn_Net_Gated if gated else Attn_Net)(L=L, D=D, dropout=dropout, n_classes=1)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    x = gen.normal(seed, (N, L), stream=3)
    gA = gen.normal(seed, (N, 1), stream=4)
    net = net.to(DEV)
    net.train() if train else net.eval()
    return net, sd, x, gA


@pytest.mark.parametrize("N,L,D,gated,dropout,train", [
    (1, 256, 256, True, False, False),
    (777, 256, 256, True, True, True),       # train mode: both branch masks, rebuilt by the oracle from the same hash
    (1000, 512, 384, False, True, True),     # the `big` scorer, ungated
    (4099, 256, 256, False, False, False),
    (20011, 256, 256, True, False, False),   # the large-bag kernels (wide K-dh tile without its fused prep, 256x256 K-tn)
    (16384, 256, 256, True, False, False),   # exactly the wide threshold: the one bag size on the 64-row K-dh tile without fused prep
])
def test_attn_net_forward_backward(N, L, D, gated, dropout, train, monkeypatch):
    from multimodalfusion_amd import ops
    net, sd, x, gA = _case(N, L, D, gated, dropout, train, seed=100 + N)
    mask_seed = 5151
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: mask_seed)
    xt = _t(x).requires_grad_(True)
    A, x_out = net(xt)
    assert x_out is xt and tuple(A.shape) == (N, 1)
    A.backward(_t(gA))
    # oracle
    masks = None
    if train and dropout:
        masks = {"a": torch.as_tensor(gen.drop_scale_mask(mask_seed, 1, N, D, 0.25, np.float64))}
        if gated:
            masks["b"] = torch.as_tensor(gen.drop_scale_mask(mask_seed, 2, N, D, 0.25, np.float64))
    tsd = tp.to_torch({"s." + k: v for k, v in sd.items()}, torch.float64)
    xr = torch.as_tensor(x).double().requires_grad_(True)
    A_r, _ = tp.attn_net(tsd, "s", xr, gated, dropout, masks)
    A_r.backward(torch.as_tensor(gA).double())
    np.testing.assert_allclose(A.detach().cpu().numpy(), A_r.detach().numpy(), rtol=0, atol=1e-4)
    got = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}
    got["x"] = xt.grad.cpu().numpy()
    ref = {k[2:]: v.grad.numpy() for k, v in tsd.items()}
    ref["x"] = xr.grad.numpy()
    for k, g in ref.items():
        tol = 1e-5 + 1e-4 * float(np.abs(g).max())
        assert float(np.abs(got[k] - g).max()) <= tol, (k, float(np.abs(got[k] - g).max()), tol)


def test_attn_net_matches_the_fused_head_scores():
    """The scorer on h = relu(x W1^T + b1) gives the head's A_raw (same kernels, same order of operations)."""
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    torch.manual_seed(9)
    model = MIL_Attention_fc_surv_path(gate_path=True, n_classes=4).to(DEV).eval()
    x = torch.randn(3000, 1024, device=DEV)
    with torch.no_grad():
        A_head = model(path_features=x, attention_only=True)
        h = torch.relu(torch.nn.functional.linear(x, model.attention_net_WSI[0].weight, model.attention_net_WSI[0].bias))
        A, _ = model.attention_net_WSI[3](h)
    np.testing.assert_allclose(A.T.cpu().numpy(), A_head.cpu().numpy(), rtol=0, atol=2e-5)
