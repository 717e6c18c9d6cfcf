"""The multimodal concat head's fused integrated-gradients call (model.integrated_gradients, one mmf_mm_ig) in a loop, beside
the two single-head calls on the same bags: the target of rocprofv3 --kernel-trace --stats runs (tools/ig_bench.py --head mm
has the model and the inputs); `tensor`: the tensor-fusion head's call (model.integrated_gradients_tensor, one mmf_mm_ig_tensor)
on a fusion='tensor' model.  usage: mm_ig_profile.py N_p N_r [calls] [fused|single|tensor]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodalfusion_amd import ops
from multimodalfusion_amd.models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
from multimodalfusion_amd.models.model_modules import stack_args

MODS = ["T1", "T2", "T1Gd", "FLAIR"]
Np, Nr = int(sys.argv[1]), int(sys.argv[2])
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
what = sys.argv[4] if len(sys.argv) > 4 else "fused"
dev = torch.device("cuda", 0)
torch.manual_seed(0)
with torch.no_grad():
    model = MM_MIL_Attention_fc_surv(input_dim=80, fusion="tensor" if what == "tensor" else "concat", dropout=False, n_classes=4,
                                     mode="radio_path_omic").to(dev).eval()
    for b in (model.attention_net_WSI[0].bias, model.attention_net_radio[0].bias, model.reduce_dim.bias,
              model.fc_omic[0][0].bias, model.fc_omic[1][0].bias):
        b.normal_(0.0, 0.1)
feats = {m: torch.randn(Nr, 1024, device=dev) for m in MODS}
feats["path_features"] = torch.randn(Np, 1024, device=dev)
feats["genomic_features"] = torch.randn(80, device=dev)
a, w = (v.astype(np.float32) for v in ops.ig_quadrature("gausslegendre", 20))
if what == "single":
    _, cols, _ = model._concat_layout()
    Wk, bk = model.classifier.weight, model.classifier.bias
    gp, sp, _, _ = stack_args(model.attention_net_WSI, False)
    gr, sr, _, _ = stack_args(model.attention_net_radio, False)
    Wk_p, Wk_r = Wk[:, cols["path"]].contiguous(), Wk[:, cols["radio"]].contiguous()
with torch.no_grad():
    for _ in range(calls):
        if what == "fused":
            model.integrated_gradients(n_steps=20, **feats)
        elif what == "tensor":
            model.integrated_gradients_tensor(n_steps=20, **feats)
        else:
            ops.amil_integrated_gradients(feats["path_features"], sp, Wk_p, bk, gp, a, w)
            ops.radio_integrated_gradients([feats[m] for m in MODS], model.reduce_dim.weight, model.reduce_dim.bias, sr, Wk_r, bk,
                                           gr, a, w)
torch.cuda.synchronize()
print(f"{what}: {calls} calls at N_p={Np} N_r={Nr}")
