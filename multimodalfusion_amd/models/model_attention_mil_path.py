"""Pathology attention-MIL head; drop-in for models/model_attention_mil_path.py of the reference
(same class names, ctor signatures :13 / :46, forward(**kwargs) contract :50-72, state_dict keys)."""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

from ..utils.utils import initialize_weights
from .model_modules import (AMIL_SIZES, amil_stack, amil_stack_head, amil_stack_ig, amil_stack_infer_group,
                            amil_stack_nll_step, amil_stack_nll_step_group, make_amil_stack)

PatchAttribution = namedtuple("PatchAttribution", ["patch_attr", "patch_abs", "total", "total_abs", "risk", "risk_baseline",
                                                   "delta", "step_risk", "attr"])


class MIL_Attention_fc_path(nn.Module):
    """Parameter container: `attention_net_WSI` (the stack) and `classifier`; the arithmetic lives in the HIP kernels."""

    def __init__(self, gate_path=True, dropout=True, model_size_wsi: str = "small", n_classes=4):
        super().__init__()
        self.size_dict_WSI = {name: list(dims) for name, dims in AMIL_SIZES.items()}
        self.attention_net_WSI = make_amil_stack(model_size_wsi, gated=gate_path, att_dropout=dropout)
        self.classifier = nn.Linear(AMIL_SIZES[model_size_wsi][1], n_classes)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def forward(self, h, return_features=False, attention_only=False):
        pass            # abstract in the reference too (:42-43)


class MIL_Attention_fc_surv_path(MIL_Attention_fc_path):
    def __init__(self, gate_path=True, model_size_wsi: str = "small", dropout=False, n_classes=4):
        super().__init__(gate_path=gate_path, model_size_wsi=model_size_wsi, dropout=dropout, n_classes=n_classes)

    def forward(self, **kwargs):
        bag = kwargs["path_features"]
        want_embedding, want_scores = kwargs.get("return_features"), kwargs.get("attention_only")
        if want_embedding or want_scores:
            M, A_raw = amil_stack(self.attention_net_WSI, bag, self.training)
            return M if want_embedding else A_raw
        # (hazards, S, Y_hat, A_raw): stack + classifier + hazard head as one autograd node
        return amil_stack_head(self.attention_net_WSI, self.classifier, bag, self.training)

    def nll_step(self, path_features, label, c, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None):
        """Extension of the reference surface (the training loop mirror uses it, utils/core_utils.py): forward +
        NLLSurvLoss(alpha) + backward of one bag in ONE C-ABI call -- what `hazards, S, Y_hat, A_raw = model(...)`,
        `loss = loss_fn(hazards=hazards, S=S, Y=label, c=c)`, `(loss * loss_scale).backward()` compute together
        (models/model_attention_mil_path.py:50-72 + utils/loss_utils.py:22-39 + autograd), with the same dropout draw.
        Gradients land in the parameters' .grad (accumulated) -- or in `grad_out`, tensors in self.parameters() order,
        overwritten unless `accumulate`; returns (hazards, S, Y_hat, A_raw, loss, risk)."""
        if any(not p.requires_grad for p in self.parameters()):
            raise RuntimeError("nll_step needs every parameter of the head to require grad")
        return amil_stack_nll_step(self.attention_net_WSI, self.classifier, path_features, self.training, label, c,
                                   alpha, loss_scale, grad_out, accumulate)

    def nll_step_group(self, bags, labels, censors, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None, seeds=None):
        """nll_step for the G bags of one accumulation window in ONE C-ABI call (ops.amil_nll_step_group): the stack's
        GEMMs run once over all of their rows.  bags: a list of [N_g x 1024] fp32 device tensors or an (x_cat, sizes)
        pair; labels / censors: G values.  Gradients of sum_g loss_g * loss_scale, same conventions as nll_step; in train
        mode bag g draws the dropout seed the g-th of G nll_step calls would (or `seeds[g]` when given).  Returns (hazards [G x K], S [G x K],
        Y_hat [G x 1], [A_raw [1 x N_g]], loss [G], risk [G])."""
        if any(not p.requires_grad for p in self.parameters()):
            raise RuntimeError("nll_step_group needs every parameter of the head to require grad")
        return amil_stack_nll_step_group(self.attention_net_WSI, self.classifier, bags, self.training, labels, censors,
                                         alpha, loss_scale, grad_out, accumulate, seeds)

    def forward_group(self, bags, labels=None, censors=None, alpha=0.0, return_features=False):
        """The eval-mode forward of G bags in ONE C-ABI call (ops.amil_infer_group) -- validation, summary and export
        evaluate one bag at a time with fixed weights (utils/core_utils.py:267-430 of the reference), and the bags are
        independent: the stack's GEMMs run once over all of their rows, pooling and the head per bag.  bags: a list of
        [N_g x 1024] fp32 / bf16 device tensors or an (x_cat, sizes) pair; labels / censors: G values for each bag's
        NLLSurvLoss(alpha) value, or None.  Each bag gets what `model(path_features=bag)` gives it under no_grad, to fp32
        rounding.  Returns (hazards [G x K], S [G x K], Y_hat [G x 1], [A_raw [1 x N_g]], loss [G] or None, risk [G]);
        return_features: M [G x H], the embeddings `model(..., return_features=True)` returns.  Eval mode only."""
        if self.training:
            raise RuntimeError("forward_group is the eval-mode pass: call model.eval() first")
        return amil_stack_infer_group(self.attention_net_WSI, self.classifier, bags, labels, censors, alpha,
                                      return_features)

    def integrated_gradients(self, path_features, n_steps=20, method="gausslegendre", return_full=False, window_steps=0):
        """Integrated-gradients patch attribution of risk = -sum(S) from a zero baseline in ONE C-ABI call
        (ops.amil_integrated_gradients) -- what the reference's create_attributions.py:94-102 gets from captum's
        IntegratedGradients(n_steps=20) through n_steps autograd passes.  method: `gausslegendre` (captum's default),
        `riemann_trapezoid` or `riemann_middle`; the nodes and weights are computed on the host in float64 and rounded once
        to fp32 (ops.ig_quadrature).  window_steps: nodes per grouped window, 0 lets the library choose.
        Returns PatchAttribution(patch_attr [N] = sum_l attr, patch_abs [N] = sum_l |attr| (the reference's reduction),
        total, total_abs, risk, risk_baseline, delta = total - (risk - risk_baseline) (captum's convergence delta),
        step_risk [n_steps], attr [N x L] when return_full else None).  Eval mode, fp32 bags, the stock head only."""
        from .. import ops
        rs, ra, _, _, *rest = amil_stack_ig(self, "path", self.attention_net_WSI, [path_features],
                                            ops.amil_integrated_gradients, (path_features,), n_steps, method, return_full,
                                            window_steps)
        return PatchAttribution(rs, ra, *rest)
