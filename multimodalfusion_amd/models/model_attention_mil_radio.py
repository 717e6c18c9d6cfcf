"""Radiology attention-MIL head; drop-in for models/model_attention_mil_radio.py of the reference
(ctor signatures :14-15 / :67-68, forward(**kwargs) :73-115, state_dict keys)."""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

from .. import ops
from ..utils.utils import initialize_weights
from .model_modules import (AMIL_SIZES, amil_stack, amil_stack_head, amil_stack_ig, amil_stack_infer_group,
                            amil_stack_nll_step, amil_stack_nll_step_group, hand_over_grads, make_amil_stack, stack_args,
                            step_grad_buffers)


RadioAttribution = namedtuple("RadioAttribution", ["inst_attr", "inst_abs", "modality_attr", "modality_abs", "total",
                                                   "total_abs", "risk", "risk_baseline", "delta", "step_risk", "attr"])


class MIL_Attention_fc_radio(nn.Module):
    """Parameter container: `reduce_dim` (several modalities), `attention_net_radio`, `classifier`."""

    def __init__(self, radio_fusion="concat", gate_radio=True, dropout=True, model_size_radio: str = "small",
                 n_classes=4, modalities=["T1", "T2", "T1Gd", "FLAIR"]):
        super().__init__()
        self.radio_fusion, self.n_classes, self.modalities = radio_fusion, n_classes, modalities
        self.size_dict_radio = {name: list(dims) for name, dims in AMIL_SIZES.items()}
        feat, hidden, _ = AMIL_SIZES[model_size_radio]
        n_mod = len(modalities)
        if n_mod > 1:                           # created before the stack, as in the reference (:27-32): same RNG order
            if radio_fusion == "concat":
                self.reduce_dim = nn.Linear(feat * n_mod, feat)
            elif radio_fusion == "tensor":
                # unusable in the reference as well (its forward reads an attribute that is never set,
                # model_attention_mil_radio.py:84)
                raise NotImplementedError("radio_fusion='tensor' is unusable in the reference and not provided")
        self.attention_net_radio = make_amil_stack(model_size_radio, gated=gate_radio, att_dropout=dropout)
        self.classifier = nn.Linear(hidden, n_classes)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def forward(self, h, return_features=False, attention_only=False):
        pass            # abstract in the reference too (:64-65)


class MIL_Attention_fc_surv_radio(MIL_Attention_fc_radio):
    def __init__(self, radio_fusion="concat", gate_radio=True, dropout=True, model_size_radio="small", n_classes=4,
                 modalities=["T1", "T2", "T1Gd", "FLAIR"]):
        model_size_radio = "small"              # the reference overrides the argument (:70)
        super().__init__(radio_fusion=radio_fusion, gate_radio=gate_radio, dropout=dropout,
                         model_size_radio=model_size_radio, n_classes=n_classes, modalities=modalities)

    def nll_step(self, label, c, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None, **kwargs):
        """Extension of the reference surface (the training-loop mirror uses it, utils/core_utils.py): forward +
        NLLSurvLoss(alpha) + backward of one patient without an autograd graph -- what `model(**kwargs)`, the loss and
        `(loss * loss_scale).backward()` compute together (models/model_attention_mil_radio.py:73-115 +
        utils/loss_utils.py:22-39), same dropout draw: `reduce_dim` over the modality segments (mmf_linear_forward), the
        stack + classifier + loss + backward as ONE call that also returns d loss / d(reduce_dim output)
        (mmf_amil_nll_step), `reduce_dim`'s backward (mmf_linear_backward).  Gradients are ADDED to .grad (fresh buffers
        where it is None) -- or go to `grad_out`, tensors in self.parameters() order, overwritten unless `accumulate`.
        Returns (hazards, S, Y_hat, A_raw, loss, risk), detached."""
        if any(not p.requires_grad for p in self.parameters()):
            raise RuntimeError("nll_step needs every parameter of the head to require grad")
        bags = [kwargs[m] for m in self.modalities]
        many = len(bags) > 1
        rd_out = head_out = None                # grad_out: reduce_dim's two entries first, then the head's
        if grad_out is not None:
            grad_out = list(grad_out)
            rd_out, head_out = (grad_out[:2], grad_out[2:]) if many else (None, grad_out)
        with torch.no_grad():
            if many:
                W, b = self.reduce_dim.weight, self.reduce_dim.bias
                x, saved = ops._linear_cat_fwd_raw(bags, W, b)
                dx = torch.empty_like(x)
            else:
                x, dx = bags[0], None
            out = amil_stack_nll_step(self.attention_net_radio, self.classifier, x, self.training, label, c, alpha,
                                      loss_scale, head_out, accumulate, dx_out=dx)
            if many:
                dW, db, _ = ops._linear_cat_bwd_raw(dx, saved, b is not None, need_dx=False)
                hand_over_grads((W, b), {W: dW, b: db}, rd_out, accumulate)
        return out

    def nll_step_group(self, bags, labels, censors, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None, seeds=None):
        """nll_step for the G bags of one accumulation window in ONE C-ABI call (ops.radio_nll_step_group): reduce_dim and
        the stack's GEMMs run once over all of their rows.  bags: a list of G {modality: [n_g x 1024]} dicts, or a
        pre-stacked pair (x [n_mod x sum N x 1024] tensor, sizes) with the modalities in self.modalities order;
        labels / censors: G values.  Gradients of sum_g loss_g * loss_scale, same .grad / grad_out conventions as
        nll_step; in train mode bag g draws the dropout seed the g-th of G nll_step calls would (or `seeds[g]` when
        given).  One modality (no reduce_dim): the pathology head's grouped step on it.
        Returns (hazards [G x K], S [G x K], Y_hat [G x 1], [A_raw [1 x N_g]], loss [G], risk [G]), detached."""
        from .. import ops
        if any(not p.requires_grad for p in self.parameters()):
            raise RuntimeError("nll_step_group needs every parameter of the head to require grad")
        xs, sizes = self._stacked(bags)
        if len(xs) == 1:
            return amil_stack_nll_step_group(self.attention_net_radio, self.classifier, (xs[0], sizes), self.training,
                                             labels, censors, alpha, loss_scale, grad_out, accumulate, seeds)
        gated, stack, p_h, p_att = stack_args(self.attention_net_radio, self.training)
        Wr, br, Wk, bk = self.reduce_dim.weight, self.reduce_dim.bias, self.classifier.weight, self.classifier.bias
        grads, accumulate = step_grad_buffers([Wr, br, *stack, Wk, bk], xs[0].device, grad_out, accumulate)
        if seeds is None:
            seeds = [ops.next_dropout_seed() for _ in sizes] if self.training else None
        with torch.no_grad():
            return ops.radio_nll_step_group(xs, sizes, Wr, br, stack, Wk, bk, gated, labels, censors, alpha, grads,
                                            loss_scale=loss_scale, accumulate=accumulate, p_h=p_h, p_att=p_att,
                                            seeds=seeds)

    def _stacked(self, bags):
        """(per-modality [sum N x k] tensors, sizes) of a list of G {modality: [n_g x k]} dicts or of a pre-stacked
        (x [n_mod x sum N x k], sizes) pair."""
        nmod = len(self.modalities)
        if (isinstance(bags, (tuple, list)) and len(bags) == 2 and torch.is_tensor(bags[0])
                and isinstance(bags[1], (list, tuple)) and all(isinstance(n, int) for n in bags[1])):
            x, sizes = bags
            if x.dim() != 3 or x.shape[0] != nmod:
                raise ops._lib.MmfError(f"pre-stacked bags must be [{nmod} x sum N x k], got {tuple(x.shape)}")
            return list(x.unbind(0)), list(sizes)
        if not all(isinstance(b, dict) for b in bags):
            raise TypeError("bags: a list of {modality: [n x k]} dicts or an (x [n_mod x sum N x k], sizes) pair")
        for b in bags:
            if len({tuple(b[m].shape) for m in self.modalities}) != 1:
                raise ops._lib.MmfError("the modalities of a bag must have the same [n x k] shape")
        sizes = [int(b[self.modalities[0]].shape[0]) for b in bags]
        return [torch.cat([b[m] for b in bags], 0) if len(bags) > 1 else bags[0][m] for m in self.modalities], sizes

    def forward_group(self, bags, labels=None, censors=None, alpha=0.0, return_features=False):
        """The eval-mode forward of G patients in ONE C-ABI call (ops.radio_infer_group): reduce_dim and the stack's
        GEMMs once over all rows, pooling and the head per bag.  bags as nll_step_group; labels / censors: G values for
        each bag's NLLSurvLoss(alpha) value, or None.  One modality (no reduce_dim): the pathology head's grouped pass on
        it.  Each bag gets what `model(**bag)` gives it under no_grad, to fp32 rounding.  Returns (hazards [G x K],
        S [G x K], Y_hat [G x 1], [A_raw [1 x N_g]], loss [G] or None, risk [G]); return_features: M [G x H].
        Eval mode only."""
        if self.training:
            raise RuntimeError("forward_group is the eval-mode pass: call model.eval() first")
        xs, sizes = self._stacked(bags)
        if len(xs) == 1:
            return amil_stack_infer_group(self.attention_net_radio, self.classifier, (xs[0], sizes), labels, censors,
                                          alpha, return_features)
        gated, stack, _, _ = stack_args(self.attention_net_radio, False)
        Wr, br = self.reduce_dim.weight, self.reduce_dim.bias
        with torch.no_grad():
            if return_features:
                return ops.radio_infer_group(xs, sizes, Wr, br, stack, gated, want_M=True)[5]
            hz, S, Y_hat, risk, A, _, loss = ops.radio_infer_group(xs, sizes, Wr, br, stack, gated, self.classifier.weight,
                                                                   self.classifier.bias, labels, censors, alpha)
        return hz, S, Y_hat, A, loss, risk

    def integrated_gradients(self, n_steps=20, method="gausslegendre", return_full=False, window_steps=0, **bags):
        """Integrated-gradients attribution of risk = -sum(S) to every instance of every modality, from a zero baseline,
        in ONE C-ABI call (ops.radio_integrated_gradients) -- what the reference's create_attributions.py:94-147 gets from
        captum through n_steps autograd passes of models/model_attention_mil_radio.py:73-115.  bags: {modality: [N x k]}
        fp32 tensors of one shape; method, window_steps as MIL_Attention_fc_surv_path.integrated_gradients.
        Returns RadioAttribution(inst_attr [n_mod x N] = sum_l attr, inst_abs [n_mod x N] = sum_l |attr|, modality_attr /
        modality_abs [n_mod]: their sums over the instances (the reference's radio_attr per sequence), total, total_abs,
        risk, risk_baseline, delta = total - (risk - risk_baseline), step_risk [n_steps], attr [n_mod x N x k] when
        return_full else None), the modalities in self.modalities order.  One modality (no reduce_dim): the pathology
        call on that bag, n_mod = 1.  Eval mode, fp32 bags, the stock head only."""
        xs = [bags[m] for m in self.modalities]
        if len(xs) > 1:
            call, lead = ops.radio_integrated_gradients, (xs, self.reduce_dim.weight, self.reduce_dim.bias)
        else:
            def call(*args, **kw):
                rs, ra, attr, *risks = ops.amil_integrated_gradients(*args, **kw)
                return (rs[None], ra[None], None if attr is None else attr[None], *risks)
            lead = (xs[0],)
        return RadioAttribution(*amil_stack_ig(self, "radio", self.attention_net_radio, xs, call, lead, n_steps, method,
                                               return_full, window_steps))

    def forward(self, **kwargs):
        bags = [kwargs[m] for m in self.modalities]
        # several modalities: cat(axis=1) + reduce_dim without materialising the concatenation (:80-82)
        x = ops.linear_cat(bags, self.reduce_dim.weight, self.reduce_dim.bias) if len(bags) > 1 else bags[0]
        flags = [kwargs.get(k) for k in ("attention_only", "return_features", "return_attention")]
        if any(flags):
            M, A_raw = amil_stack(self.attention_net_radio, x, self.training)
            return M if (flags[1] and not flags[0]) else A_raw      # attention_only wins, then features (:91-113)
        return amil_stack_head(self.attention_net_radio, self.classifier, x, self.training)
