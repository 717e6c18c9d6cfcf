"""Stage-2 models with a scalar risk head (Cox / ranking losses): drop-in for
models/coxranking_models_pretrained.py:14-200 of the reference (same class names, constructor signatures, submodule
trees / state_dict keys).  forward returns (risk, None, None) as the reference does."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..utils.utils_pretrained import initialize_weights
from .model_modules import Highway, Residual, XlinearFusion, fcnn_block
from .nll_models_pretrained import _pick, _seed, late_branches, stage2_integrated_gradients, stage2_step, stage2_step_ok


class unimonal_pretrained(nn.Module):
    """models/coxranking_models_pretrained.py:14-58."""

    def __init__(self, dropout=True, n_classes=4, mode="radio", train_type=None, bag_loss=None, n_layers=1):
        super().__init__()
        self.n_classes = n_classes
        self.train_type = train_type
        self.bag_loss = bag_loss
        self.mode = mode
        self.n_layers = n_layers
        if self.train_type == "fcnn":
            self.classifier = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7),
                                              nn.Linear(128, 1)])
        elif self.train_type == "highway":
            self.highway = Highway(256, n_layers)
            self.classifier = nn.Linear(256, 1)
        elif self.train_type == "residual":
            self.residual = Residual(256, n_layers)
            self.classifier = nn.Linear(256, 1)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def forward(self, **kwargs):
        h = kwargs[{"path": "h_path", "radio": "h_radio", "omic": "h_omic"}[self.mode]]
        if self.train_type == "fcnn":
            risk = fcnn_block(self.classifier, h, _seed(self.training), 0)
        elif self.train_type == "highway":
            risk = ops.dense(self.highway(h), self.classifier.weight, self.classifier.bias)
        elif self.train_type == "residual":
            risk = ops.dense(self.residual(h), self.classifier.weight, self.classifier.bias)
        else:
            raise NotImplementedError(f"train_type {self.train_type!r}")
        return risk.squeeze(), None, None


class multimodal_pretrained(nn.Module):
    """models/coxranking_models_pretrained.py:62-200."""

    def __init__(self, dropout=True, n_classes=4, mode="radio_path_omic", train_type=None, bag_loss=None, n_layers=1):
        super().__init__()
        self.n_classes = n_classes
        self.mode = mode
        self.train_type = train_type
        self.bag_loss = bag_loss
        self.n_layers = n_layers
        num_modalities = sum(k in mode for k in ("radio", "path", "omic"))
        blk = lambda: nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7), nn.Linear(128, 1)])
        if train_type == "late-fcnn":
            self.layer_WSI = blk()
            self.layer_MRI = blk()
            self.layer_omic = blk()
            self.classifier = nn.Sequential(*[nn.Linear(num_modalities, 1)])
        elif train_type == "early-fcnn":
            self.classifier = nn.Sequential(*[nn.Linear(num_modalities * 256, 128), nn.BatchNorm1d(128), nn.ReLU(),
                                              nn.Dropout(0.7), nn.Linear(128, 1)])
        elif train_type == "early-highway":
            self.highway = Highway(num_modalities * 256, n_layers)
            self.classifier = nn.Linear(num_modalities * 256, 1)
        elif train_type == "late-highway":
            self.highway_radio = Highway(256, n_layers)
            self.highway_path = Highway(256, n_layers)
            self.highway_omic = Highway(256, n_layers)
            self.classifier = nn.Linear(num_modalities * 256, 1)
        elif train_type == "kronecker":
            self.xfusion = XlinearFusion(num_modalities=num_modalities, dropout_rate=0.7)
            self.classifier = nn.Linear(256, 1)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def _risk(self, h_radio=None, h_path=None, h_omic=None):
        """The scalar output for the embeddings that are given: forward hands in all three (a late type evaluates the one
        the mode drops too, as the reference does), the captum_* methods leave that one out (None)."""
        seed = _seed(self.training) if self.training else None
        if "late" in self.train_type:
            out = late_branches(self, h_radio, h_path, h_omic, seed)
            mm = torch.cat(_pick(self.mode, *out), dim=1)
            cls = self.classifier[0] if isinstance(self.classifier, nn.Sequential) else self.classifier
            return ops.dense(mm, cls.weight, cls.bias).squeeze()
        if "early" in self.train_type:
            mm = torch.cat(_pick(self.mode, h_radio, h_path, h_omic), dim=1)
            if self.train_type == "early-fcnn":
                return fcnn_block(self.classifier, mm, seed or 0, 0)
            return ops.dense(self.highway(mm, seed=seed), self.classifier.weight, self.classifier.bias)
        if self.train_type == "kronecker":
            mm = self.xfusion(v_list=_pick(self.mode, h_radio, h_path, h_omic), seed=seed)
            return ops.dense(mm, self.classifier.weight, self.classifier.bias)
        raise NotImplementedError(f"train_type {self.train_type!r}")

    def forward(self, h_radio, h_path, h_omic):
        return self._risk(h_radio, h_path, h_omic), None, None

    def step_ok(self, h_radio, h_path, h_omic, loss_fn):
        """True when step can take this batch (nll_models_pretrained.multimodal_pretrained.step_ok; the scalar head takes
        CoxSurvLoss and RankingSurvLoss)."""
        return stage2_step_ok(self, "cox", h_radio, h_path, h_omic, loss_fn)

    def step(self, h_radio, h_path, h_omic, loss_fn, label=None, event_time=None, c=None, loss_scale=1.0, grad_out=None,
             accumulate=None, backward=True):
        """forward, the loss and `(loss * loss_scale).backward()` as ONE C-ABI call (ops.stage2_step); see
        nll_models_pretrained.multimodal_pretrained.step.  Returns (risk [B], None, None, loss), detached."""
        return stage2_step(self, "cox", h_radio, h_path, h_omic, loss_fn, label, event_time, c, loss_scale, grad_out,
                           accumulate, backward)

    # the methods captum is pointed at (models/coxranking_models_pretrained.py:202-305): the risk alone, as a function of
    # the embeddings the mode keeps, through the same autograd ops as forward
    def captum_radio_path(self, h_radio, h_path):
        return self._risk(h_radio, h_path, None)

    def captum_path_omic(self, h_omic, h_path):
        return self._risk(None, h_path, h_omic)

    def captum_radio_omic(self, h_radio, h_omic):
        return self._risk(h_radio, None, h_omic)

    def captum(self, h_radio, h_path, h_omic):
        return self._risk(h_radio, h_path, h_omic)

    def integrated_gradients(self, h_radio=None, h_path=None, h_omic=None, n_steps=20, method="gausslegendre",
                             return_full=False):
        """Integrated gradients of the scalar risk with respect to the embeddings the mode keeps, from a zero baseline, for
        a cohort [P x 256] in ONE fused call (ops.stage2_integrated_gradients).  Eval mode, fp32.  Returns a
        Stage2Attribution (nll_models_pretrained.py) without hazards and S."""
        return stage2_integrated_gradients(self, "cox", h_radio, h_path, h_omic, n_steps, method, return_full)
