"""Stage-2 models on the exported 256-d embeddings, discrete-hazard (nll) heads: drop-in for
models/nll_models_pretrained.py:13-197 of the reference (same class names -- including the reference's spelling
`unimonal_pretrained` --, constructor signatures, submodule trees and therefore state_dict keys).
All arithmetic runs in the HIP kernels behind include/mmf_amil.h (dense, batchnorm, highway mix, Kronecker fusion,
hazards)."""
from __future__ import annotations

import collections

import torch
import torch.nn as nn

from .. import ops
from ..utils.utils_pretrained import initialize_weights
from .model_modules import Highway, XlinearFusion, fcnn_block


def _seed(training):
    return ops.next_dropout_seed() if training else 0


class unimonal_pretrained(nn.Module):
    """models/nll_models_pretrained.py:13-62."""

    def __init__(self, dropout=True, n_classes=4, mode=None, train_type=None, bag_loss=None, n_layers=1):
        super().__init__()
        self.n_classes = n_classes
        self.train_type = train_type
        self.bag_loss = bag_loss
        self.mode = mode
        if self.train_type == "fcnn":
            self.classifier = nn.Sequential(*[nn.Linear(256, n_classes), nn.Dropout(0.7)])
        elif self.train_type == "highway":
            self.highway = Highway(256, n_layers)
            self.classifier = nn.Linear(256, n_classes)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def forward(self, **kwargs):
        h = kwargs[{"path": "h_path", "radio": "h_radio", "omic": "h_omic"}[self.mode]]
        if self.train_type == "fcnn":
            lin, drop = self.classifier[0], self.classifier[1]
            p = drop.p if self.training else 0.0
            logits = ops.dense(h, lin.weight, lin.bias, drop_kind="dropout" if p > 0 else "none", drop_p=p,
                               seed=_seed(self.training), site=0)
        elif self.train_type == "highway":
            logits = ops.dense(self.highway(h), self.classifier.weight, self.classifier.bias)
        else:
            raise NotImplementedError(f"train_type {self.train_type!r}")     # 'residual' is commented out in the reference (:27-29)
        risk, hazards, S, _ = ops.hazards_from_logits(logits)
        return risk, hazards, S


def _pick(mode, h_radio, h_path, h_omic):
    """The modality order of the reference's cat / v_list (nll_models_pretrained.py:153-160, 164-171, 180-187):
    [radio, path] | [radio, omic] | [omic, path] | [radio, path, omic]."""
    r, p, o = "radio" in mode, "path" in mode, "omic" in mode
    if r and p and not o:
        return [h_radio, h_path]
    if r and o and not p:
        return [h_radio, h_omic]
    if o and p and not r:
        return [h_omic, h_path]
    if r and p and o:
        return [h_radio, h_path, h_omic]
    raise NotImplementedError(f"mode {mode!r}")


# what integrated_gradients returns: dicts by modality name ("radio", "path", "omic": the ones the mode keeps) of
# per-patient tensors [P]; attr: dict of [P x 256] or None; the risks [P]; step_risk [P x n_steps]; hazards, S [P x K] or None
Stage2Attribution = collections.namedtuple("Stage2Attribution", [
    "modality_attr", "modality_abs", "share", "attr", "risk", "risk_baseline", "delta", "step_risk", "hazards", "S"])


def _names(mode):
    """The present modalities in _pick's order."""
    return _pick(mode, "radio", "path", "omic")


def _bn_args(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def _highway_args(hw):
    pairs = lambda layers: [(l.weight, l.bias) for l in layers]
    return dict(bn1=_bn_args(hw.bn1), bn2=_bn_args(hw.bn2), gate=pairs(hw.gate), nonlinear=pairs(hw.nonlinear),
                linear=pairs(hw.linear))


def _fcnn_args(seq):
    d = dict(W0=seq[0].weight, b0=seq[0].bias, bn=_bn_args(seq[1]))
    if len(seq) > 4:
        d.update(W4=seq[4].weight, b4=seq[4].bias)
    return d


def stage2_ig_operands(model, family):
    """(blocks, Wk, bk, n_layers, xfusion weights or None) of a multimodal_pretrained for
    ops.stage2_integrated_gradients."""
    tt, names = model.train_type, _names(model.mode)
    late = {"radio": "MRI", "path": "WSI", "omic": "omic"}
    if tt == "early-fcnn":
        seq = model.classifier
        return [dict(W0=seq[0].weight, b0=seq[0].bias, bn=_bn_args(seq[1]))], seq[4].weight, seq[4].bias, 1, None
    if tt == "late-fcnn":
        cls = model.classifier[0]
        return [_fcnn_args(getattr(model, "layer_" + late[n])) for n in names], cls.weight, cls.bias, 1, None
    if tt == "early-highway":
        return [_highway_args(model.highway)], model.classifier.weight, model.classifier.bias, model.highway.num_layers, None
    if tt == "late-highway":
        hws = [getattr(model, "highway_" + n) for n in names]
        return [_highway_args(h) for h in hws], model.classifier.weight, model.classifier.bias, hws[0].num_layers, None
    if tt == "kronecker":
        xw = []
        for i in range(len(names)):
            for lin in (model.xfusion.reduce[i][0][0], model.xfusion.reduce[i][1][0], model.xfusion.reduce[i][2][0]):
                xw += [lin.weight, lin.bias]
        e1, e2 = model.xfusion.encoder1[0], model.xfusion.encoder2[0]
        return [], model.classifier.weight, model.classifier.bias, 1, xw + [e1.weight, e1.bias, e2.weight, e2.bias]
    raise NotImplementedError(f"integrated_gradients: train_type {tt!r}")


def stage2_integrated_gradients(model, family, h_radio, h_path, h_omic, n_steps, method, return_full):
    """integrated_gradients of both multimodal_pretrained classes: the refusals (train mode, non-fp32 or CPU-side shapes),
    the rule's nodes, the one fused call and the per-patient sums."""
    if model.training:
        raise RuntimeError("integrated_gradients is an eval-mode pass (dropout and batch statistics would make the "
                           "integrand depend on the cohort): call model.eval() first")
    names = _names(model.mode)
    given = dict(radio=h_radio, path=h_path, omic=h_omic)
    vs = [given[n] for n in names]
    if any(v is None for v in vs):
        raise ops._lib.MmfError(f"mode {model.mode!r} needs the embeddings {names}")
    if any(v.dtype != torch.float32 for v in vs):
        raise NotImplementedError("integrated_gradients takes fp32 embeddings")
    alphas, weights = ops.ig_quadrature(method, n_steps)
    blocks, Wk, bk, n_layers, xfusion = stage2_ig_operands(model, family)
    present = tuple(n in names for n in ("radio", "path", "omic"))
    with torch.no_grad():
        r = ops.stage2_integrated_gradients(family, model.train_type, present, vs, blocks, Wk, bk, alphas, weights,
                                            n_layers=n_layers, want_attr=return_full, xfusion=xfusion)
        m_attr = {n: r["mod_sum"][:, i] for i, n in enumerate(names)}
        m_abs = {n: r["mod_abs"][:, i] for i, n in enumerate(names)}
        tot_abs = r["mod_abs"].sum(1)
        share = {n: m_abs[n] / tot_abs for n in names}
        delta = r["mod_sum"].sum(1) - (r["risk"] - r["risk_base"])
    attr = dict(zip(names, r["attr"])) if return_full else None
    return Stage2Attribution(m_attr, m_abs, share, attr, r["risk"], r["risk_base"], delta, r["step_risk"], r["hazards"],
                             r["S"])


def late_branches(model, h_radio, h_path, h_omic, seed):
    """The late types' per-modality blocks (layer_MRI / layer_WSI / layer_omic, or the three Highways) on every embedding
    that is given, dropout sites 0, 1, 2: forward hands in all three, as the reference does (:144-151), even if the mode
    drops one; the captum_* methods leave that one out (None).  Shared by both families' multimodal_pretrained."""
    late = {"radio": "MRI", "path": "WSI", "omic": "omic"}
    out = []
    for site, (n, h) in enumerate((("radio", h_radio), ("path", h_path), ("omic", h_omic))):
        if h is None:
            out.append(None)
        elif model.train_type == "late-fcnn":
            out.append(fcnn_block(getattr(model, "layer_" + late[n]), h, seed or 0, site))
        else:
            out.append(getattr(model, "highway_" + n)(h, seed=None if seed is None else seed + site))
    return out


class multimodal_pretrained(nn.Module):
    """models/nll_models_pretrained.py:66-197."""

    def __init__(self, input_dim: int = 37, dropout=True, n_classes=4, mode="radio_path_omic", train_type=None,
                 bag_loss=None, n_layers=1):
        super().__init__()
        self.n_classes = n_classes
        self.mode = mode
        self.train_type = train_type
        self.bag_loss = bag_loss
        num_modalities = sum(k in mode for k in ("radio", "path", "omic"))
        if train_type == "early-fcnn":
            self.classifier = nn.Sequential(*[nn.Linear(num_modalities * 256, 128), nn.BatchNorm1d(128), nn.ReLU(),
                                              nn.Dropout(0.7), nn.Linear(128, n_classes)])
        elif train_type == "late-fcnn":
            self.layer_WSI = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7)])
            self.layer_MRI = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7)])
            self.layer_omic = nn.Sequential(*[nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Dropout(0.7)])
            self.classifier = nn.Sequential(*[nn.Linear(num_modalities * 128, n_classes)])
        elif train_type == "early-highway":
            self.highway = Highway(num_modalities * 256, n_layers)
            self.classifier = nn.Linear(num_modalities * 256, n_classes)
        elif train_type == "late-highway":
            self.highway_radio = Highway(256, n_layers)
            self.highway_path = Highway(256, n_layers)
            self.highway_omic = Highway(256, n_layers)
            self.classifier = nn.Linear(num_modalities * 256, n_classes)
        elif train_type == "kronecker":
            self.xfusion = XlinearFusion(num_modalities=num_modalities, dropout_rate=0.7)
            self.classifier = nn.Linear(256, n_classes)
        initialize_weights(self)

    def relocate(self):
        self.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))

    def _logits(self, h_radio, h_path, h_omic):
        seed = _seed(self.training) if self.training else None
        if "late" in self.train_type:
            r, p, o = late_branches(self, h_radio, h_path, h_omic, seed)
            mm = torch.cat(_pick(self.mode, r, p, o), dim=1)
            cls = self.classifier[0] if isinstance(self.classifier, nn.Sequential) else self.classifier
            return ops.dense(mm, cls.weight, cls.bias)
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
        logits = self._logits(h_radio, h_path, h_omic)
        risk, hazards, S, _ = ops.hazards_from_logits(logits)
        return risk, hazards, S

    # the methods captum is pointed at (models/nll_models_pretrained.py:200-320): the risk alone, as a function of the
    # embeddings the mode keeps, through the same autograd ops as forward
    def _risk(self, h_radio=None, h_path=None, h_omic=None):
        return ops.hazards_from_logits(self._logits(h_radio, h_path, h_omic))[0]

    def captum_radio_path(self, h_radio, h_path):
        return self._risk(h_radio=h_radio, h_path=h_path)

    def captum_path_omic(self, h_omic, h_path):
        return self._risk(h_path=h_path, h_omic=h_omic)

    def captum_radio_omic(self, h_radio, h_omic):
        return self._risk(h_radio=h_radio, h_omic=h_omic)

    def captum(self, h_radio, h_path, h_omic):
        return self._risk(h_radio, h_path, h_omic)

    def integrated_gradients(self, h_radio=None, h_path=None, h_omic=None, n_steps=20, method="gausslegendre",
                             return_full=False):
        """Integrated gradients of risk = -sum(S) with respect to the embeddings the mode keeps, from a zero baseline, for
        a cohort [P x 256] in ONE fused call (ops.stage2_integrated_gradients): create_attributions.py:93-164 for every
        patient at once.  Eval mode, fp32.  Returns a Stage2Attribution; modality_abs holds the columns of attr.csv,
        modality_attr those of attr_orig.csv."""
        return stage2_integrated_gradients(self, "nll", h_radio, h_path, h_omic, n_steps, method, return_full)
