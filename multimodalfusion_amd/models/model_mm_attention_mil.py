"""Multimodal (radiology + pathology + omic) attention-MIL with concat / tensor fusion; drop-in for
models/model_mm_attention_mil.py of the reference (ctor signatures :19-23 / :118-121, forward :128-200,
state_dict keys of Appendix B).

The reference class cannot be constructed or run as shipped.  What this module does
about each defect -- the signature and the mathematics are kept, nothing else is changed:
  * `gate_omic=` is accepted by the subclass and not forwarded (the reference forwards it to a base ctor
    without that parameter -> TypeError, :124);
  * the fused width uses size_WSI (the reference names an undefined `size_path`, :83);
  * `genomic_features` may be [G] (what the forward expects, :165) or [1 x G] (what the collate delivers);
  * radio_fusion='tensor' raises NotImplementedError (the reference calls an attribute that is never
    defined, :141);
  * return_features=True returns the fused embedding (the reference raises NameError, :196-198).
"""
from __future__ import annotations

import collections
import contextlib

import torch
import torch.nn as nn

from .. import ops
from ..utils.utils import initialize_weights
from .model_modules import (Attn_Net, Attn_Net_Gated, SNN_Block, XlinearFusion, amil_stack, hand_over_grads, ig_refusals,
                            snn_stack, stack_args)


ModalityAttribution = collections.namedtuple("ModalityAttribution", [
    "modality_attr", "modality_abs", "share", "patch_attr", "patch_abs", "inst_attr", "inst_abs", "sequence_abs", "gene_attr",
    "total", "total_abs", "risk", "risk_baseline", "delta", "step_risk", "hazards", "S", "Y_hat", "attr"])


class MM_MIL_Attention_fc(nn.Module):
    def __init__(self, input_dim: int = 80, radio_fusion="concat", fusion="tensor", gate=True, gate_path=True,
                 gate_radio=True, dropout=True, model_size_radio: str = "small", model_size_wsi: str = "small",
                 model_size_omic: str = "small", n_classes=4, modalities=["T1", "T2", "T1Gd", "FLAIR"],
                 mode="radio_path_omic"):
        super().__init__()
        self.radio_fusion = radio_fusion
        self.fusion = fusion
        self.n_classes = n_classes
        self.size_dict_radio = {"small": [1024, 256, 256], "big": [1024, 256, 384]}
        self.size_dict_WSI = {"small": [1024, 256, 256], "big": [1024, 256, 384]}
        self.size_dict_omic = {"small": [256, 256], "big": [1024, 256]}
        self.modalities = modalities
        self.mode = mode

        size_omic = self.size_dict_omic[model_size_omic]
        fc_omic = [SNN_Block(dim1=input_dim, dim2=size_omic[0])]
        for i, _ in enumerate(size_omic[1:]):
            fc_omic.append(SNN_Block(dim1=size_omic[i], dim2=size_omic[i + 1], dropout=0.25))
        self.fc_omic = nn.Sequential(*fc_omic)

        size_radio = self.size_dict_radio[model_size_radio]
        fc_radio = [nn.Linear(size_radio[0], size_radio[1]), nn.ReLU(), nn.Dropout(0.25)]
        if gate_radio:
            att = Attn_Net_Gated(L=size_radio[1], D=size_radio[2], dropout=dropout, n_classes=1)
        else:
            att = Attn_Net(L=size_radio[1], D=size_radio[2], dropout=dropout, n_classes=1)
        fc_radio.append(att)
        self.attention_net_radio = nn.Sequential(*fc_radio)

        if self.radio_fusion == "tensor":
            raise NotImplementedError("radio_fusion='tensor' is unusable in the reference and not provided")
        elif self.radio_fusion == "concat":
            self.reduce_dim = nn.Linear(size_radio[0] * len(self.modalities), size_radio[0])

        size_WSI = self.size_dict_WSI[model_size_wsi]
        fc_WSI = [nn.Linear(size_WSI[0], size_WSI[1]), nn.ReLU(), nn.Dropout(0.25)]
        if gate_path:
            att = Attn_Net_Gated(L=size_WSI[1], D=size_WSI[2], dropout=dropout, n_classes=1)
        else:
            att = Attn_Net(L=size_WSI[1], D=size_WSI[2], dropout=dropout, n_classes=1)
        fc_WSI.append(att)
        self.attention_net_WSI = nn.Sequential(*fc_WSI)

        classifier_size = 0
        n_modalities = 0
        if "radio" in mode:
            classifier_size += size_radio[1]
            n_modalities += 1
        if "path" in mode:
            classifier_size += size_WSI[1]
            n_modalities += 1
        if "omic" in mode:
            classifier_size += size_omic[1]
            n_modalities += 1

        if self.fusion == "tensor":
            self.mm = XlinearFusion(dim=256, scale_dim=16, mmhid1=512, mmhid2=512, num_modalities=n_modalities,
                                    gate=gate, skip=1)
            self.classifier = nn.Sequential(*[nn.Linear(512, 256), nn.ReLU(), nn.Dropout(0.25),
                                              nn.Linear(256, n_classes)])
        elif self.fusion == "concat":
            self.classifier = nn.Linear(classifier_size, n_classes)
        initialize_weights(self)

    def relocate(self):
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.fc_omic = self.fc_omic.to(device)
        self.attention_net_radio = self.attention_net_radio.to(device)
        self.attention_net_WSI = self.attention_net_WSI.to(device)
        self.classifier = self.classifier.to(device)
        if self.fusion == "tensor":
            self.mm = self.mm.to(device)
        if self.radio_fusion == "concat":
            self.reduce_dim = self.reduce_dim.to(device)

    def forward(self, h, return_features=False, attention_only=False):
        pass


class MM_MIL_Attention_fc_surv(MM_MIL_Attention_fc):
    def __init__(self, input_dim: int = 80, radio_fusion: str = "concat", fusion: str = "tensor", gate=True,
                 gate_path=True, gate_omic=True, gate_radio=True, model_size_radio="small",
                 model_size_wsi: str = "small", model_size_omic="small", dropout=False, n_classes=4,
                 mode="radio_path_omic"):
        super().__init__(input_dim=input_dim, radio_fusion=radio_fusion, fusion=fusion, gate=gate,
                         gate_path=gate_path, gate_radio=gate_radio, model_size_radio="small",
                         model_size_wsi=model_size_wsi, model_size_omic=model_size_omic, dropout=dropout,
                         n_classes=n_classes, mode=mode)

    def _side_stream(self, device):
        """A second HIP stream for the small branches (radio stack, omic SNN): they are independent of the pathology
        stack until the fusion, and its big kernels leave CUs idle (224 of 256 at 50k instances), so the small
        kernels run beside them instead of after them.  Autograd replays each branch on the stream it ran on.
        One per main stream, chosen by measurement (streams.stream_beside): a pool stream that shares the main stream's
        hardware queue would run the branches after the stack, not beside it."""
        from ..streams import stream_beside
        cur = torch.cuda.current_stream(device)
        pool = self.__dict__.setdefault("_mmf_side", {})        # not a parameter / buffer: stays out of state_dict
        st = pool.get(cur.cuda_stream)
        if st is None or st.device != device:
            st = pool[cur.cuda_stream] = stream_beside([cur], device)
        return st

    def _fork(self, path_x, min_units=120_000):
        """The side-stream fork of forward() and nll_step: (cur, side, branch) -- the current stream, the side stream
        (ordered after the work cur has queued) and a context manager that issues on it -- or (None, None, a null context)
        when the branches stay on the current stream."""
        # worth it only while the step is GPU-bound, i.e. the pathology stack runs for longer than the host needs to
        # issue the step (~0.9 ms): >= 30k fp32 instances / >= 120k bf16 instances (measured: 50k fp32 1.30 -> 1.07 ms;
        # 100k bf16 is host-bound and the extra stream calls cost 0.05 ms)
        if not (getattr(self, "mmf_side_stream", True)          # set False on an instance to keep everything on one stream
                and path_x is not None and path_x.is_cuda and ("radio" in self.mode or "omic" in self.mode)
                and path_x.shape[0] * (1 if path_x.dtype == torch.bfloat16 else 4) >= min_units):
            return None, None, contextlib.nullcontext
        cur = torch.cuda.current_stream(path_x.device)
        side = self._side_stream(path_x.device)
        side.wait_stream(cur)
        return cur, side, lambda: torch.cuda.stream(side)

    def _concat_order(self):
        has = lambda k: k in self.mode
        if has("radio") and has("path") and not has("omic"):
            return ["radio", "path"]
        if has("radio") and has("omic") and not has("path"):
            return ["radio", "omic"]
        if has("omic") and has("path") and not has("radio"):
            return ["omic", "path"]
        return ["radio", "path", "omic"]

    def _concat_layout(self):
        """(order, {branch: slice of the fused vector}, width of the fused vector): the embeddings side by side in
        _concat_order()."""
        order = self._concat_order()
        width = {"radio": self.attention_net_radio[0].out_features, "path": self.attention_net_WSI[0].out_features,
                 "omic": self.fc_omic[-1][0].out_features}
        cols, F = {}, 0
        for k in order:
            cols[k] = slice(F, F + width[k])
            F += width[k]
        return order, cols, F

    def xfusion_step_ok(self):
        """The XlinearFusion configuration nll_step and forward_group take: skip, the scaled embeddings within 384 columns."""
        return bool(self.mm.skip) and len(self._concat_order()) * self.mm.reduce[0][0][0].weight.shape[0] <= 384

    def xfusion_group_ok(self):
        """The XlinearFusion configuration nll_step_group_tensor takes: skip, scale width 16."""
        return bool(self.mm.skip) and self.mm.reduce[0][0][0].weight.shape[0] == 16

    def _window_checks(self, path, radio, omic, labels, censors, forward_only=False):
        """Every refusal of a window (_stacked_patients' branches) before the first launch -> (G, labels [G], censors [G]);
        forward_only: forward_group's window -- a stricter omic check, labels optional."""
        MmfError = ops._lib.MmfError
        counts = {}
        if path is not None:
            counts["path"] = len(path[1])
        if radio is not None:
            counts["radio"] = len(radio[1])
        if omic is not None:
            G_in = self.fc_omic[0][0].in_features
            if forward_only and (omic.dim() != 2 or omic.dtype != torch.float32 or omic.shape[1] != G_in):
                raise MmfError(f"omic features must be fp32 [G x {G_in}], got {omic.dtype} {tuple(omic.shape)}")
            if omic.dim() != 2:
                raise MmfError(f"omic features must be [G x input_dim], got {tuple(omic.shape)}")
            counts["omic"] = int(omic.shape[0])
        if len(set(counts.values())) != 1:
            raise MmfError(f"the branches hold different numbers of patients: {counts}")
        G = next(iter(counts.values()))
        if G < 1 or G > ops.GROUP_MAX:
            raise MmfError(f"a group holds 1 .. {ops.GROUP_MAX} patients, got {G}")
        for k, br in (("path", path), ("radio", radio)):
            if br is None:
                continue
            xs = br[0] if k == "radio" else [br[0]]
            if any(x.dtype != torch.float32 for x in xs):
                raise MmfError("the grouped pass takes fp32 bags only (bf16 bags: one forward per patient)" if forward_only
                               else "the grouped step takes fp32 bags only (bf16 bags: one nll_step per patient)")
            if min(br[1]) < 1:
                raise MmfError("empty bag in the group")
            if any(x.dim() != 2 or x.shape[0] != sum(br[1]) for x in xs):
                raise MmfError(f"the {k} bags hold {[tuple(x.shape) for x in xs]} rows, their sizes add up to {sum(br[1])}")
        if forward_only and labels is None:
            return G, None, None
        Y = torch.as_tensor(labels).reshape(-1)
        cc = torch.as_tensor(censors).reshape(-1)
        if Y.numel() != G or cc.numel() != G:
            raise MmfError(f"{G} patients need {G} labels and censorships, got {Y.numel()} / {cc.numel()}")
        return G, Y, cc

    def nll_step(self, label, c, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None, **kwargs):
        """Extension of the reference surface (the training-loop mirror uses it, utils/core_utils.py): the whole training
        step of one patient (fusion='concat'; fusion='tensor' in the heads' configuration) -- what `hazards, S, Y_hat, A_raw = model(**kwargs)`,
        `loss = NLLSurvLoss(alpha)(hazards=hazards, S=S, Y=label, c=c)`, `(loss * loss_scale).backward()` compute together
        (models/model_mm_attention_mil.py:128-200 + utils/loss_utils.py:22-39 + autograd), with the same dropout draws --
        as a fixed sequence of C-ABI calls with no autograd graph: the branches' forward calls (radio and omic on the side
        stream beside the pathology stack), ONE launch for classifier + hazards + loss + their backward
        (mmf_surv_head_nll_step; the branches write their embeddings side by side, so the concatenation is never a
        launch; with the tensor fusion the XlinearFusion block and classifier[0] run in front of it), the branches'
        backward calls.  Gradients are ADDED to the parameters' .grad (a parameter whose .grad is
        None receives the fresh buffer, as autograd does) -- or to `grad_out`, tensors in self.parameters() order,
        overwritten unless `accumulate`.  Returns (hazards, S, Y_hat, A_raw dict, loss, risk), detached."""
        from ..ops import (_dense_bwd_raw, _dense_fwd_raw, _linear_cat_bwd_raw, _linear_cat_fwd_raw, _stack_bwd_raw,
                           _stack_fwd_raw, _xfusion_bwd_raw, _xfusion_fwd_raw)
        order, cols, F = self._concat_layout()
        if self.fusion == "tensor" and not self.xfusion_step_ok():
            raise NotImplementedError("nll_step covers the XlinearFusion configuration the heads use (skip, one patient)")
        params = list(self.parameters())
        if any(not p.requires_grad for p in params):
            raise RuntimeError("nll_step needs every parameter to require grad")
        tr = self.training
        path_x = kwargs.get("path_features") if "path" in order else None
        dev = (path_x if path_x is not None else kwargs[self.modalities[0]] if "radio" in order
               else kwargs["genomic_features"]).device
        grads = {}                                   # parameter -> gradient tensor of this step

        def stack_forward(seq, x, k):
            """The stack of branch k, its M written into k's slot of feat.  Returns (A_raw, what stack_backward takes)."""
            gated, ps, p_h, p_att = stack_args(seq, tr)
            seed = ops.next_dropout_seed() if tr else 0
            saved, _, state = _stack_fwd_raw(x, ps, gated, p_h, p_att, seed, M_out=feat[:, cols[k]])
            return saved[-1], (ps, saved, state)

        def stack_backward(run, g, need_dx=False):
            ps, saved, state = run
            dx, ds = _stack_bwd_raw(saved, state, g, None, need_dx)
            grads.update((p, gr) for p, gr in zip(ps, ds) if p is not None)
            return dx

        with torch.no_grad():
            feat = torch.empty((1, F), dtype=torch.float32, device=dev)
            # the side stream costs this step ~0.12 ms of host time (stream switches, four cross-stream waits) and pays from
            # 20k fp32 rows on (20k 0.60 -> 0.54 ms, 50k 1.02 -> 0.89; 10k 0.43 -> 0.45; bf16 100k 0.59 -> 0.56)
            cur, side, branch = self._fork(path_x, getattr(self, "mmf_fork_min_one_call", 80_000))
            fork = side is not None
            A_raw = {}
            # ---- forward: python order (and with it the dropout-seed order) radio, path, omic as in forward()
            if "radio" in order:
                with branch():
                    xs = [kwargs[m] for m in self.modalities]
                    cat = None
                    if len(xs) > 1:
                        h_radio, cat = _linear_cat_fwd_raw(xs, self.reduce_dim.weight, self.reduce_dim.bias)
                    else:
                        h_radio = xs[0]
                    A_raw["radiology"], run_r = stack_forward(self.attention_net_radio, h_radio, "radio")
            if "path" in order:
                prev = ops.set_concurrent(True) if fork else None      # see forward(): 224-CU tile plan beside the branches
                try:
                    A_raw["pathology"], run_p = stack_forward(self.attention_net_WSI, path_x, "path")
                finally:
                    if fork:
                        ops.set_concurrent(prev)
            if "omic" in order:
                with branch():
                    X = kwargs["genomic_features"]
                    if X.dim() == 1:
                        X = X.unsqueeze(0)
                    seed = ops.next_dropout_seed() if tr else 0
                    word = ops._seed_word
                    acts = [ops._f32c(X)]
                    nblk = len(self.fc_omic)
                    for i, blk in enumerate(self.fc_omic):
                        lin, adrop = blk[0], blk[2]
                        acts.append(_dense_fwd_raw(acts[-1], lin.weight, lin.bias, "selu", "alpha" if tr else "none",
                                                   adrop.p if tr else 0.0, seed, i, word,
                                                   out=feat[:, cols["omic"]] if i == nblk - 1 else None))
            if fork:
                cur.wait_stream(side)
            if self.fusion == "concat":
                # ---- classifier + hazards + loss + their backward: one launch on the branches' slots
                Wk, bk = self.classifier.weight, self.classifier.bias
                dWk, dbk = torch.empty_like(Wk), torch.empty_like(bk)
                hazards, S, Y_hat, loss, risk, dfeat = ops.surv_head_nll_step(feat, Wk, bk, label, c, alpha, dWk, dbk,
                                                                              loss_scale=loss_scale)
                grads[Wk], grads[bk] = dWk, dbk
                dslot = lambda k: dfeat[:, cols[k]]
            else:
                # ---- XlinearFusion (XFusionFn's forward / backward), classifier[0] + ReLU + Dropout, then classifier[3] +
                # hazards + loss + their backward in one launch (forward() lines 182-188)
                seed_f = ops.next_dropout_seed() if tr else 0
                word_f = ops._seed_word
                weights = self._xfusion_weights(len(order))
                p_f = self.mm.dropout_rate if tr else 0.0
                MMv, saved_x, state_x = _xfusion_fwd_raw([feat[:, cols[k]] for k in order], weights, p_f, seed_f)
                c0, c3 = self.classifier[0], self.classifier[3]
                p_c = self.classifier[2].p if tr else 0.0
                kind_c = "dropout" if tr else "none"
                hid = _dense_fwd_raw(MMv, c0.weight, c0.bias, "relu", kind_c, p_c, seed_f, 11, word_f)
                dWk, dbk = torch.empty_like(c3.weight), torch.empty_like(c3.bias)
                hazards, S, Y_hat, loss, risk, dhid = ops.surv_head_nll_step(hid, c3.weight, c3.bias, label, c, alpha,
                                                                             dWk, dbk, loss_scale=loss_scale)
                grads[c3.weight], grads[c3.bias] = dWk, dbk
                dMM, grads[c0.weight], grads[c0.bias] = _dense_bwd_raw(dhid, hid, MMv, c0.weight, True, "relu", kind_c, p_c,
                                                                       seed_f, 11, word=word_f)
                dv, dw = _xfusion_bwd_raw(dMM, saved_x, state_x)
                dvs = dict(zip(order, dv))
                grads.update(zip(weights, dw))
                dslot = lambda k: dvs[k]
            if fork:
                side.wait_stream(cur)
            # ---- backward: the pathology stack on this stream, the small branches beside it
            if "path" in order:
                stack_backward(run_p, dslot("path"))
            if "omic" in order:
                with branch():
                    g = dslot("omic")
                    for i in range(nblk - 1, -1, -1):
                        lin, adrop = self.fc_omic[i][0], self.fc_omic[i][2]
                        g, dW, db = _dense_bwd_raw(g, acts[i + 1], acts[i], lin.weight, lin.bias is not None, "selu",
                                                   "alpha" if tr else "none", adrop.p if tr else 0.0, seed, i,
                                                   need_dx=i > 0, word=word)
                        grads[lin.weight] = dW
                        if lin.bias is not None:
                            grads[lin.bias] = db
            if "radio" in order:
                with branch():
                    dh = stack_backward(run_r, dslot("radio"), need_dx=cat is not None)
                    if cat is not None:
                        W, b = self.reduce_dim.weight, self.reduce_dim.bias
                        grads[W], grads[b], _ = _linear_cat_bwd_raw(dh, cat, b is not None, need_dx=False)
            if fork:
                cur.wait_stream(side)
            # ---- hand the gradients over (parameters of branches outside `mode` took no part: no gradient, as in autograd)
            hand_over_grads(params, grads, grad_out, accumulate)
        return hazards, S, Y_hat, A_raw, loss, risk

    def _stacked_patients(self, patients):
        """The window's inputs per branch: (path (x_cat [sum N x L], sizes) or None, radio ([modality tensors, each
        [sum n x L]], sizes) or None, omic [G x input_dim] or None), from a list of per-patient kwarg dicts as nll_step
        takes them or from the pre-stacked triple (path (x, sizes), radio ([n_mod x rows x L], sizes), omic [G x
        input_dim]) with None for a branch outside `mode`.  Branches outside `mode` are dropped."""
        MmfError = ops._lib.MmfError
        has = lambda k: k in self.mode
        if isinstance(patients, tuple) and len(patients) == 3 and not any(isinstance(p, dict) for p in patients):
            path, radio, omic = patients
            for k, v in (("path", path), ("radio", radio), ("omic", omic)):
                if has(k) and v is None:
                    raise MmfError(f"mode {self.mode!r} needs the {k} branch of the pre-stacked window")
            if has("radio"):
                x, sizes = radio
                if x.dim() != 3 or x.shape[0] != len(self.modalities):
                    raise MmfError(f"pre-stacked radio bags must be [{len(self.modalities)} x rows x L], got {tuple(x.shape)}")
                radio = (list(x.unbind(0)), [int(n) for n in sizes])
            if has("path"):
                path = (path[0], [int(n) for n in path[1]])
            return (path if has("path") else None, radio if has("radio") else None, omic if has("omic") else None)
        if not isinstance(patients, (list, tuple)) or not all(isinstance(p, dict) for p in patients):
            raise TypeError("patients: a list of per-patient kwarg dicts or a pre-stacked (path, radio, omic) triple")
        if not patients:
            raise MmfError(f"a group holds 1 .. {ops.GROUP_MAX} patients, got 0")
        cat = lambda ts: torch.cat(ts, 0) if len(ts) > 1 else ts[0]
        path = radio = omic = None
        if has("path"):
            bags = [p["path_features"] for p in patients]
            path = (cat(bags), [int(b.shape[0]) for b in bags])
        if has("radio"):
            for p in patients:
                if len({tuple(p[m].shape) for m in self.modalities}) != 1:
                    raise MmfError("the modalities of a patient must have the same [n x L] shape")
            radio = ([cat([p[m] for p in patients]) for m in self.modalities],
                     [int(p[self.modalities[0]].shape[0]) for p in patients])
        if has("omic"):
            omic = cat([p["genomic_features"].reshape(1, -1) for p in patients])
        return path, radio, omic

    def nll_step_group(self, patients, labels, censors, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None,
                       seeds=None):
        """nll_step for the G <= 64 patients of one accumulation window (fusion='concat', fp32 bags, exact-fp32 GEMMs):
        within a window the weights are fixed (utils/core_utils.py:242-247 of the reference), so the patients are
        independent forward passes and their summed gradient is one contraction over all rows.  Each stack runs once
        over its branch's concatenated rows (ops._group_half_fwd_raw / _group_half_bwd_raw), the omic SNN as one B = G
        batch whose row g draws patient g's masks (ops._dense_rows_*), and the classifier, hazards, loss and their
        backward as one launch over the [G x F] feature matrix the branches write side by side
        (ops.surv_head_nll_step_group).  Everything is issued on the current stream, in this order: radio forward,
        pathology forward, omic forward, head, pathology backward, omic backward, radio backward, hand_over_grads -- no
        side stream: the grouped chains fill the GPU themselves.

        patients: a list of per-patient kwarg dicts as nll_step takes them, or the pre-stacked triple (path (x [sum N x
        L], sizes), radio ([n_mod x rows x L], sizes), omic [G x input_dim]) with None for a branch outside `mode`;
        pathology and radio sizes are independent and ragged.  labels / censors: G values.
        Seeds: in train mode patient g draws ops.next_dropout_seed() in nll_step's order -- radio, path, omic for patient
        0, then patient 1, ... -- so the same seed stream gives every patient the masks G nll_step calls give it; or
        `seeds` = {"radio": [G], "path": [G], "omic": [G]} (the branches in `mode`).
        Gradients of sum_g loss_g * loss_scale, same .grad / grad_out conventions as nll_step.
        Returns (hazards [G x K], S [G x K], Y_hat [G], A_raw {"radiology": [per patient], "pathology": [per patient]},
        loss [G], risk [G]), detached."""
        if self.fusion != "concat":
            raise NotImplementedError("nll_step_group covers fusion='concat'; XlinearFusion's kernels take one patient")
        return self._group_step("nll_step_group", patients, labels, censors, alpha, loss_scale, grad_out, accumulate, seeds)

    def nll_step_group_tensor(self, patients, labels, censors, alpha=0.0, loss_scale=1.0, grad_out=None, accumulate=None,
                              seeds=None):
        """nll_step_group for fusion='tensor' (the XlinearFusion / Kronecker head in the configuration nll_step takes: skip,
        scale width 16): the same window, the same `patients` forms, refusals and results.  The stacks and the omic batch
        write their embeddings into the columns of encoder2's input matrix (ops.xfusion_group_input); the XlinearFusion
        block and classifier[0] run as ONE call of four launches for the window (ops._xfusion_group_fwd_raw: encoder1's
        10 MB weight is read once per window, not once per patient), the hazard head with classifier[3] on hid [G x 256],
        and the fusion backward as one call (ops._xfusion_group_bwd_raw: encoder1's weight gradient is written once).
        Everything is issued on the current stream, in this order: radio forward, pathology forward, omic forward, fusion
        forward, head, fusion backward, pathology backward, omic backward, radio backward, hand_over_grads.

        Seeds: in train mode patient g draws ops.next_dropout_seed() in nll_step's order -- radio, path, omic, fusion for
        patient 0, then patient 1, ... -- so the same seed stream gives every patient the masks G nll_step calls give
        it; or `seeds` = {"radio": [G], "path": [G], "omic": [G], "fusion": [G]} (the branches in `mode`, and "fusion").
        The fusion seed of a patient keys its masks of the sites 0 .. 2 (o_i), 8 (product), 9, 10 (encoders) and 11
        (classifier[2])."""
        if self.fusion != "tensor":
            raise NotImplementedError("nll_step_group_tensor covers fusion='tensor'; the concat head has nll_step_group")
        if not self.xfusion_group_ok():
            raise NotImplementedError("nll_step_group_tensor covers the XlinearFusion configuration the heads use "
                                      "(skip, scale width 16)")
        return self._group_step("nll_step_group_tensor", patients, labels, censors, alpha, loss_scale, grad_out, accumulate,
                                seeds)

    def _group_step(self, what, patients, labels, censors, alpha, loss_scale, grad_out, accumulate, seeds):
        """The one body of nll_step_group and nll_step_group_tensor: the window checks, the seeds, the stack chains and
        the omic batch are the same; the fusion decides where the embeddings are written and what runs between the
        branches' forward and backward halves."""
        from ..ops import (_dense_rows_bwd_raw, _dense_rows_fwd_raw, _group_half_bwd_raw, _group_half_fwd_raw,
                           _xfusion_group_bwd_raw, _xfusion_group_fwd_raw)
        MmfError = ops._lib.MmfError
        tensor = self.fusion == "tensor"
        if ops._gemm != 0:
            raise MmfError(f"{what} runs the exact-fp32 GEMMs only (ops.set_gemm(0))")
        order, cols, F = self._concat_layout()
        params = list(self.parameters())
        if any(not p.requires_grad for p in params):
            raise RuntimeError(f"{what} needs every parameter to require grad")
        head = self.classifier[3] if tensor else self.classifier
        Wk, bk = head.weight, head.bias
        if Wk.shape[0] > 32:
            raise MmfError(f"{what}: the fused hazard head takes K <= 32 classes")
        path, radio, omic = self._stacked_patients(patients)
        G, Y, cc = self._window_checks(path, radio, omic, labels, censors)
        if not Y.is_cuda and bool(((Y < 0) | (Y >= Wk.shape[0])).any()):
            raise IndexError(f"nll_surv: label out of range [0, {Wk.shape[0]})")
        tr = self.training
        draws = [k for k in ("radio", "path", "omic") if k in order] + (["fusion"] if tensor else [])   # nll_step's order
        if seeds is None:
            seeds = {k: [0] * G for k in draws}
            if tr:
                for g in range(G):
                    for k in draws:
                        seeds[k][g] = ops.next_dropout_seed()
        elif any(k not in seeds or len(seeds[k]) != G for k in draws):
            raise MmfError(f"seeds: {G} dropout seeds for each of {draws}")
        dev = (path[0] if path is not None else radio[0][0] if radio is not None else omic).device
        grads = {}

        def stack_forward(seq, xs, sizes, k, Wr=None, br=None):
            gated, ps, p_h, p_att = stack_args(seq, tr)
            A, state = _group_half_fwd_raw(xs, sizes, ps, gated, p_h, p_att, seeds[k], slot[k], Wr, br)
            return A, (ps, state)

        def stack_backward(run, k):
            ps, state = run
            ds, rd = _group_half_bwd_raw(state, dslot[k])
            grads.update((p, gr) for p, gr in zip(ps, ds) if p is not None)
            return rd

        with torch.no_grad():
            # where branch k writes its embeddings: its columns of the [G x F] feature matrix (concat), or of encoder2's
            # input matrix behind encoder1's columns (tensor) -- either way the concatenation is never a launch
            if tensor:
                xw = self._xfusion_weights(len(order))
                x2, views = ops.xfusion_group_input(G, len(order), F // len(order), int(xw[6 * len(order)].shape[0]), dev)
                slot = dict(zip(order, views))
            else:
                feat = torch.empty((G, F), dtype=torch.float32, device=dev)
                slot = {k: feat[:, cols[k]] for k in order}
            A_raw = {}
            if "radio" in order:
                many = len(radio[0]) > 1         # one modality: no reduce_dim, the pathology pair on that bag
                A_raw["radiology"], run_r = stack_forward(self.attention_net_radio, radio[0], radio[1], "radio",
                                                          *((self.reduce_dim.weight, self.reduce_dim.bias) if many else ()))
            if "path" in order:
                A_raw["pathology"], run_p = stack_forward(self.attention_net_WSI, [path[0]], path[1], "path")
            if "omic" in order:
                word = ops._seed_word
                base = ops.dropout_row_base(seeds["omic"], dev)
                acts = [ops._f32c(omic)]
                nblk = len(self.fc_omic)
                for i, blk in enumerate(self.fc_omic):
                    lin, adrop = blk[0], blk[2]
                    acts.append(_dense_rows_fwd_raw(acts[-1], lin.weight, lin.bias, "selu", "alpha" if tr else "none",
                                                    adrop.p if tr else 0.0, i, base, word,
                                                    out=slot["omic"] if i == nblk - 1 else None))
            # ---- classifier + hazards + loss + their backward for every patient: one launch and its reduce
            dWk, dbk = torch.empty_like(Wk), torch.empty_like(bk)
            if tensor:
                # XlinearFusion + classifier[0] in front of it, their backward behind it (forward() lines 182-188)
                c0 = self.classifier[0]
                _, hid, xstate = _xfusion_group_fwd_raw(x2, len(order), xw, c0.weight, c0.bias,
                                                        self.mm.dropout_rate if tr else 0.0,
                                                        self.classifier[2].p if tr else 0.0, seeds["fusion"], ops._seed_word)
                hazards, S, Y_hat, loss, risk, dhid = ops.surv_head_nll_step_group(hid, Wk, bk, Y, cc, alpha, dWk, dbk,
                                                                                   loss_scale=loss_scale)
                dvs, gw = _xfusion_group_bwd_raw(dhid, xstate)
                grads.update(zip(xw + [c0.weight, c0.bias], gw))
                dslot = dict(zip(order, dvs))
            else:
                hazards, S, Y_hat, loss, risk, dfeat = ops.surv_head_nll_step_group(feat, Wk, bk, Y, cc, alpha, dWk, dbk,
                                                                                    loss_scale=loss_scale)
                dslot = {k: dfeat[:, cols[k]] for k in order}
            grads[Wk], grads[bk] = dWk, dbk
            if "path" in order:
                stack_backward(run_p, "path")
            if "omic" in order:
                g = dslot["omic"]
                for i in range(nblk - 1, -1, -1):
                    lin, adrop = self.fc_omic[i][0], self.fc_omic[i][2]
                    g, dW, db = _dense_rows_bwd_raw(g, acts[i + 1], acts[i], lin.weight, lin.bias is not None, "selu",
                                                    "alpha" if tr else "none", adrop.p if tr else 0.0, i, base,
                                                    need_dx=i > 0, word=word)
                    grads[lin.weight] = dW
                    if lin.bias is not None:
                        grads[lin.bias] = db
            if "radio" in order:
                rd = stack_backward(run_r, "radio")
                if rd is not None:
                    grads[self.reduce_dim.weight], grads[self.reduce_dim.bias] = rd
            hand_over_grads(params, grads, grad_out, accumulate)
        return hazards, S, Y_hat.view(-1), A_raw, loss, risk

    def _xfusion_weights(self, m):
        """XlinearFusion's weights in ops.xfusion's order: per modality (Wh, bh, Wz, bz, Wo, bo), then We1, be1, We2, be2."""
        fus = self.mm
        weights = []
        for i in range(m):
            for lin in (fus.reduce[i][0][0], fus.reduce[i][1][0], fus.reduce[i][2][0]):
                weights += [lin.weight, lin.bias]
        return weights + [fus.encoder1[0].weight, fus.encoder1[0].bias, fus.encoder2[0].weight, fus.encoder2[0].bias]

    def forward_group(self, patients, labels=None, censors=None, alpha=0.0, return_features=False):
        """The eval-mode forward of the G <= 64 patients of an evaluation window, both fusions -- validation and the
        summary evaluate one patient at a time with fixed weights (utils/core_utils.py:267-430 of the reference), and the
        patients are independent.  Each stack runs once over its branch's concatenated rows with no head behind it
        (ops.radio_infer_group / ops.amil_infer_group: M [G x 256]), the eval-mode SNN as one B = G batch, then
          concat: the hazard head on the embeddings where the branches left them (ops.surv_head_infer_group; no torch.cat);
          tensor: XlinearFusion + classifier[0] in one call of four launches (ops.xfusion_infer_group), the hazard head on hid.
        Everything is issued on the current stream, in the order radio, pathology, omic, fusion, head.

        patients: as nll_step_group takes them (a list of per-patient kwarg dicts, or the pre-stacked triple); labels /
        censors: G values for each patient's NLLSurvLoss(alpha) value, or None.  fp32 2-D bags, exact-fp32 GEMMs, K <= 32,
        eval mode; every refusal comes before the first launch.  Each patient gets what `model(**kwargs)` gives it under
        no_grad, to fp32 rounding.
        Returns (hazards [G x K], S [G x K], Y_hat [G], A_raw {"radiology": [per patient], "pathology": [per patient]},
        loss [G] or None, risk [G]), detached; return_features: the fused embedding [G x F] (concat) or [G x mmhid2]
        (tensor), as forward(return_features=True) returns it per patient."""
        from ..ops import _dense_fwd_raw
        MmfError = ops._lib.MmfError
        if self.training:
            raise RuntimeError("forward_group is the eval-mode pass: call model.eval() first")
        if ops._gemm != 0:
            raise MmfError("forward_group runs the exact-fp32 GEMMs only (ops.set_gemm(0))")
        order, _, F = self._concat_layout()
        tensor = self.fusion == "tensor"
        if tensor and not self.xfusion_step_ok():
            raise NotImplementedError("forward_group covers the XlinearFusion configuration the heads use (skip)")
        head = self.classifier[3] if tensor else self.classifier
        Wk, bk = head.weight, head.bias
        if Wk.shape[0] > 32:
            raise MmfError("forward_group: the fused hazard head takes K <= 32 classes")
        path, radio, omic = self._stacked_patients(patients)
        G, Y, cc = self._window_checks(path, radio, omic, labels, censors, forward_only=True)
        with torch.no_grad():
            A_raw, emb = {}, {}
            if "radio" in order:
                gated, stack, _, _ = stack_args(self.attention_net_radio, False)
                if len(radio[0]) > 1:
                    out = ops.radio_infer_group(radio[0], radio[1], self.reduce_dim.weight, self.reduce_dim.bias, stack,
                                                gated, want_M=True)
                else:                          # one modality: no reduce_dim, the pathology pass on that bag
                    out = ops.amil_infer_group(radio[0][0], radio[1], stack, gated, want_M=True)
                A_raw["radiology"], emb["radio"] = out[4], out[5]
            if "path" in order:
                gated, stack, _, _ = stack_args(self.attention_net_WSI, False)
                out = ops.amil_infer_group(path[0], path[1], stack, gated, want_M=True)
                A_raw["pathology"], emb["path"] = out[4], out[5]
            if "omic" in order:
                x = ops._f32c(omic)
                for i, blk in enumerate(self.fc_omic):
                    x = _dense_fwd_raw(x, blk[0].weight, blk[0].bias, "selu", "none", 0.0, 0, i)
                emb["omic"] = x
            vs = [emb[k] for k in order]
            if tensor:
                c0 = self.classifier[0]
                MM, hid = ops.xfusion_infer_group(vs, self._xfusion_weights(len(order)), c0.weight, c0.bias)
                segs = [hid]
            else:
                MM, segs = None, vs
            if return_features:
                return MM if tensor else torch.cat(vs, dim=1)
            hazards, S, Y_hat, loss, risk = ops.surv_head_infer_group(segs, Wk, bk, Y, cc, alpha)
        return hazards, S, Y_hat.view(-1), A_raw, loss, risk

    def integrated_gradients(self, n_steps=20, method="gausslegendre", return_full=False, window_steps=0, **features):
        """How much of the predicted risk comes from radiology, pathology and omics: integrated gradients of
        risk = -sum(S) with respect to every input from a joint zero baseline, in ONE C-ABI call
        (ops.mm_integrated_gradients) -- what the reference's create_attributions.py:93-164 gets from captum through n_steps
        autograd passes of the whole forward.  features: what forward takes for self.mode ({modality: [N_r x k]},
        path_features [N_p x L], genomic_features [G] or [1 x G]), fp32; method, window_steps as
        MIL_Attention_fc_surv_path.integrated_gradients.  fusion='concat' (fusion='tensor': integrated_gradients_tensor),
        eval mode, the stock head only.
        Returns ModalityAttribution: modality_attr / modality_abs {radio, path, omic} (the abs values are the reference's
        radio_attr, path_attr, omic_attr), share = modality_abs / their sum, patch_attr / patch_abs [N_p], inst_attr /
        inst_abs [n_mod x N_r], sequence_abs [n_mod], gene_attr [G], total, total_abs, risk, risk_baseline,
        delta = total - (risk - risk_baseline), step_risk [n_steps], hazards, S, Y_hat at alpha = 1, and with return_full
        attr {radio: [n_mod x N_r x k], path: [N_p x L], omic: [G]}.  The fields of an absent branch are None."""
        if self.fusion == "tensor":
            raise NotImplementedError("integrated_gradients covers fusion='concat'; a tensor-fusion model has "
                                      "integrated_gradients_tensor")
        return self._integrated_gradients(False, n_steps, method, return_full, window_steps, features)

    def integrated_gradients_tensor(self, n_steps=20, method="gausslegendre", return_full=False, window_steps=0, **features):
        """integrated_gradients for fusion='tensor', the default: the same question, arguments and ModalityAttribution, in ONE
        C-ABI call (ops.mm_integrated_gradients with xfusion) -- per window of nodes the XlinearFusion block, classifier[0],
        the hazard head and their input gradients run as seven launches between the branches' halves, and no weight
        gradient is formed.  The XlinearFusion configuration nll_step_group_tensor takes (skip, scale width 16), eval mode,
        the stock head only; a concat model has integrated_gradients."""
        if self.fusion != "tensor":
            raise NotImplementedError("integrated_gradients_tensor covers fusion='tensor'; a concat model has "
                                      "integrated_gradients")
        if not self.xfusion_group_ok():
            raise NotImplementedError("integrated_gradients_tensor covers the XlinearFusion configuration the heads use "
                                      "(skip, scale width 16)")
        return self._integrated_gradients(True, n_steps, method, return_full, window_steps, features)

    def _integrated_gradients(self, tensor, n_steps, method, return_full, window_steps, features):
        """The one body of integrated_gradients and integrated_gradients_tensor: the refusals, the branches' operands, the
        call and the ModalityAttribution."""
        MmfError = ops._lib.MmfError
        order, _, _ = self._concat_layout()
        need = {"radio": list(self.modalities), "path": ["path_features"], "omic": ["genomic_features"]}
        missing = [k for b in order for k in need[b] if features.get(k) is None]
        if missing:
            raise MmfError(f"mode {self.mode!r} needs {missing}")
        bags = [features[m] for m in self.modalities] if "radio" in order else []
        tensors = bags + [features[k] for b in order if b != "radio" for k in need[b]]
        ig_refusals(self, "mm", tensors, bags)
        if "radio" in order and len(bags) < 2:
            raise NotImplementedError("integrated_gradients takes 2 .. 4 radiology sequences behind reduce_dim")
        branches = []
        for b in order:
            if b == "radio":
                gated, stack, _, _ = stack_args(self.attention_net_radio, False)
                branches.append(("radio", bags, self.reduce_dim.weight, self.reduce_dim.bias, stack, gated))
            elif b == "path":
                gated, stack, _, _ = stack_args(self.attention_net_WSI, False)
                branches.append(("path", features["path_features"], stack, gated))
            else:
                x = features["genomic_features"]
                G_in = self.fc_omic[0][0].in_features
                if x.numel() != G_in or x.dim() > 2:
                    raise MmfError(f"genomic_features must be [{G_in}] or [1 x {G_in}], got {tuple(x.shape)}")
                l0, l1 = self.fc_omic[0][0], self.fc_omic[1][0]
                branches.append(("omic", x.reshape(-1), l0.weight, l0.bias, l1.weight, l1.bias))
        alphas, weights = ops.ig_quadrature(method, n_steps)
        with torch.no_grad():
            head, xfusion = self.classifier, None
            if tensor:
                c0, head = self.classifier[0], self.classifier[3]
                xfusion = (self._xfusion_weights(len(order)), c0.weight, c0.bias)
            out, risk, base, step_risk, (hazards, S, Y_hat) = ops.mm_integrated_gradients(
                branches, head.weight, head.bias, alphas, weights, want_attr=return_full, window_steps=window_steps,
                xfusion=xfusion)
            f = dict.fromkeys(("patch_attr", "patch_abs", "inst_attr", "inst_abs", "sequence_abs", "gene_attr"))
            m_attr, m_abs, full = dict.fromkeys(need), dict.fromkeys(need), dict.fromkeys(need)
            if "path" in out:
                f["patch_attr"], f["patch_abs"], full["path"] = out["path"]
                m_attr["path"], m_abs["path"] = f["patch_attr"].sum(), f["patch_abs"].sum()
            if "radio" in out:
                f["inst_attr"], f["inst_abs"], full["radio"] = out["radio"]
                f["sequence_abs"] = f["inst_abs"].sum(-1)
                m_attr["radio"], m_abs["radio"] = f["inst_attr"].sum(), f["sequence_abs"].sum()
            if "omic" in out:
                f["gene_attr"] = full["omic"] = out["omic"]
                m_attr["omic"], m_abs["omic"] = out["omic"].sum(), out["omic"].abs().sum()
            total = sum(m_attr[b] for b in order)
            total_abs = sum(m_abs[b] for b in order)
            share = {b: (m_abs[b] / total_abs if b in order else None) for b in need}
            delta = total - (risk[0] - base[0])
        return ModalityAttribution(m_attr, m_abs, share, f["patch_attr"], f["patch_abs"], f["inst_attr"], f["inst_abs"],
                                   f["sequence_abs"], f["gene_attr"], total, total_abs, risk[0], base[0], delta, step_risk,
                                   hazards, S, Y_hat, full if return_full else None)

    def forward(self, **kwargs):
        A_raw = {}
        path_x = kwargs.get("path_features") if "path" in self.mode else None
        cur, side, branch = self._fork(path_x)
        fork = side is not None
        joined = []
        # python order (and with it the dropout-seed order) stays radio, path, omic, fusion
        if "radio" in self.mode:
            with branch():
                h_radio = [kwargs[m] for m in self.modalities]
                if fork:
                    for t in h_radio:
                        t.record_stream(side)
                if len(self.modalities) > 1:
                    h_radio = ops.linear_cat(h_radio, self.reduce_dim.weight, self.reduce_dim.bias)
                else:
                    h_radio = h_radio[0]
                M_radio, A_raw["radiology"] = amil_stack(self.attention_net_radio, h_radio, self.training)
                joined += [M_radio, A_raw["radiology"]]
        if "path" in self.mode:
            # with the small branches on the side stream the pathology stack plans its wide tiles for 224 CUs (the hint of
            # mmf_amil_desc::concurrent): the branches' kernels then find CUs while a projection / K-dh launch is resident
            # instead of waiting for it to drain (as one hipGraph 1.13 -> 1.05 ms)
            prev = ops.set_concurrent(True) if fork else None
            M_path, A_raw["pathology"] = amil_stack(self.attention_net_WSI, kwargs["path_features"], self.training)
            if fork:
                ops.set_concurrent(prev)
        if "omic" in self.mode:
            with branch():
                X = kwargs["genomic_features"]
                if fork:
                    X.record_stream(side)
                if X.dim() == 1:
                    X = X.unsqueeze(0)
                O = snn_stack(self.fc_omic, X, self.training)
                joined.append(O)
        if fork:
            cur.wait_stream(side)
            for t in joined:
                t.record_stream(cur)

        emb = {"radio": M_radio if "radio" in self.mode else None, "path": M_path if "path" in self.mode else None,
               "omic": O if "omic" in self.mode else None}
        v_list = [emb[k] for k in self._concat_order()]

        if self.fusion == "tensor":
            seed = ops.next_dropout_seed() if self.training else 0
            MM = self.mm(v_list=v_list, seed=seed)
            c0, c3 = self.classifier[0], self.classifier[3]
            hid = ops.dense(MM, c0.weight, c0.bias, act="relu", drop_kind="dropout" if self.training else "none",
                            drop_p=self.classifier[2].p if self.training else 0.0, seed=seed, site=11)
            hazards, S, Y_hat = ops.surv_head(hid, c3.weight, c3.bias)
        else:
            MM = torch.cat(v_list, dim=1)
            hazards, S, Y_hat = ops.surv_head(MM, self.classifier.weight, self.classifier.bias)
        if kwargs.get("return_features"):
            return MM
        return hazards, S, Y_hat, A_raw
