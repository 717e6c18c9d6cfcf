"""The route each bag takes through train_loop_survival (utils/core_utils._bag_route) and the head kind of an evaluation
pass (_eval_group_head), as tables: (head, loss, inputs, switches) -> answer.  No GPU: a tensor "on the device" only
claims to be one, and whether the loop's copy would land on a GPU is patched in per row.

The tables state what the loops did BEFORE the routes were gathered into one function: they were first run against the old
predicates and the old flag lines of the loop, wrapped as a route function, and only then against _bag_route."""
import pytest
import torch

from multimodalfusion_amd.models import (MaxNet, MIL_Attention_fc_surv_path, MIL_Attention_fc_surv_radio,
                                         MM_MIL_Attention_fc_surv)
from multimodalfusion_amd.models.model_modules import XlinearFusion
from multimodalfusion_amd.utils import core_utils
from multimodalfusion_amd.utils.loss_utils import CoxSurvLoss, NLLSurvLoss


class OnDevice(torch.Tensor):
    @property
    def is_cuda(self):
        return True


class OtherNLL(NLLSurvLoss):
    pass


class OtherCox(CoxSurvLoss):
    pass


LOSSES = {"nll": lambda: NLLSurvLoss(alpha=0.0), "other_nll": lambda: OtherNLL(alpha=0.0), "cox": CoxSurvLoss,
          "other_cox": OtherCox}
MODS2 = ["T1", "T2"]


def _head(head, K=4, override=False, size="small", gate=True, omic_loss="cox_surv", width=16, skip=1):
    base, kw = {"path": (MIL_Attention_fc_surv_path, dict(n_classes=K, model_size_wsi=size, gate_path=gate)),
                "radio": (MIL_Attention_fc_surv_radio, dict(n_classes=K, modalities=MODS2)),
                "concat": (MM_MIL_Attention_fc_surv, dict(n_classes=K, fusion="concat")),
                "tensor": (MM_MIL_Attention_fc_surv, dict(n_classes=K, fusion="tensor")),
                "omic": (MaxNet, dict(input_dim=80, bag_loss=omic_loss, n_classes=K)),
                "other": (torch.nn.Linear, dict(in_features=4, out_features=4))}[head]
    if override:
        class Tweaked(base):
            def forward(self, *a, **k):
                return super().forward(*a, **k)
        base = Tweaked
    model = base(**kw)
    if head == "tensor" and width != 16:
        model.mm = XlinearFusion(dim=256, scale_dim=256 // width, mmhid1=512, mmhid2=512, num_modalities=3, gate=True, skip=1)
    if head == "tensor":
        model.mm.skip = skip
    return model


def _inputs(head, where="dev", dtype=torch.float32, unequal=False, omic_width=80, dim3=False, rows=3):
    """The smallest inputs that still decide a route: a 4 x 1024 pathology bag, 2 x 1024 per modality, an 80-wide omic row
    (the omic head: a batch of `rows` of them); the other modalities are the dataset's "missing" sentinel."""
    put = (lambda t: t.as_subclass(OnDevice)) if where == "dev" else (lambda t: t)
    missing = lambda: put(torch.zeros(1, 1))
    radio, path, omic = {}, missing(), missing()
    if head in ("path", "concat", "tensor", "other"):
        path = put(torch.zeros((4, 2, 512) if dim3 else (4, 1024), dtype=dtype))
    if head in ("radio", "concat", "tensor"):
        mods = MODS2 if head == "radio" else ["T1", "T2", "T1Gd", "FLAIR"]
        radio = {m: put(torch.zeros((3 if unequal and i == 1 else 2, 1024), dtype=dtype if head == "radio" else torch.float32))
                 for i, m in enumerate(mods)}
    if head in ("concat", "tensor"):
        omic = put(torch.zeros(1, omic_width))
    if head == "omic":
        omic = put(torch.zeros((rows, omic_width), dtype=dtype))
    return radio, path, omic


def R(head, route, loss="nll", group=False, inflight=1, gemm=0, gpu=False, **kw):
    return pytest.param(head, route, loss, group, inflight, gemm, gpu, kw,
                        id="-".join([head, loss, f"group{int(group)}", f"inflight{inflight}", f"gemm{gemm}", f"gpu{int(gpu)}"]
                                    + [f"{k}={getattr(v, '__name__', v) if not isinstance(v, torch.dtype) else str(v)[6:]}"
                                       for k, v in kw.items()]))


BF16, FP64 = torch.bfloat16, torch.float64
ROUTES = [
    # ---- the pathology head: its one-call step ignores mmf_one_call_step; a bf16 bag is never held
    R("path", "step-path"), R("path", "autograd", where="host"), R("path", "step-path", where="host", gpu=True),
    R("path", "autograd", override=True), R("path", "autograd", hook="module"), R("path", "autograd", hook="global"),
    R("path", "autograd", frozen=True), R("path", "autograd", K=33), R("path", "step-path", K=32),
    R("path", "autograd", loss="other_nll"), R("path", "autograd", loss="cox"), R("path", "step-path", one_call=False),
    R("path", "step-path", dtype=BF16), R("path", "autograd", dtype=FP64), R("path", "autograd", dim3=True),
    R("path", "step-path", gemm=1), R("path", "step-path", group=True, gemm=1),
    R("path", "held-path", group=True), R("path", "autograd", group=True, where="host"),
    R("path", "held-path", group=True, where="host", gpu=True), R("path", "step-path", group=True, dtype=BF16),
    R("path", "autograd", group=True, dtype=FP64), R("path", "autograd", group=True, hook="module"),
    R("path", "autograd", group=True, frozen=True), R("path", "held-path", group=True, one_call=False),
    R("path", "autograd", group=True, loss="other_nll"),
    R("path", "pipe-fused", inflight=2), R("path", "pipe-fused", inflight=2, dtype=BF16),
    R("path", "pipe-fused", inflight=2, where="host", gpu=True), R("path", "pipe-autograd", inflight=2, where="host"),
    R("path", "pipe-autograd", inflight=2, dtype=FP64), R("path", "pipe-autograd", inflight=2, hook="module"),
    R("path", "pipe-autograd", inflight=2, loss="other_nll"), R("path", "pipe-autograd", inflight=2, override=True),
    # ---- the radiology head: honours mmf_one_call_step; fp32 modalities of one shape; held straight from the host
    R("radio", "step-radio"), R("radio", "autograd", where="host"), R("radio", "step-radio", where="host", gpu=True),
    R("radio", "autograd", override=True), R("radio", "autograd", hook="module"), R("radio", "autograd", hook="global"),
    R("radio", "autograd", frozen=True), R("radio", "autograd", K=33), R("radio", "autograd", loss="other_nll"),
    R("radio", "autograd", one_call=False), R("radio", "autograd", dtype=BF16), R("radio", "autograd", dtype=FP64),
    R("radio", "autograd", unequal=True), R("radio", "step-radio", gemm=1),
    R("radio", "held-radio", group=True), R("radio", "held-radio", group=True, where="host"),
    R("radio", "held-radio", group=True, where="host", gpu=True),
    R("radio", "step-radio", group=True, gemm=1), R("radio", "autograd", group=True, gemm=1, where="host"),
    R("radio", "step-radio", group=True, gemm=1, where="host", gpu=True),
    R("radio", "autograd", group=True, one_call=False), R("radio", "autograd", group=True, dtype=BF16),
    R("radio", "autograd", group=True, unequal=True), R("radio", "autograd", group=True, hook="global"),
    R("radio", "autograd", group=True, frozen=True), R("radio", "autograd", group=True, K=33),
    R("radio", "pipe-autograd", inflight=2), R("radio", "pipe-autograd", inflight=2, hook="module"),
    # ---- the multimodal head, concat fusion: the per-patient step asks nothing of the bags but where they are
    R("concat", "step-mm"), R("concat", "autograd", where="host"), R("concat", "step-mm", where="host", gpu=True),
    R("concat", "autograd", override=True), R("concat", "autograd", hook="module"), R("concat", "autograd", hook="global"),
    R("concat", "autograd", frozen=True), R("concat", "autograd", K=33), R("concat", "autograd", loss="other_nll"),
    R("concat", "autograd", one_call=False), R("concat", "step-mm", dtype=BF16), R("concat", "step-mm", dtype=FP64),
    R("concat", "step-mm", unequal=True), R("concat", "step-mm", omic_width=81), R("concat", "step-mm", gemm=1),
    R("concat", "held-mm", group=True), R("concat", "held-mm", group=True, where="host"),
    R("concat", "held-mm", group=True, where="host", gpu=True), R("concat", "step-mm", group=True, gemm=1),
    R("concat", "step-mm", group=True, dtype=BF16), R("concat", "autograd", group=True, dtype=BF16, where="host"),
    R("concat", "step-mm", group=True, unequal=True), R("concat", "autograd", group=True, unequal=True, where="host"),
    R("concat", "step-mm", group=True, omic_width=81), R("concat", "autograd", group=True, omic_width=81, where="host"),
    R("concat", "autograd", group=True, one_call=False), R("concat", "autograd", group=True, hook="module"),
    R("concat", "autograd", group=True, frozen=True), R("concat", "held-mm", group=True, group_tensor=True),
    R("concat", "pipe-autograd", inflight=2),
    # ---- tensor fusion: per patient within 384 fused columns; held only when opted in, with scale width 16
    R("tensor", "step-mm"), R("tensor", "autograd", where="host"), R("tensor", "step-mm", group=True),
    R("tensor", "autograd", group=True, where="host"), R("tensor", "step-mm", group_tensor=True),
    R("tensor", "held-mm", group=True, group_tensor=True), R("tensor", "held-mm", group=True, group_tensor=True, where="host"),
    R("tensor", "step-mm", group=True, group_tensor=True, gemm=1),
    R("tensor", "step-mm", group=True, group_tensor=True, dtype=BF16),
    R("tensor", "step-mm", width=32), R("tensor", "step-mm", group=True, group_tensor=True, width=32),
    R("tensor", "autograd", group=True, group_tensor=True, width=32, where="host"),
    R("tensor", "autograd", skip=0),
    R("tensor", "autograd", group=True, group_tensor=True, skip=0), R("tensor", "autograd", K=33),
    R("tensor", "autograd", one_call=False), R("tensor", "autograd", group=True, group_tensor=True, one_call=False),
    R("tensor", "autograd", hook="module"), R("tensor", "autograd", group=True, group_tensor=True, frozen=True),
    R("tensor", "pipe-autograd", inflight=2, group_tensor=True),
    # ---- the omic head: no requires_grad test of the loop's own (cox_step_ok has one), no switch, any dtype (the copy
    # makes the batch fp32)
    R("omic", "step-cox", loss="cox"), R("omic", "autograd", loss="cox", where="host"),
    R("omic", "step-cox", loss="cox", where="host", gpu=True), R("omic", "autograd", loss="cox", override=True),
    R("omic", "autograd", loss="cox", hook="module"), R("omic", "autograd", loss="cox", hook="global"),
    R("omic", "autograd", loss="cox", frozen=True), R("omic", "autograd", loss="nll"),
    R("omic", "autograd", loss="other_cox"), R("omic", "step-cox", loss="cox", dtype=FP64),
    R("omic", "step-cox", loss="cox", one_call=False), R("omic", "step-cox", loss="cox", group=True),
    R("omic", "step-cox", loss="cox", gemm=1), R("omic", "autograd", loss="cox", rows=300),
    R("omic", "autograd", loss="cox", omic_width=300), R("omic", "autograd", loss="cox", omic_loss="nll_surv"),
    R("omic", "pipe-autograd", loss="cox", inflight=2),
    # ---- any other module
    R("other", "autograd"), R("other", "autograd", group=True), R("other", "pipe-autograd", inflight=2),
]

_MODEL_KEYS = ("K", "override", "size", "gate", "omic_loss", "width", "skip")
_INPUT_KEYS = ("where", "dtype", "unequal", "omic_width", "dim3", "rows")


def _switched(head, kw):
    """The model of a row with its switches set; the handle of a hook it registered, to be removed."""
    model = _head(head, **{k: v for k, v in kw.items() if k in _MODEL_KEYS})
    handle = None
    if kw.get("hook") == "module":
        handle = list(model.modules())[-1].register_forward_hook(lambda m, i, o: None)       # a SUB-module hook
    elif kw.get("hook") == "global":
        handle = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
    if kw.get("frozen"):
        next(iter(model.parameters())).requires_grad_(False)
    if "one_call" in kw:
        model.mmf_one_call_step = kw["one_call"]
    if "group_tensor" in kw:
        model.mmf_group_tensor = kw["group_tensor"]
    return model, handle


@pytest.mark.parametrize("head, route, loss, group, inflight, gemm, gpu, kw", ROUTES)
def test_bag_route(monkeypatch, head, route, loss, group, inflight, gemm, gpu, kw):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: gpu)         # where the loop's copy would leave a host tensor
    model, handle = _switched(head, kw)
    try:
        inputs = _inputs(head, **{k: v for k, v in kw.items() if k in _INPUT_KEYS})
        assert core_utils._bag_route(model, LOSSES[loss](), *inputs, group, inflight, gemm) == route
    finally:
        if handle is not None:
            handle.remove()


def test_a_hook_registered_mid_epoch_counts_from_the_next_bag():
    """The route is asked per bag, not once per epoch."""
    model, inputs, loss = _head("path"), _inputs("path"), NLLSurvLoss(alpha=0.0)
    assert core_utils._bag_route(model, loss, *inputs) == "step-path"
    handle = model.classifier.register_forward_pre_hook(lambda m, i: None)
    assert core_utils._bag_route(model, loss, *inputs) == "autograd"
    handle.remove()
    assert core_utils._bag_route(model, loss, *inputs) == "step-path"


def test_the_route_walks_the_modules_once(monkeypatch):
    for head in ("path", "radio", "concat", "tensor", "omic"):
        model, walks = _head(head), []
        real = model.modules
        monkeypatch.setattr(model, "modules", lambda: (walks.append(1), real())[1])
        core_utils._bag_route(model, LOSSES["cox" if head == "omic" else "nll"](), *_inputs(head), True, 1, 0)
        assert len(walks) <= 1, (head, walks)


def E(head, kind, gemm=0, **kw):
    return pytest.param(head, kind, gemm, kw, id="-".join([head, f"gemm{gemm}"] + [f"{k}={v}" for k, v in kw.items()]))


EVAL_KINDS = [
    # the `small` gated pathology head takes fused bf16 forms one bag at a time: its grouped pass is fp32 only
    E("path", "path_fp32"), E("path", "path", size="big"), E("path", "path", gate=False),
    E("path", None, override=True), E("path", None, hook="module"), E("path", None, hook="global"), E("path", None, K=33),
    E("path", "path_fp32", K=32), E("path", "path_fp32", frozen=True), E("path", "path_fp32", one_call=False),
    E("path", None, gemm=1),
    E("radio", "radio"), E("radio", None, override=True), E("radio", None, hook="module"), E("radio", None, hook="global"),
    E("radio", None, K=33), E("radio", "radio", frozen=True), E("radio", "radio", one_call=False), E("radio", None, gemm=1),
    E("concat", "mm"), E("concat", None, override=True), E("concat", None, hook="module"), E("concat", None, K=33),
    E("concat", "mm", frozen=True), E("concat", "mm", one_call=False), E("concat", None, gemm=1),
    E("tensor", "mm"), E("tensor", "mm", width=32), E("tensor", None, skip=0),
    E("tensor", None, K=33), E("tensor", None, hook="global"), E("tensor", "mm", group_tensor=True), E("tensor", None, gemm=1),
    E("omic", None), E("other", None),
]


@pytest.mark.parametrize("head, kind, gemm, kw", EVAL_KINDS)
def test_eval_group_head(monkeypatch, head, kind, gemm, kw):
    from multimodalfusion_amd import ops
    monkeypatch.setattr(ops, "_gemm", gemm)
    model, handle = _switched(head, kw)
    try:
        assert core_utils._eval_group_head(model) == kind
    finally:
        if handle is not None:
            handle.remove()
