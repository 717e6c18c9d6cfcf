"""ctypes binding of libmmf_amil.so (C ABI: include/mmf_amil.h).

There is no CPU fallback: if the shared library is missing or a call is made with
non-GPU tensors the functions raise.  The library itself is only *loaded* here (symbol
resolution); no HIP call happens until an entry point is invoked.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMF_LIB_PATH") or os.path.join(_HERE, "libmmf_amil.so")   # override: the tuning build (tools/diag_build.py)

ABI_VERSION = 12

c_f32p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())


class AmilDesc(C.Structure):
    """struct mmf_amil_desc (include/mmf_amil.h)."""
    _fields_ = [
        ("N", C.c_int64), ("L", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("gated", C.c_int32),
        ("W1", C.c_void_p), ("b1", C.c_void_p), ("Wa", C.c_void_p), ("ba", C.c_void_p),
        ("Wb", C.c_void_p), ("bb", C.c_void_p), ("Wc", C.c_void_p), ("bc", C.c_void_p),
        ("p_h", C.c_float), ("p_att", C.c_float), ("seed", C.c_uint32),
        ("seed_dev", C.c_void_p), ("trace", C.c_void_p), ("concurrent", C.c_int32), ("gemm", C.c_int32),
        ("sync", C.c_void_p), ("sync_words", C.c_int32),
    ]


class AmilGrads(C.Structure):
    """struct mmf_amil_grads (include/mmf_amil.h)."""
    _fields_ = [
        ("dW1", C.c_void_p), ("db1", C.c_void_p), ("dWa", C.c_void_p), ("dba", C.c_void_p),
        ("dWb", C.c_void_p), ("dbb", C.c_void_p), ("dWc", C.c_void_p), ("dbc", C.c_void_p),
        ("dx", C.c_void_p),
    ]


class SurvHead(C.Structure):
    """struct mmf_surv_head (include/mmf_amil.h)."""
    _fields_ = [("Wk", C.c_void_p), ("bk", C.c_void_p), ("K", C.c_int32), ("logits", C.c_void_p),
                ("hazards", C.c_void_p), ("S", C.c_void_p), ("Y_hat", C.c_void_p), ("risk", C.c_void_p)]


class NllTarget(C.Structure):
    """struct mmf_nll_target (include/mmf_amil.h)."""
    _fields_ = [("Y", C.c_void_p), ("c", C.c_void_p), ("alpha", C.c_float), ("eps", C.c_float),
                ("loss_scale", C.c_float), ("loss", C.c_void_p), ("dWk", C.c_void_p), ("dbk", C.c_void_p),
                ("accumulate", C.c_int32)]


class BagGroup(C.Structure):
    """mmf_bag_group: the bags of one grouped step (host arrays)."""
    _fields_ = [("G", C.c_int32), ("offsets", C.POINTER(C.c_int64)), ("seeds", C.POINTER(C.c_uint32))]


class IgDesc(C.Structure):
    """struct mmf_ig_desc (include/mmf_amil.h): alpha / weight are host arrays, the outputs device pointers."""
    _fields_ = [("n_steps", C.c_int32), ("alpha", C.POINTER(C.c_float)), ("weight", C.POINTER(C.c_float)),
                ("window_steps", C.c_int32), ("row_sum", C.c_void_p), ("row_abs", C.c_void_p), ("attr", C.c_void_p),
                ("risk_x", C.c_void_p), ("risk_base", C.c_void_p), ("step_risk", C.c_void_p)]


class RadioReduce(C.Structure):
    """mmf_radio_reduce: the radiology head's reduce_dim in a grouped step (x: host array of nseg device pointers)."""
    _fields_ = [("x", C.POINTER(C.c_void_p)), ("nseg", C.c_int32), ("kseg", C.c_int32), ("W", c_f32p),
                ("bias", c_f32p), ("dW", c_f32p), ("db", c_f32p)]


class MmIgDesc(C.Structure):
    """struct mmf_mm_ig_desc (include/mmf_amil.h): alpha / weight are host arrays, path / radio / rd point at host structs
    (NULL: the branch is absent; omic: omic_x NULL), everything else is a device pointer."""
    _fields_ = [("n_steps", C.c_int32), ("window_steps", C.c_int32), ("alpha", C.POINTER(C.c_float)),
                ("weight", C.POINTER(C.c_float)),
                ("path", C.POINTER(AmilDesc)), ("path_x", C.c_void_p), ("path_row_sum", C.c_void_p),
                ("path_row_abs", C.c_void_p), ("path_attr", C.c_void_p),
                ("radio", C.POINTER(AmilDesc)), ("rd", C.POINTER(RadioReduce)), ("radio_row_sum", C.c_void_p),
                ("radio_row_abs", C.c_void_p), ("radio_attr", C.c_void_p),
                ("omic_x", C.c_void_p), ("omic_W0", C.c_void_p), ("omic_b0", C.c_void_p), ("omic_W1", C.c_void_p),
                ("omic_b1", C.c_void_p), ("omic_attr", C.c_void_p),
                ("omic_Gin", C.c_int32), ("omic_W0n", C.c_int32), ("omic_We", C.c_int32),
                ("path_col", C.c_int32), ("radio_col", C.c_int32), ("omic_col", C.c_int32),
                ("risk_x", C.c_void_p), ("risk_base", C.c_void_p), ("step_risk", C.c_void_p)]


class MaxnetDesc(C.Structure):
    """struct mmf_maxnet_desc (include/mmf_amil.h)."""
    _fields_ = [("B", C.c_int32), ("G", C.c_int32), ("H0", C.c_int32), ("H1", C.c_int32),
                ("x", C.c_void_p), ("W0", C.c_void_p), ("b0", C.c_void_p), ("W1", C.c_void_p), ("b1", C.c_void_p),
                ("Wc", C.c_void_p), ("bc", C.c_void_p), ("p_drop", C.c_float), ("seed", C.c_uint32),
                ("seed_dev", C.c_void_p), ("sync", C.c_void_p), ("sync_words", C.c_int32), ("trace", C.c_void_p)]


class MaxnetGrads(C.Structure):
    """struct mmf_maxnet_grads (include/mmf_amil.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("dW0", "db0", "dW1", "db1", "dWc", "dbc")]


class XReduceIO(C.Structure):
    """struct mmf_xreduce_io (include/mmf_amil.h)."""
    _P3 = C.c_void_p * 3
    _fields_ = [("m", C.c_int32), ("B", C.c_int32), ("dim", C.c_int32), ("sdim", C.c_int32)] + [
        (n, C.c_void_p * 3) for n in ("v", "Wh", "bh", "Wz", "bz", "Wo", "bo", "h", "z", "gm", "o", "d_o", "dv",
                                      "dWh", "dbh", "dWz", "dbz", "dWo", "dbo")]


class XFusionWeights(C.Structure):
    """struct mmf_xfusion_weights (include/mmf_amil.h)."""
    _fields_ = [(n, C.c_int32) for n in ("m", "dim", "sdim", "mmhid1", "mmhid2", "nhid")] + [
        (n, C.c_void_p * 3) for n in ("Wh", "bh", "Wz", "bz", "Wo", "bo")] + [
        (n, C.c_void_p) for n in ("We1", "be1", "We2", "be2", "Wc0", "bc0")]


class XFusionGrads(C.Structure):
    """struct mmf_xfusion_grads (include/mmf_amil.h)."""
    _fields_ = [(n, C.c_void_p * 3) for n in ("dWh", "dbh", "dWz", "dbz", "dWo", "dbo")] + [
        (n, C.c_void_p) for n in ("dWe1", "dbe1", "dWe2", "dbe2", "dWc0", "dbc0")]


class Bn1d(C.Structure):
    """struct mmf_bn1d (include/mmf_amil.h): nn.BatchNorm1d in eval mode."""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p), ("eps", C.c_float)]


class Stage2Block(C.Structure):
    """struct mmf_stage2_block (include/mmf_amil.h): the per-layer members are host arrays of device pointers."""
    _fields_ = [("W0", C.c_void_p), ("b0", C.c_void_p), ("bn", Bn1d), ("W4", C.c_void_p), ("b4", C.c_void_p),
                ("bn1", Bn1d), ("bn2", Bn1d)] + [
        (n, C.POINTER(C.c_void_p)) for n in ("Wgate", "bgate", "Wnl", "bnl", "Wlin", "blin")]


class Stage2IgDesc(C.Structure):
    """struct mmf_stage2_ig_desc (include/mmf_amil.h): alpha / weight are host arrays, xf points at a host struct."""
    _fields_ = [(n, C.c_int32) for n in ("family", "train_type", "radio", "path", "omic", "n_layers", "P", "K", "n_steps")] + [
        ("alpha", C.POINTER(C.c_float)), ("weight", C.POINTER(C.c_float)), ("v", C.c_void_p * 3), ("blk", Stage2Block * 3),
        ("xf", C.POINTER(XFusionWeights)), ("Wk", C.c_void_p), ("bk", C.c_void_p), ("mod_sum", C.c_void_p),
        ("mod_abs", C.c_void_p), ("attr", C.c_void_p * 3), ("risk", C.c_void_p), ("risk_base", C.c_void_p),
        ("step_risk", C.c_void_p), ("hazards", C.c_void_p), ("S", C.c_void_p), ("trace", C.c_void_p)]


class Stage2BnTrain(C.Structure):
    """struct mmf_stage2_bn_train (include/mmf_amil.h): nn.BatchNorm1d with running statistics a step moves."""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("eps", C.c_float), ("momentum", C.c_float)]


class Stage2StepBlock(C.Structure):
    """struct mmf_stage2_step_block (include/mmf_amil.h): the per-layer members are host arrays of device pointers."""
    _fields_ = [("W0", C.c_void_p), ("b0", C.c_void_p), ("bn", Stage2BnTrain), ("W4", C.c_void_p), ("b4", C.c_void_p),
                ("bn1", Stage2BnTrain), ("bn2", Stage2BnTrain)] + [
        (n, C.POINTER(C.c_void_p)) for n in ("Wgate", "bgate", "Wnl", "bnl", "Wlin", "blin")]


class Stage2StepDesc(C.Structure):
    """struct mmf_stage2_step_desc (include/mmf_amil.h)."""
    _fields_ = [(n, C.c_int32) for n in ("family", "train_type", "radio", "path", "omic", "n_layers", "B", "K", "training")] + [
        ("h", C.c_void_p * 3), ("blk", Stage2StepBlock * 3), ("Wk", C.c_void_p), ("bk", C.c_void_p), ("p_drop", C.c_float),
        ("seed", C.c_uint32), ("seed_dev", C.c_void_p), ("trace", C.c_void_p)]


class Stage2Target(C.Structure):
    """struct mmf_stage2_target (include/mmf_amil.h)."""
    _fields_ = [("loss", C.c_int32), ("Y", C.c_void_p), ("c", C.c_void_p), ("times", C.c_void_p), ("alpha", C.c_float),
                ("nll_ratio", C.c_float), ("phi", C.c_int32), ("reduction", C.c_int32), ("loss_scale", C.c_float)]


class Stage2BlockGrads(C.Structure):
    """struct mmf_stage2_block_grads (include/mmf_amil.h): the per-layer members are host arrays of device pointers."""
    _fields_ = [(n, C.c_void_p) for n in ("dW0", "db0", "dbn_weight", "dbn_bias", "dW4", "db4", "dbn1_weight", "dbn1_bias",
                                          "dbn2_weight", "dbn2_bias")] + [
        (n, C.POINTER(C.c_void_p)) for n in ("dWgate", "dbgate", "dWnl", "dbnl", "dWlin", "dblin")]


class Stage2StepGrads(C.Structure):
    """struct mmf_stage2_step_grads (include/mmf_amil.h)."""
    _fields_ = [("blk", Stage2BlockGrads * 3), ("dWk", C.c_void_p), ("dbk", C.c_void_p)]


# name -> (restype, argtypes): every symbol include/mmf_amil.h declares
SYMBOLS = {
    "mmf_strerror": (C.c_char_p, [C.c_int]),
    "mmf_abi_version": (C.c_int, []),
    "mmf_amil_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_amil_forward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_amil_backward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(AmilGrads), C.c_void_p]),
    "mmf_amil_bf16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_amil_bf16_forward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_amil_bf16_backward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(AmilGrads), C.c_void_p]),
    "mmf_amil_head_forward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                        C.POINTER(SurvHead), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_amil_nll_step": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                    C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p, C.POINTER(AmilGrads), C.c_void_p]),
    "mmf_amil_group_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                     C.c_int32]),
    "mmf_amil_nll_step_group": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p, C.POINTER(AmilGrads),
                                          C.c_void_p]),
    "mmf_radio_group_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                      C.c_int32, C.c_int32]),
    "mmf_radio_nll_step_group": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.POINTER(RadioReduce), C.c_void_p,
                                           C.c_size_t, C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p,
                                           C.POINTER(AmilGrads), C.c_void_p]),
    "mmf_surv_head_nll_step": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p,
                                         C.c_void_p]),
    "mmf_amil_group_forward": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mmf_amil_group_backward": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(AmilGrads), C.c_int32, C.c_void_p]),
    "mmf_radio_group_forward": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.POINTER(RadioReduce), C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mmf_radio_group_backward": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.POINTER(RadioReduce), C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(AmilGrads), C.c_int32,
                                           C.c_void_p]),
    "mmf_surv_head_group_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "mmf_surv_head_nll_step_group": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SurvHead),
                                               C.POINTER(NllTarget), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mmf_dropout_row_base": (C.c_uint32, [C.c_uint32]),
    "mmf_dense_forward_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_void_p]),
    "mmf_dense_backward_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "mmf_amil_group_infer_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
                                                           C.c_int32, C.c_int32, C.c_int32]),
    "mmf_amil_infer_group": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_size_t, C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "mmf_amil_ig_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32]),
    "mmf_amil_ig": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SurvHead),
                              C.POINTER(IgDesc), C.c_void_p]),
    "mmf_radio_ig_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_int32]),
    "mmf_radio_ig": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(RadioReduce), C.c_void_p, C.c_size_t, C.POINTER(SurvHead),
                               C.POINTER(IgDesc), C.c_void_p]),
    "mmf_mm_ig_workspace_bytes": (C.c_size_t, [C.c_int64] + [C.c_int32] * 4 + [C.c_int64] + [C.c_int32] * 10),
    "mmf_mm_ig": (C.c_int, [C.POINTER(MmIgDesc), C.c_void_p, C.c_size_t, C.POINTER(SurvHead), C.c_void_p]),
    "mmf_mm_ig_tensor_workspace_bytes": (C.c_size_t, [C.c_int64] + [C.c_int32] * 4 + [C.c_int64] + [C.c_int32] * 15),
    "mmf_mm_ig_tensor": (C.c_int, [C.POINTER(MmIgDesc), C.POINTER(XFusionWeights), C.c_void_p, C.c_size_t,
                                   C.POINTER(SurvHead), C.c_void_p]),
    "mmf_stage2_ig_workspace_bytes": (C.c_size_t, [C.c_int32] * 7),
    "mmf_stage2_ig": (C.c_int, [C.POINTER(Stage2IgDesc), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mmf_stage2_step_workspace_bytes": (C.c_size_t, [C.c_int32] * 7),
    "mmf_stage2_step": (C.c_int, [C.POINTER(Stage2StepDesc), C.POINTER(Stage2Target), C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stage2StepGrads), C.c_int32, C.c_void_p]),
    "mmf_radio_group_infer_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
                                                            C.c_int32, C.c_int32, C.c_int32]),
    "mmf_radio_infer_group": (C.c_int, [C.POINTER(AmilDesc), C.POINTER(BagGroup), C.POINTER(RadioReduce), C.c_void_p,
                                        C.c_size_t, C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "mmf_xfusion_group_infer_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_xfusion_infer_group": (C.c_int, [C.POINTER(XFusionWeights), C.POINTER(C.c_void_p), C.c_int32, C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_xfusion_group_workspace_bytes": (C.c_size_t, [C.c_int32] * 7),
    "mmf_xfusion_group_forward": (C.c_int, [C.POINTER(XFusionWeights), C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "mmf_xfusion_group_backward": (C.c_int, [C.POINTER(XFusionWeights), C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(XFusionGrads), C.c_int32,
                                             C.c_void_p]),
    "mmf_surv_head_infer_group": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                            C.POINTER(SurvHead), C.POINTER(NllTarget), C.c_void_p]),
    "mmf_amil_infer_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_amil_infer": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_amil_bf16_infer_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_amil_bf16_infer": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_attn_net_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_attn_net_forward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mmf_attn_net_backward": (C.c_int, [C.POINTER(AmilDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.POINTER(AmilGrads), C.c_void_p]),
    "mmf_linear_forward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "mmf_linear_forward": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p]),
    "mmf_maxnet_cox_step_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "mmf_maxnet_cox_step": (C.c_int, [C.POINTER(MaxnetDesc), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_void_p, C.POINTER(MaxnetGrads), C.c_int32, C.c_void_p]),
    "mmf_linear_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "mmf_linear_backward": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int64,
                                      C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "mmf_linear_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                        C.POINTER(C.c_void_p), C.c_void_p]),
    "mmf_surv_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_surv_head_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_nll_surv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                               C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_cox_surv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_dropout_keep_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]),
    "mmf_dense_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "mmf_dense_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_gate_mul_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mmf_gate_mul_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p]),
    "mmf_kron_forward": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32,
                                   C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_kron_backward": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32,
                                    C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "mmf_adam_l1_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_void_p]),
    "mmf_abs_sum": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmf_xreduce_forward": (C.c_int, [C.POINTER(XReduceIO), C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mmf_xreduce_backward": (C.c_int, [C.POINTER(XReduceIO), C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mmf_batchnorm_forward": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                                         C.c_float, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5),
    "mmf_batchnorm_backward": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                          C.c_float, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6),
    "mmf_highway_mix_forward": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p]),
    "mmf_highway_mix_backward": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 4),
    "mmf_ranking_loss": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p] * 3),
    "mmf_hazards_forward": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5),
    "mmf_hazards_backward": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mmf_bag_gather": (C.c_int, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mmf_trace_create": (C.c_void_p, [C.c_int32]),
    "mmf_trace_destroy": (None, [C.c_void_p]),
    "mmf_trace_dump": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
}


class KernelTrace:
    """Per-kernel device time of the attention-stack calls made inside the `with` block (include/mmf_amil.h
    "Kernel trace": HIP events on the launch stream).  dump() -> {kernel_name: (launches, total_ms)}."""

    def __init__(self, capacity: int = 4096):
        self.handle = lib().mmf_trace_create(capacity)
        if not self.handle:
            raise MmfError("mmf_trace_create failed")

    def __enter__(self):
        from . import ops
        self._prev = ops.set_trace(self.handle)
        return self

    def __exit__(self, *a):
        from . import ops
        ops.set_trace(self._prev)

    def dump(self):
        l = lib()
        buf = C.create_string_buffer(1 << 16)     # one call: the dump clears the records
        l.mmf_trace_dump(self.handle, buf, 1 << 16)
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            out[name] = (int(cnt), float(ms))
        return out

    def close(self):
        if self.handle:
            lib().mmf_trace_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

_lib = None


class MmfError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libmmf_amil.so once; raise loudly if it is missing (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MmfError(
                f"{LIB_PATH} not found: the HIP extension has not been built. "
                "Run `python -m multimodalfusion_amd.build` (needs hipcc, gfx950 target). "
                "There is no CPU fallback for the attention-MIL path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        v = l.mmf_abi_version()
        if v != ABI_VERSION:
            raise MmfError(f"libmmf_amil.so ABI version {v}, binding expects {ABI_VERSION}: rebuild")
        _lib = l
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = lib().mmf_strerror(code).decode()
        raise MmfError(f"{what} failed: {msg} (code {code})")


def ptr(t):
    """Device pointer of a contiguous fp32/int64/fp64 CUDA(HIP) tensor, or None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MmfError("multimodalfusion_amd ops need tensors on the MI355X (device 'cuda'); "
                       "there is no CPU path -- call model.relocate() / .to('cuda') first")
    if not t.is_contiguous():
        raise MmfError("tensor must be contiguous")
    return t.data_ptr()


def stream_ptr():
    """The raw handle of torch's current HIP stream on the current device.  (torch.cuda.current_stream() builds a Stream
    object and goes through is_available(), which reads the environment: ~5 us a call, twenty calls in a multimodal step.)"""
    import torch
    torch.cuda._lazy_init()
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
