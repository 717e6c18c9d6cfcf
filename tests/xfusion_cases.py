"""Inputs and the float64 oracle of the tensor-fusion tail at any admitted shape (helper module, not collected by pytest):
what tests/test_gpu_xfusion_shapes.py runs on the device and tests/test_abi_shapes_cpu.py checks for ReLU kinks.

Weights: N(0, 1 / fan_in) with bias spread 0.1 (gen.mm_state_dict is fixed to the shipped widths); embeddings v_i ~ N(0, 1);
an upstream gradient for hid; one fusion seed per patient.  Row g of every per-patient input depends on g alone, so that
a patient can be run alone (G = 1) on the same numbers.  The oracle is oracle.torch_port.xfusion + classifier[0] under
torch fp64 autograd, patient by patient with that patient's masks -- _raw_oracle of test_gpu_mm_tensor_group_step.py at
the case's widths."""
import functools

import numpy as np
import torch

from oracle import inputs as gen
from oracle import torch_port as tp
from test_gpu_mm_tensor_group_step import KINK, P_FUS, TAIL_RELU, _raw_names, fusion_masks  # noqa: F401  (re-exported)

ROWS = 64                                    # per-patient inputs are drawn for a full window and cut to G


def state_dict(c):
    """The tail's weights at the case's widths, keyed as the model's state dict; seed: c.seed."""
    m, shapes = c.m, {}
    for i in range(m):
        shapes[f"mm.reduce.{i}.0.0"] = (c.sdim, c.dim)
        shapes[f"mm.reduce.{i}.1.0"] = (c.sdim, m * c.dim)
        shapes[f"mm.reduce.{i}.2.0"] = (c.sdim, c.sdim)
    shapes["mm.encoder1.0"] = (c.mmhid1, c.E)
    shapes["mm.encoder2.0"] = (c.mmhid2, c.K2)
    shapes["classifier.0"] = (c.nhid, c.mmhid2)
    sd = {}
    for s, (k, (n, f)) in enumerate(shapes.items()):
        sd[k + ".weight"] = gen.normal(7000 + c.seed, (n, f), stream=2 * s, std=1.0 / np.sqrt(f))
        sd[k + ".bias"] = gen.normal(7000 + c.seed, (n,), stream=2 * s + 1, std=0.1)
    return sd


def inputs(c):
    """(state dict, [v_i [G x dim]], dhid [G x nhid], fusion seeds [G])."""
    G = max(c.G, 1)
    vs = [gen.normal(31 + i, (ROWS + 1, c.dim), stream=5)[:G] for i in range(c.m)]
    dhid = gen.normal(37, (ROWS + 1, c.nhid), stream=6)[:G]
    seeds = [(2654435761 * (g + 1) + 12345 + 977 * c.seed) & 0xFFFFFFFF for g in range(G)]
    return state_dict(c), vs, dhid, seeds


def weight_list(sd, m):
    """(xfusion's weight order, Wc0, bc0) as numpy arrays."""
    w = []
    for i in range(m):
        for j in range(3):
            w += [sd[f"mm.reduce.{i}.{j}.0.weight"], sd[f"mm.reduce.{i}.{j}.0.bias"]]
    for k in ("mm.encoder1.0", "mm.encoder2.0"):
        w += [sd[k + ".weight"], sd[k + ".bias"]]
    return w, sd["classifier.0.weight"], sd["classifier.0.bias"]


@functools.lru_cache(maxsize=None)
def oracle(c, train):
    """(MM, hid, [dv_i], {weight gradient sums}, smallest |ReLU pre-activation| over every patient and unit) for
    loss = sum hid . dhid; computed once per (case, mode) and left unchanged."""
    sd_np, vs, dhid, seeds = inputs(c)
    sd = tp.to_torch(sd_np, torch.float64)
    tv = [torch.as_tensor(v).double().requires_grad_(True) for v in vs]
    pre, lin = [], tp._lin

    def spy(sd_, name, x):
        y = lin(sd_, name, x)
        if name in TAIL_RELU:
            pre.append(float(y.detach().abs().min()))
        return y

    tp._lin = spy
    try:
        MMs, hids = [], []
        for g in range(c.G):
            mm, cls = fusion_masks(seeds[g], c.m, mmhid1=c.mmhid1, mmhid2=c.mmhid2, nhid=c.nhid) if train else (None, None)
            MM = tp.xfusion(sd, "mm", [v[g:g + 1] for v in tv], mm)
            hid = torch.relu(tp._lin(sd, "classifier.0", MM))
            MMs.append(MM)
            hids.append(hid * cls if train else hid)
    finally:
        tp._lin = lin
    assert len(pre) == c.G * (2 * c.m + 3)              # h_i, o_i per modality, the encoders, classifier[0]: no unit excused
    MM, hid = torch.cat(MMs), torch.cat(hids)
    (hid * torch.as_tensor(dhid).double()).sum().backward()
    return (MM.detach().numpy(), hid.detach().numpy(), [v.grad.numpy() for v in tv],
            {k: sd[k].grad.numpy() for k in _raw_names(c.m)}, min(pre))
