"""Inputs, float64 references and the C-ABI calls of the RADIO and HALF tables of tests/abi_shapes.py (helper module, not
collected by pytest): the radiology window (mmf_radio_nll_step_group, mmf_radio_infer_group) and the grouped half chains
(mmf_amil_group_forward / _backward, mmf_radio_group_forward / _backward) at stacks other than the shipped `small` one.

  * bag_metas(c): one oracle `meta` record per bag of a case -- oracle/cases.py radio_inputs / run_radio with an explicit
    size = (L, H, D); bag g has its own rows (x_seed) and its own hash masks (mask_seed, which the GPU file passes as the
    bag's dropout seed).
  * full_reference(c): per bag cases.run_radio in float64; the summed gradients sum_g loss_scale * grads_g.
  * half_reference(c): M_g and A_raw of the same float64 forward; with the fixed random dM [G x H] of half_dm(c) the
    float64 autograd gradients of sum_g <dM_g, M_g> with respect to every stack parameter and reduce_dim.
  * kink_units(c): relu_kink_units (tests/test_gpu_path.py) on the float64 reduce_dim output of every row of the window.
    The seeds the tables record were chosen, on the CPU and from this function alone, so that no case has any such unit:
    every gradient is then held to the tight bar.  tests/test_radio_shapes_cpu.py asserts it on these arrays.
  * entry_calls(...): the six entry points on one set of pointers -- fake ones and a zero-byte workspace on the CPU, where
    an admitted shape stops at MMF_ERR_WORKSPACE before any launch; device pointers on the GPU, for the refused cases.
"""
import ctypes as C
import functools

import numpy as np
import torch

import abi_shapes as ab
from oracle import cases
from oracle import torch_port as tp

K, ALPHA, P_DROP = 4, 0.3, 0.25
PREFIX = "attention_net_radio"
OUT_BAR = 1e-5                    # the project's bar between two fp32 routes of the same forward (outputs of unit scale)
KINK_THR = 4e-6                   # tests/test_gpu_path.py relu_kink_units


def n_mod(c):
    return c.nseg or 1


def bag_metas(c):
    base = dict(gated=c.gated, n_mod=n_mod(c), K=K, dropout=c.train, alpha=ALPHA, bias_std=0.05, train=c.train, seed=c.seed,
                size=c.size)
    return [dict(base, n=n, x_seed=510 + 101 * g, mask_seed=910 + 7 * g, y=(g + 1) % K, c=g % 2) for g, n in enumerate(c.sizes)]


def loss_scale(c):
    return 1.0 / len(c.sizes)


@functools.lru_cache(maxsize=None)
def state(c):
    """The state dict of a case (numpy fp32): reduce_dim (radio), attention_net_radio.*, classifier."""
    return cases.radio_inputs(dict(bag_metas(c)[0], n=1))[0]


@functools.lru_cache(maxsize=None)
def window(c):
    """The modality matrices of a case: n_mod arrays [sum N x L], the bags' rows in order."""
    per_bag = [cases.radio_inputs(m)[1] for m in bag_metas(c)]
    return [np.concatenate([xs[i] for xs in per_bag]) for i in range(n_mod(c))]


def stack_names(c):
    """State-dict names of (W1, b1, Wa, ba, Wb, bb, Wc, bc); None for an ungated Wb, bb."""
    p = PREFIX
    if c.gated:
        mid = [f"{p}.3.attention_a.0", f"{p}.3.attention_b.0", f"{p}.3.attention_c"]
    else:
        mid = [f"{p}.3.module.0", None, f"{p}.3.module.{3 if c.train else 2}"]
    names = []
    for m in [f"{p}.0"] + mid:
        names += [None, None] if m is None else [m + ".weight", m + ".bias"]
    return names


def grad_names(c):
    """The order of ops.radio_nll_step_group's gradient list: reduce_dim, the stack, the classifier."""
    return ["reduce_dim.weight", "reduce_dim.bias"] + stack_names(c) + ["classifier.weight", "classifier.bias"]


def reduce_dim_output(c):
    """reduce_dim's float64 output over the window's rows (the stack's input); the rows themselves without reduce_dim."""
    sd, xs = state(c), window(c)
    if n_mod(c) == 1:
        return np.asarray(xs[0], np.float64)
    return np.concatenate([np.asarray(x, np.float64) for x in xs], 1) @ np.asarray(sd["reduce_dim.weight"], np.float64).T \
        + np.asarray(sd["reduce_dim.bias"], np.float64)


def kink_units(c, thr=KINK_THR):
    """tests/test_gpu_path.py relu_kink_units on reduce_dim_output(c): hidden units of the stack's first layer with a
    float64 pre-activation within fp32 rounding of zero for some row of the window."""
    u = reduce_dim_output(c) @ np.asarray(state(c)[PREFIX + ".0.weight"], np.float64).T \
        + np.asarray(state(c)[PREFIX + ".0.bias"], np.float64)
    return set(np.nonzero((np.abs(u) < thr).any(axis=0))[0].tolist())


def before(c, name, shape):
    """The non-zero values an accumulate case's gradient buffer starts from."""
    i = sorted(n for n in grad_names(c) if n).index(name)
    return (0.25 + 0.01 * i + 0.5 * np.cos(np.arange(int(np.prod(shape)), dtype=np.float64) * 0.37 + i)).reshape(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def full_reference(c):
    """(per-bag results of cases.run_radio in float64, {name: sum_g loss_scale * grad_g})."""
    refs = [cases.run_radio(m) for m in bag_metas(c)]
    s = loss_scale(c)
    gsum = {k: sum(s * r["grads"][k] for r in refs) for k in refs[0]["grads"]}
    return refs, gsum


def half_dm(c):
    """The fixed random dM [G x H] of a half case, fp32."""
    from oracle import inputs as gen
    return gen.normal(7000 + c.seed, (len(c.sizes), c.H), stream=3, std=1.0)


@functools.lru_cache(maxsize=None)
def half_reference(c):
    """(M [G x H], [A_raw_g [1 x N_g]], {name: d sum_g <dM_g, M_g> / d parameter}) in float64."""
    sd = tp.to_torch({k: v for k, v in state(c).items() if not k.startswith("classifier")}, torch.float64)
    dM = torch.as_tensor(half_dm(c)).double()
    Ms, As, total = [], [], 0.0
    for g, m in enumerate(bag_metas(c)):
        _, xs, masks = cases.radio_inputs(m)
        tm = {k: torch.as_tensor(v).double() for k, v in masks.items()} if masks else None
        h = torch.cat([torch.as_tensor(x).double() for x in xs], 1)
        if n_mod(c) > 1:
            h = torch.nn.functional.linear(h, sd["reduce_dim.weight"], sd["reduce_dim.bias"])
        M, A_raw = tp.amil_pool(sd, PREFIX, h, c.gated, c.train, tm)
        total = total + (dM[g:g + 1] * M).sum()
        Ms.append(M.detach().numpy())
        As.append(A_raw.detach().numpy())
    grads = {k: v.detach().numpy() for k, v in tp.grads_of(total, sd).items()}
    return np.concatenate(Ms), As, grads


def grad_bar(ref):
    """1e-5 + 1e-4 max|ref|: compare()'s gradient bar, and the one test_attn_net and check_group hold reduce_dim to."""
    return 1e-5 + 1e-4 * float(np.abs(ref).max())


# ---- the six entry points on one set of pointers ---------------------------------------------------------------------------
PTRS = ("W1", "b1", "Wa", "ba", "Wb", "bb", "Wc", "bc", "dW1", "db1", "dWa", "dba", "dWb", "dbb", "dWc", "dbc", "Wk", "bk",
        "logits", "hazards", "S", "Y_hat", "risk", "Y", "c", "loss", "dWk", "dbk", "W", "bias", "dW", "db", "M", "dM", "A_raw",
        "ws", "x0", "x1", "x2", "x3", "x4")
RADIO_ENTRIES = ("mmf_radio_nll_step_group", "mmf_radio_infer_group", "mmf_radio_group_forward", "mmf_radio_group_backward")
PLAIN_ENTRIES = ("mmf_amil_group_forward", "mmf_amil_group_backward")
WRITES_GRADS = {"mmf_radio_nll_step_group": True, "mmf_radio_infer_group": False, "mmf_radio_group_forward": False,
                "mmf_radio_group_backward": True, "mmf_amil_group_forward": False, "mmf_amil_group_backward": True}


def fake_pointers():
    """Pointer values for calls that must return before any pointer is read: 16-byte aligned, never dereferenced."""
    return {n: 0x100000 + 0x10000 * i for i, n in enumerate(PTRS)}


def entry_calls(m, l, c, p, sizes=None, ws_bytes=0, ldm=None, train=True, accumulate=0, stream=None, seeds=None, sync=None,
                entries=None):
    """Return codes of the radio entry points (c.nseg != 0; all four, or `entries`) or of the plain half pair (c.nseg == 0)
    for case c (a Radio or a Half) on the pointers p ({name of PTRS: address}); misalignments of the case (c.misalign:
    "segment", "W", "dW", "dM") are applied to them here.  sizes: the window, default c.sizes."""
    sizes = tuple(c.sizes if sizes is None else sizes)
    G, R = len(sizes), sum(sizes)
    off = lambda name, what: p[name] + (4 if c.misalign == what else 0)
    p_drop = P_DROP if train else 0.0

    def desc(p_h, p_att):
        return m.AmilDesc(N=R, L=c.L, H=c.H, D=c.D, gated=1 if c.gated else 0, W1=p["W1"], b1=p["b1"], Wa=p["Wa"], ba=p["ba"],
                          Wb=p["Wb"] if c.gated else None, bb=p["bb"] if c.gated else None, Wc=p["Wc"], bc=p["bc"], p_h=p_h,
                          p_att=p_att, seed=0, seed_dev=None, trace=None, concurrent=0, gemm=0, sync=sync,
                          sync_words=0 if sync is None else 1024)     # ops.SYNC_WORDS: the tick words ops.py passes
    offs = (C.c_int64 * (G + 1))(*np.concatenate([[0], np.cumsum(sizes)]).tolist())
    sd = (C.c_uint32 * G)(*(seeds if seeds is not None else range(1, G + 1)))
    grp = m.BagGroup(G=G, offsets=offs, seeds=sd)
    head = m.SurvHead(Wk=p["Wk"], bk=p["bk"], K=K, logits=p["logits"], hazards=p["hazards"], S=p["S"], Y_hat=p["Y_hat"],
                      risk=p["risk"])
    tgt = m.NllTarget(Y=p["Y"], c=p["c"], alpha=ALPHA, eps=1e-7, loss_scale=1.0 / G, loss=p["loss"], dWk=p["dWk"], dbk=p["dbk"],
                      accumulate=accumulate)
    g = m.AmilGrads(dW1=p["dW1"], db1=p["db1"], dWa=p["dWa"], dba=p["dba"], dWb=p["dWb"] if c.gated else None,
                    dbb=p["dbb"] if c.gated else None, dWc=p["dWc"], dbc=p["dbc"], dx=None)
    by, ws = C.byref, p["ws"]
    ldm = c.H if ldm is None else ldm
    dM = off("dM", "dM")
    d_train, d_eval = desc(p_drop, p_drop), desc(0.0, 0.0)
    if not c.nseg:
        calls = {"mmf_amil_group_forward": lambda: l.mmf_amil_group_forward(by(d_train), by(grp), p["x0"], ws, ws_bytes, p["M"], ldm,
                                                                            p["A_raw"], stream),
                 "mmf_amil_group_backward": lambda: l.mmf_amil_group_backward(by(d_train), by(grp), p["x0"], ws, ws_bytes, dM, ldm,
                                                                              p["A_raw"], by(g), accumulate, stream)}
    else:
        n = max(c.nseg, 1)
        xs = [p[f"x{i}"] for i in range(n)]
        if c.misalign == "segment":
            xs[1] += 4
        arr = (C.c_void_p * n)(*xs)
        rd = m.RadioReduce(x=C.cast(arr, C.POINTER(C.c_void_p)), nseg=c.nseg, kseg=c.kseg, W=off("W", "W"), bias=p["bias"],
                           dW=off("dW", "dW"), db=p["db"])
        calls = {"mmf_radio_nll_step_group": lambda: l.mmf_radio_nll_step_group(by(d_train), by(grp), by(rd), ws, ws_bytes, by(head),
                                                                                by(tgt), p["A_raw"], by(g), stream),
                 "mmf_radio_infer_group": lambda: l.mmf_radio_infer_group(by(d_eval), by(grp), by(rd), ws, ws_bytes, by(head), by(tgt),
                                                                          p["M"], p["A_raw"], stream),
                 "mmf_radio_group_forward": lambda: l.mmf_radio_group_forward(by(d_train), by(grp), by(rd), ws, ws_bytes, p["M"], ldm,
                                                                              p["A_raw"], stream),
                 "mmf_radio_group_backward": lambda: l.mmf_radio_group_backward(by(d_train), by(grp), by(rd), ws, ws_bytes, dM, ldm,
                                                                                p["A_raw"], by(g), accumulate, stream)}
    return {name: f() for name, f in calls.items() if entries is None or name in entries}

