"""Cases, float64 oracle and error bars of the multimodal tensor-fusion head's integrated-gradients tests (helper module,
not collected by pytest), on top of tests/mm_ig_cases.py (imported, not edited).  tests/test_mm_tensor_ig_cases_cpu.py
checks the input conditions and the caps on these very arrays; tests/test_gpu_mm_tensor_ig.py runs the kernels on them.

Weights.  Tiers A: oracle.inputs._linear / _attn_stack under the model's key names -- fc_omic, attention_net_radio,
reduce_dim, attention_net_WSI as in mm_ig_cases, then mm.reduce.{i}.{0,1,2}.0, mm.encoder1.0, mm.encoder2.0, classifier.0,
classifier.3 -- xavier, bias_std = 0.1 everywhere.  Tier C: oracle.inputs.mm_state_dict(fusion = "tensor", bias_std = 0.1),
the shipped widths, which the model loads.  Inputs: mm_ig_cases.draw.

Oracle.  Integrated gradients by the definition: for every node alpha_k (the fp32 value the kernels get) one autograd pass
in float64 over oracle.torch_port.mm_forward(..., fusion = "tensor") on alpha_k * every input, risk = -sum(S), attr = input
* sum_k w_k d risk / d(alpha_k input).  Computed once per case (lru_cache) and never modified.

Stack and omic kinks are flagged as mm_ig_cases flags them (the bounds do not depend on what follows the embedding).  The
small cases are kink-free there by redraw (mm_ig_cases' tier A rule); tier C carries mm_ig_cases' allowance, with d risk /
d embedding taken through the tail.

Tail kinks -- the ReLUs at h_i, o_i, e1 (encoder1), e2 (encoder2) and c0 (classifier[0]).  A tail unit near 0 changes every
attribution at its node, so no allowance: a unit is FLAGGED at a node when its float64 pre-activation lies within BOUND of 0,
and for a node with f flagged units the oracle holds the node's contribution under all 2^f assignments of those units'
derivatives (recomputed with the ReLU's mask forced to 0 or 1: y = u * mask, so the forward value moves by at most |u| <=
BOUND).  The GPU result must lie within the plain bar -- 1e-4 * max|oracle| per array, 1e-4 on the risks -- of ONE
combination of per-node assignments, the same for every array of the call (match).  Caps, conditions on the committed seeds
and never to be changed: at most NODE_CAP = 3 flagged tail units per node and CASE_CAP = 10 per case.

BOUND: the local summation error of the kernel that forms the unit, d 2^-24 (sum |w x| + |b|) with d the number of dependent
roundings on the longest path through its code -- a worst case, no cancellation assumed -- plus the error of its inputs
carried through W.  From the code (csrc/mmf_mlp.hip, csrc/mmf_xfusion_ig.hip), with it = ceil(dim / 256):
  h_i   xgate_group_kernel: wave_dot adds per lane it groups of four products (product, three additions, the accumulator:
        it + 4), the butterfly 6, the bias 1                                                  d = it + 11, + 2 slack
  z_i   the same over m partial dots added before the butterfly                               d = it + 11 + m, + 2
  gm    sigmoid(z) h: d gm = (dz / 4 + 4 2^-24) |h| + dh + 2^-24 |gm| (expf one ulp, the division, the product)
  o_i   the bias, then 16 products added in order                                              d = 17, + 2
  e1    kron_dense_group_kernel: 17 products in order, the outer factor (two products at m = 3), NQ = ceil(17^(m-1) / 64)
        partial sums, the butterfly 6, the bias                                                d = 26 + NQ, + 2
        its input is the product kr = o'_0 x o'_1 (x o'_2), o' = [o, 1]: d kr = sum_t do'_t prod_{s != t} |o'_s|
  e2    dense_segs_group_kernel: ceil(K2 / 64) products into four accumulators in turn, two additions to join them, the
        butterfly 6, the bias                                                                  d = ceil(ceil(K2 / 64) / 4) + 10, + 2
  c0    xfusion_ig_head_kernel: ceil(mmhid2 / 64) fused multiply-adds per lane, the butterfly 6, the bias
                                                                                               d = ceil(mmhid2 / 64) + 7, + 2
A ReLU passes its input's error on unchanged.
How the input error is carried (carry): in squares, sqrt(sum_k W_k^2 d_k^2) -- the errors of different inputs taken as
independent, as the probabilistic rounding analyses do -- not as sum_k |W_k| d_k.  The absolute form does not
serve: through five layers every |W| multiplies the error by the layer's loss of cancellation (10 to 16 here), the bound
at classifier[0] reaches 1e-3 of sum |w x|, 4 to 300 tail units are flagged at one node in every one of the ten cases as drawn (the shipped
tail over 20), which no change of seed brings under the caps; the float32 forward below stays under 2 % of it at the first layer and 0.05 % at the last.  In squares the
same float32 forward stays under 11 % of BOUND at every unit of every case (the figure the CPU test prints), and the draws
flag 0 to 5 units per case.
The embeddings' own error dv is the one input the tail's code does not show.  Omic: mm_ig_cases.omic_bounds' second-layer
bound through SELU's largest slope.  A stack, M_j = sum_i p_i h_ij: the projection's error e_ij -- the chain depths of
mm_ig_cases.path_bound / radio_ig_cases.kink_bound, the terms added in squares (projection_error, radio_projection_error) --
averaged under the weights in squares, plus A 2^-24 sum_i p_i |h_ij| with A = (H / 2 + 8) + (D / 64 + 8) + 16 +
(ceil(N / 64) + 8): the gate GEMM's chain, the scorer's, the ulps of tanh, sigmoid and exp, and the pooling's, each stage's
rounding taken once relative to the sum it feeds.
So BOUND is a derived estimate with a measured margin, not a proof: tests/test_mm_tensor_ig_cases_cpu.py holds it against a
float32 evaluation of the same forward on the CPU at every unit of every case and node -- if that fails, it is too small.

Bars: mm_ig_cases' -- 1e-4 * max|oracle| per array (plus the stack / omic allowance in tier C), 1e-4 per risk."""
import collections
import functools
import itertools

import numpy as np
import torch

import mm_ig_cases as mc
import radio_ig_cases as rc
from oracle import inputs as gen
from oracle import torch_port as tp

U = mc.U
NODE_CAP, CASE_CAP = 3, 10
PRE_P, PRE_R = mc.PRE_P, mc.PRE_R
SLOPE = mc.SELU_SCALE * mc.SELU_ALPHA

Tail = collections.namedtuple("Tail", "mmhid1 mmhid2 nhid")
Case = collections.namedtuple("Case", mc.Case._fields + ("tail",))


def _c(name, tier, mode, tail, path=None, radio=None, omic=None, **kw):
    return Case(*mc._c(name, tier, mode, path, radio, omic, **kw), Tail(*tail))


TIER_A = [
    # the model's tail but for a narrower encoder2: dim 256, mmhid1 512, mmhid2 256, nhid 256, m = 3
    _c("t_rpo_shipped_tail", "A", "radio_path_omic", (512, 256, 256), (32, 256, 256, True, 65), (4, 32, 256, 256, True, 17),
       (80, 256, 256), seed=31),
    # mixed gates; the scalar remainders of the tail's widths
    _c("t_rp_remainders_k1", "A", "radio_path", (100, 7, 6), (32, 256, 256, False, 300), (2, 32, 256, 256, True, 33), K=1),
    # omic first in the row; a second dkr pass of 4 rows
    _c("t_po_omic_first_k32", "A", "path_omic", (516, 40, 40), (32, 256, 128, True, 33), None, (7, 33, 256), K=32),
    # one row per sequence, three sequences
    _c("t_ro_one_row", "A", "radio_omic", (64, 32, 32), None, (3, 32, 256, 128, True, 1), (36, 64, 256)),
    # the widest admitted row: K2 = 512 + 2 * 512 = 1536
    _c("t_rp_widest_row", "A", "radio_path", (512, 48, 24), (32, 512, 128, True, 17), (2, 32, 512, 128, False, 17), n_steps=4,
       method="riemann_middle"),
    # S = 64, the riders alone in the last window
    _c("t_rp_riders_alone", "A", "radio_path", (64, 32, 32), (32, 256, 128, False, 17), (2, 32, 256, 128, False, 17), n_steps=64,
       window_steps=64),
    # one patient past the dkr launch's group of 16
    _c("t_po_window_17", "A", "path_omic", (64, 32, 32), (32, 256, 128, True, 17), None, (7, 33, 256), window_steps=17),
    _c("t_po_one_step_windows", "A", "path_omic", (64, 32, 32), (32, 256, 128, True, 17), None, (7, 33, 256), n_steps=1,
       method="riemann_middle", window_steps=1),
]
TIER_C = [
    _c("tc_rpo_small_gated", "C", "radio_path_omic", (512, 512, 256), (1024, 256, 256, True, 150), (4, 1024, 256, 256, True, 33),
       (80, 256, 256)),
    _c("tc_po_small_ungated", "C", "path_omic", (512, 512, 256), (1024, 256, 256, False, 33), None, (80, 256, 256), n_steps=4,
       method="riemann_middle"),
]
CASES = TIER_A + TIER_C
BY_NAME = {c.name: c for c in CASES}
order, quadrature = mc.order, mc.quadrature


def dim(c):
    w = {v for v in mc.widths(c).values() if v}
    assert len(w) == 1, w
    return w.pop()


def state_dict(c):
    m, d = len(order(c.mode)), dim(c)
    if c.tier == "C":
        assert c.tail == Tail(512, 512, 256) and d == 256
        return gen.mm_state_dict(seed=c.seed, input_dim=80, fusion="tensor", gate_path=c.path.gated,
                                 gate_radio=c.radio.gated if c.radio else True, dropout=False, n_classes=c.K, mode=c.mode,
                                 n_mod=4, bias_std=mc.BIAS_STD)
    sd, st = collections.OrderedDict(), 0
    lin = lambda name, n, k: gen._linear(sd, name, n, k, c.seed, st, "xavier", mc.BIAS_STD)
    if c.omic:
        st = lin("fc_omic.0.0", c.omic.W0, c.omic.Gin)
        st = lin("fc_omic.1.0", c.omic.We, c.omic.W0)
    if c.radio:
        r = c.radio
        st = gen._attn_stack(sd, PRE_R, (r.kseg, r.H, r.D), r.gated, False, c.seed, st, "xavier", mc.BIAS_STD)
        st = lin("reduce_dim", r.kseg, r.kseg * r.nseg)
    if c.path:
        p = c.path
        st = gen._attn_stack(sd, PRE_P, (p.L, p.H, p.D), p.gated, False, c.seed, st, "xavier", mc.BIAS_STD)
    for i in range(m):
        st = lin(f"mm.reduce.{i}.0.0", 16, d)
        st = lin(f"mm.reduce.{i}.1.0", 16, d * m)
        st = lin(f"mm.reduce.{i}.2.0", 16, 16)
    st = lin("mm.encoder1.0", c.tail.mmhid1, 17 ** m)
    st = lin("mm.encoder2.0", c.tail.mmhid2, c.tail.mmhid1 + d * m)
    st = lin("classifier.0", c.tail.nhid, c.tail.mmhid2)
    lin("classifier.3", c.K, c.tail.nhid)
    return sd


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(state dict, {branch: fp32 read-only array}, redraw rounds): mm_ig_cases.inputs' rule -- tier A is redrawn until no
    stack or omic unit is flagged."""
    c = BY_NAME[name]
    sd = state_dict(c)
    xs = {k: v.copy() for k, v in mc.draw(c, 0).items()}
    rounds = 0
    if c.tier == "A":
        alphas = quadrature(c)[0]
        while True:
            f = mc.flagged(c, sd, xs, alphas)
            bad_p = f["path"].any(axis=1) if c.path else np.zeros(0, bool)
            bad_r = f["radio"].any(axis=1) if c.radio else np.zeros(0, bool)
            bad_o = bool(c.omic) and bool(f["omic"][0].any() or f["omic"][1].any())
            if not (bad_p.any() or bad_r.any() or bad_o):
                break
            rounds += 1
            assert rounds <= mc.MAX_ROUNDS, (name, rounds)
            nxt = mc.draw(c, rounds)
            if bad_p.any():
                xs["path"][bad_p] = nxt["path"][bad_p]
            if bad_r.any():
                xs["radio"][:, bad_r] = nxt["radio"][:, bad_r]
            if bad_o:
                xs["omic"] = nxt["omic"].copy()
    for v in xs.values():
        v.setflags(write=False)
    return sd, xs, rounds


# ---- the forward, cut where the tests need it ---------------------------------------------------------------------------
def _stack_tail(sdt, pre, h, gated):
    A, _ = tp.attn_net(sdt, pre + ".3", h, gated, False, None)
    p = torch.softmax(A.T, dim=1)
    return p @ h, p


def embeddings(c, sdt, t, leaves=False):
    """{branch: [1 x dim] embedding} of mm_forward's branches on {branch: tensor(s)}, and what the bounds and the cut need:
    {path / radio: (u, h, p), omic: (z1, h1, z2)}.  leaves: the activations h (omic: h1, and O) are detached leaves."""
    emb, mid = {}, {}
    leaf = (lambda x: x.detach().requires_grad_()) if leaves else (lambda x: x)
    if c.radio:
        u = tp._lin(sdt, PRE_R + ".0", tp._lin(sdt, "reduce_dim", torch.cat(list(t["radio"]), dim=1)))
        h = leaf(torch.relu(u))
        emb["radio"], p = _stack_tail(sdt, PRE_R, h, c.radio.gated)
        mid["radio"] = (u, h, p)
    if c.path:
        u = tp._lin(sdt, PRE_P + ".0", t["path"])
        h = leaf(torch.relu(u))
        emb["path"], p = _stack_tail(sdt, PRE_P, h, c.path.gated)
        mid["path"] = (u, h, p)
    if c.omic:
        z1 = tp._lin(sdt, "fc_omic.0.0", t["omic"].unsqueeze(0))
        h1 = leaf(torch.nn.functional.selu(z1))
        z2 = tp._lin(sdt, "fc_omic.1.0", h1)
        O = torch.nn.functional.selu(z2)               # differentiated as it stands: h1 reaches the risk through it
        emb["omic"] = O
        mid["omic"] = (z1, h1, z2, O)
    return emb, mid


def tail(c, sdt, emb, force=None):
    """The XlinearFusion block, classifier[0] and classifier[3] on the embeddings (oracle.torch_port.xfusion / mm_forward's
    arithmetic), every ReLU as y = u * mask with mask = [u > 0] but where force = {(layer, unit): 0 or 1} says otherwise.
    Returns (logits, {layer: pre-activation [n]}, {what the bounds need})."""
    pre, force = {}, force or {}

    def relu(u, key):
        m = (u > 0).to(u.dtype)
        for (lay, j), bit in force.items():
            if lay == key:
                m[0, j] = bit
        pre[key] = u
        return u * m

    vs = [emb[b] for b in order(c.mode)]
    v_cat = torch.cat(vs, dim=1)
    os_, keep = [], {}
    for i, v in enumerate(vs):
        h = relu(tp._lin(sdt, f"mm.reduce.{i}.0.0", v), f"h{i}")
        z = tp._lin(sdt, f"mm.reduce.{i}.1.0", v_cat)
        gm = torch.sigmoid(z) * h
        o = relu(tp._lin(sdt, f"mm.reduce.{i}.2.0", gm), f"o{i}")
        keep[f"z{i}"], keep[f"hh{i}"], keep[f"gm{i}"], keep[f"oo{i}"] = z, h, gm, o
        os_.append(torch.cat((o, torch.ones(1, 1, dtype=o.dtype)), 1))
    kr = os_[0]
    for o in os_[1:]:
        kr = torch.bmm(kr.unsqueeze(2), o.unsqueeze(1)).flatten(start_dim=1)
    e1 = relu(tp._lin(sdt, "mm.encoder1.0", kr), "e1")
    x2 = torch.cat([e1] + vs, dim=1)
    MM = relu(tp._lin(sdt, "mm.encoder2.0", x2), "e2")
    hid = relu(tp._lin(sdt, "classifier.0", MM), "c0")
    keep.update(kr=kr, e1=e1, x2=x2, MM=MM, hid=hid)
    return tp._lin(sdt, "classifier.3", hid), pre, keep


def _risk(logits):
    return -tp.surv_head(logits)[1].sum()


def _f(sd, k):
    return np.asarray(sd[k], np.float64)


def _n(t):
    return t.detach().numpy().astype(np.float64).reshape(-1)


# ---- the bound ------------------------------------------------------------------------------------------------------------
def _rms(X, W):
    return np.sqrt((X * X) @ (W * W).T)


def projection_error(sd, x, a):
    """[N x H]: one standard deviation of the fp32 pre-activation a x W1^T + b1 of the pathology stack under independent
    roundings -- mm_ig_cases.path_bound's chain of L / 2 + 8, its terms added in squares."""
    W1, b1 = _f(sd, PRE_P + ".0.weight"), _f(sd, PRE_P + ".0.bias")
    x = np.asarray(x, np.float64)
    return np.sqrt(x.shape[1] // 2 + 8) * U * np.sqrt((a * _rms(x, W1)) ** 2 + b1 ** 2)


def radio_projection_error(f, a):
    """[N x H]: the same for the radiology stack behind reduce_dim -- radio_ig_cases.kink_bound's three terms, the two
    GEMMs' in squares (reduce_dim's error carried through W1 in squares), the composed bias's as it stands."""
    nk, L = f.X.shape[1], f.W1.shape[1]
    dy = np.sqrt(nk // 2 + 8) * U * _rms(f.X, f.Wr)
    bias = np.abs(f.W1) @ np.abs(f.br) + np.abs(f.b1)
    return a * (_rms(dy, f.W1) + np.sqrt(L // 2 + 8) * U * _rms(f.y, f.W1)) + (rc.bias_chain(L) + 8) * U * bias[None, :]


def embedding_error(c, sd, xs32, a, mid, fr=None):
    """{branch: dv [dim]} at node a (module docstring); mid: embeddings' second result in float64."""
    out = {}
    for b in order(c.mode):
        if b == "omic":
            _, _, _, e2 = mc.omic_bounds(sd, xs32["omic"], a)
            O = _n(mid["omic"][3])
            out[b] = SLOPE * e2 + 4 * U * (np.abs(O) + SLOPE)
            continue
        s = c.path if b == "path" else c.radio
        u, h, p = (t.detach().numpy() for t in mid[b])
        e = projection_error(sd, xs32["path"], a) if b == "path" else radio_projection_error(fr, a)
        A = (s.H // 2 + 8) + (s.D // 64 + 8) + 16 + ((s.N + 63) // 64 + 8)
        out[b] = np.sqrt((p * p) @ (e * e)).reshape(-1) + A * U * (p @ np.abs(h)).reshape(-1)
    return out


def carry(W, d):
    """The error d of a layer's inputs behind its weights W, in squares (module docstring)."""
    return np.sqrt((W * W) @ (d * d))


def tail_bounds(c, sd, emb, dv, keep):
    """{layer: BOUND [n]} for the pre-activations tail() returns, from float64 values (emb, keep as numpy) and the embeddings'
    error dv {branch: [dim]}."""
    m, d = len(order(c.mode)), dim(c)
    it = (d + 255) // 256
    v = np.concatenate([emb[b] for b in order(c.mode)])
    dvc = np.concatenate([dv[b] for b in order(c.mode)])
    out, do = {}, []
    for i, b in enumerate(order(c.mode)):
        Wh, bh = _f(sd, f"mm.reduce.{i}.0.0.weight"), _f(sd, f"mm.reduce.{i}.0.0.bias")
        Wz, bz = _f(sd, f"mm.reduce.{i}.1.0.weight"), _f(sd, f"mm.reduce.{i}.1.0.bias")
        Wo, bo = _f(sd, f"mm.reduce.{i}.2.0.weight"), _f(sd, f"mm.reduce.{i}.2.0.bias")
        out[f"h{i}"] = (it + 13) * U * (np.abs(Wh) @ np.abs(emb[b]) + np.abs(bh)) + carry(Wh, dv[b])
        dz = (it + 13 + m) * U * (np.abs(Wz) @ np.abs(v) + np.abs(bz)) + carry(Wz, dvc)
        h, gm = keep[f"hh{i}"], keep[f"gm{i}"]
        dgm = (dz / 4 + 4 * U) * np.abs(h) + out[f"h{i}"] + U * np.abs(gm)
        out[f"o{i}"] = 19 * U * (np.abs(Wo) @ np.abs(gm) + np.abs(bo)) + carry(Wo, dgm)
        do.append(np.append(out[f"o{i}"], 0.0))
    op = [np.append(keep[f"oo{i}"], 1.0) for i in range(m)]
    dkr = np.zeros(17 ** m)
    for t in range(m):
        term = np.ones(1)
        for s in range(m):
            term = np.outer(term, do[s] if s == t else np.abs(op[s])).reshape(-1)
        dkr += term
    NQ = (17 ** (m - 1) + 63) // 64
    W, bb = _f(sd, "mm.encoder1.0.weight"), _f(sd, "mm.encoder1.0.bias")
    out["e1"] = (28 + NQ) * U * (np.abs(W) @ np.abs(keep["kr"]) + np.abs(bb)) + carry(W, dkr)
    W, bb = _f(sd, "mm.encoder2.0.weight"), _f(sd, "mm.encoder2.0.bias")
    K2 = W.shape[1]
    out["e2"] = (((K2 + 63) // 64 + 3) // 4 + 12) * U * (np.abs(W) @ np.abs(keep["x2"]) + np.abs(bb)) \
        + carry(W, np.concatenate([out["e1"], dvc]))
    W, bb = _f(sd, "classifier.0.weight"), _f(sd, "classifier.0.bias")
    out["c0"] = ((W.shape[1] + 63) // 64 + 9) * U * (np.abs(W) @ np.abs(keep["MM"]) + np.abs(bb)) + carry(W, out["e2"])
    return out


LAYERS = lambda m: [f"h{i}" for i in range(m)] + [f"o{i}" for i in range(m)] + ["e1", "e2", "c0"]


def node_tail(c, sd, sdt, xs32, xs, a, fr):
    """At node a: (risk, {layer: pre [n]}, {layer: BOUND [n]}, the flagged units [(layer, unit)])."""
    scale = lambda t: [x * a for x in t] if isinstance(t, list) else t * a
    with torch.no_grad():
        emb, mid = embeddings(c, sdt, {b: scale(v) for b, v in xs.items()})
        logits, pre, keep = tail(c, sdt, emb)
    dv = embedding_error(c, sd, xs32, a, mid, fr)
    bounds = tail_bounds(c, sd, {b: _n(v) for b, v in emb.items()}, dv, {k: _n(v) for k, v in keep.items()})
    pre = {k: _n(v) for k, v in pre.items()}
    flagged = [(lay, int(j)) for lay in LAYERS(len(emb)) for j in np.nonzero(np.abs(pre[lay]) <= bounds[lay])[0]]
    return float(_risk(logits)), pre, bounds, flagged


# ---- the oracle --------------------------------------------------------------------------------------------------------------
Oracle = collections.namedtuple("Oracle", "attr alt row_sum row_abs mod_abs total total_abs risk risk_base step_risk hazards S "
                                          "Y_hat logits flagged allow allow_max allow_rowmax bar_attr bar_row")


def _split(c, prod):
    attr, k = {}, 0
    for b in order(c.mode):
        n = c.radio.nseg if b == "radio" else 1
        attr[b] = np.stack(prod[k:k + n]) if b == "radio" else prod[k]
        k += n
    return attr


@functools.lru_cache(maxsize=None)
def oracle(name):
    """attr {branch: array} by the definition; alt: for every node with flagged tail units, [(node, [(assignment, {branch:
    what the node's term adds to attr under it, minus its term under float64's own assignment})])]; flagged {node:
    [(layer, unit)]} (nodes n and n + 1 are the riders alpha = 1 and 0, which carry no term); the sums, the risks, the head at
    alpha = 1; the stack / omic allowance (tier C; zero in tier A) and the bars."""
    c = BY_NAME[name]
    sd, xs32, _ = inputs(name)
    sdt = tp.to_torch(sd, torch.float64, False)
    T = lambda v: torch.as_tensor(np.array(v)).double()
    xs = {b: ([T(x) for x in v] if b == "radio" else T(v)) for b, v in xs32.items()}
    alphas, weights = quadrature(c)
    scale = lambda t, a: [x * a for x in t] if isinstance(t, list) else t * a
    flat = lambda t: [x for b in order(c.mode) for x in (t[b] if b == "radio" else [t[b]])]
    fr = rc.folded_operands(sd, xs32["radio"]) if c.radio else None
    fwd = lambda t: tp.mm_forward(sdt, t.get("radio"), t.get("path"), t.get("omic"), fusion="tensor",
                                  gate_path=c.path.gated if c.path else True, gate_radio=c.radio.gated if c.radio else True,
                                  dropout=False, mode=c.mode)
    allowance = c.tier == "C"
    shapes = {b: np.shape(v) for b, v in xs32.items()}
    allow = {b: np.zeros(s) for b, s in shapes.items()}
    allow_max = {b: np.zeros(s) for b, s in shapes.items()}
    allow_rowmax = {b: np.zeros(s[:-1]) for b, s in shapes.items() if b != "omic"}
    if allowance and c.radio:
        aXr = np.abs(fr.X)
    if allowance and c.path:
        aW1p, axp = np.abs(_f(sd, PRE_P + ".0.weight")), np.abs(np.asarray(xs32["path"], np.float64))
    if allowance and c.omic:
        aW0, aW1o = np.abs(_f(sd, "fc_omic.0.0.weight")), np.abs(_f(sd, "fc_omic.1.0.weight"))
        axo = np.abs(np.asarray(xs32["omic"], np.float64))

    def grads(ti, force):
        leaves = [x.requires_grad_() for x in flat(ti)]
        emb, _ = embeddings(c, sdt, ti)
        return [g.numpy() for g in torch.autograd.grad(_risk(tail(c, sdt, emb, force)[0]), leaves)]

    acc = [np.zeros(x.shape) for x in flat(xs)]
    step_risk, flagged, alt = [], {}, []
    for k, (a, w) in enumerate(zip(alphas, weights)):
        ti = {b: scale(v, a) for b, v in xs.items()}
        leaves = [x.requires_grad_() for x in flat(ti)]
        risk = -fwd(ti)[1].sum()
        g0 = [g.numpy() for g in torch.autograd.grad(risk, leaves)]
        for t, g in zip(acc, g0):
            t += w * g
        step_risk.append(float(risk.detach()))
        r2, pre, _, fl = node_tail(c, sd, sdt, xs32, xs, a, fr)
        assert abs(r2 - step_risk[-1]) <= 1e-12, (name, k)           # the cut forward is mm_forward
        if fl:
            flagged[k] = fl
            assert len(fl) <= NODE_CAP, (name, k, fl)
            natural = tuple(int(pre[lay][j] > 0) for lay, j in fl)
            opts = []
            for bits in itertools.product((0, 1), repeat=len(fl)):
                if bits == natural:
                    continue
                g = grads({b: scale(v, a) for b, v in xs.items()}, dict(zip(fl, bits)))
                d = [w * (gi - g0i) * x.numpy() for gi, g0i, x in zip(g, g0, flat(xs))]
                opts.append((bits, _split(c, d)))
            alt.append((k, opts))
        if not allowance:
            continue
        # the stack / omic allowance of mm_ig_cases.oracle, d risk / d embedding taken through the tail
        ti = {b: ([x.detach() for x in v] if b == "radio" else v.detach()) for b, v in ti.items()}
        emb, mid = embeddings(c, sdt, ti, leaves=True)
        lv = {b: ([mid[b][1]] if b != "omic" else [mid[b][1], mid[b][3]]) for b in emb}
        fl_ = [x for b in order(c.mode) for x in lv[b]]
        gs = dict(zip([id(x) for x in fl_], torch.autograd.grad(_risk(tail(c, sdt, emb)[0]), fl_)))
        if c.path:
            dh, u = gs[id(lv["path"][0])].numpy(), mid["path"][0].detach().numpy()
            i, j = np.nonzero(np.abs(u) <= mc.path_bound(sd, xs32["path"], a)[1])
            if i.size:
                term = (w * np.abs(dh[i, j]))[:, None] * aW1p[j] * axp[i]
                np.add.at(allow["path"], i, term)
                np.maximum.at(allow_max["path"], i, term)
                np.maximum.at(allow_rowmax["path"], i, term.sum(1))
        if c.radio:
            dh, u = gs[id(lv["radio"][0])].numpy(), mid["radio"][0].detach().numpy()
            i, j = np.nonzero(np.abs(u) <= rc.kink_bound(fr, a))
            if i.size:
                r = c.radio
                term = (w * np.abs(dh[i, j]))[:, None] * np.abs(fr.WW[j]) * aXr[i]
                term = term.reshape(-1, r.nseg, r.kseg).transpose(1, 0, 2)
                for m in range(r.nseg):
                    np.add.at(allow["radio"][m], i, term[m])
                    np.maximum.at(allow_max["radio"][m], i, term[m])
                    np.maximum.at(allow_rowmax["radio"][m], i, term[m].sum(1))
        if c.omic:
            dh1, dO = gs[id(lv["omic"][0])].numpy().reshape(-1), gs[id(lv["omic"][1])].numpy().reshape(-1)
            z1, e1, z2, e2 = mc.omic_bounds(sd, xs32["omic"], a)
            for cc in np.nonzero(np.abs(z1) <= e1)[0]:
                term = w * mc.JUMP * abs(dh1[cc]) * aW0[cc] * axo
                allow["omic"] += term
                np.maximum(allow_max["omic"], term, out=allow_max["omic"])
            for e in np.nonzero(np.abs(z2) <= e2)[0]:
                term = w * mc.JUMP * abs(dO[e]) * ((aW1o[e] * np.abs(mc.selu_grad(z1))) @ aW0) * axo
                allow["omic"] += term
                np.maximum(allow_max["omic"], term, out=allow_max["omic"])
    for k, a in ((c.n_steps, 1.0), (c.n_steps + 1, 0.0)):             # the riders: counted against the caps, no term
        fl = node_tail(c, sd, sdt, xs32, xs, a, fr)[3]
        if fl:
            flagged[k] = fl
    assert sum(len(v) for v in flagged.values()) <= CASE_CAP, (name, flagged)
    attr = _split(c, [t * x.numpy() for t, x in zip(acc, flat(xs))])
    with torch.no_grad():
        hz, S, Yh, _, _ = fwd(xs)
        logits = tail(c, sdt, embeddings(c, sdt, xs)[0])[0]
        risk = float(-S.sum())
        base = float(-fwd({b: scale(v, 0.0) for b, v in xs.items()})[1].sum())
    row_sum = {b: (v.sum(-1) if b != "omic" else v) for b, v in attr.items()}
    row_abs = {b: (np.abs(v).sum(-1) if b != "omic" else np.abs(v)) for b, v in attr.items()}
    mod_abs = {b: float(np.abs(v).sum()) for b, v in attr.items()}
    total, total_abs = float(sum(v.sum() for v in attr.values())), sum(mod_abs.values())
    arow = {b: (v.sum(-1) if b != "omic" else v) for b, v in allow.items()}
    bar_attr = {b: 1e-4 * np.abs(v).max() + allow[b] for b, v in attr.items()}
    bar_row = {b: 1e-4 * np.abs(row_abs[b]).max() + arow[b] for b in attr}
    return Oracle(attr, alt, row_sum, row_abs, mod_abs, total, total_abs, risk, base, np.asarray(step_risk),
                  hz.numpy().reshape(-1), S.numpy().reshape(-1), int(Yh), logits.numpy().reshape(-1), flagged, allow, allow_max,
                  allow_rowmax, bar_attr, bar_row)


def combinations(o):
    """Every combination of per-node assignments, float64's own first: ({node: assignment or None}, {branch: attr})."""
    nodes = [k for k, _ in o.alt]
    for pick in itertools.product(*[[None] + opts for _, opts in o.alt]):
        attr = {b: v.copy() for b, v in o.attr.items()} if any(p is not None for p in pick) else o.attr
        for p in pick:
            if p is not None:
                for b, d in p[1].items():
                    attr[b] += d
        yield {k: (p and p[0]) for k, p in zip(nodes, pick)}, attr


def match(o, got_attr, got_row_sum, got_row_abs):
    """The combination rule: the first combination under which EVERY array given lies within its bar -- attr (None: not
    returned), row_sum, row_abs, {branch: array} each.  Returns (combination, worst error / bar) or (None, the best
    combination's worst error / bar)."""
    best = np.inf
    for pick, attr in combinations(o):
        worst = 0.0
        for b, ref in attr.items():
            rs = ref.sum(-1) if b != "omic" else ref
            ra = np.abs(ref).sum(-1) if b != "omic" else np.abs(ref)
            if got_attr.get(b) is not None:
                worst = max(worst, float((np.abs(got_attr[b] - ref) / o.bar_attr[b]).max()))
            worst = max(worst, float((np.abs(got_row_sum[b] - rs) / o.bar_row[b]).max()),
                        float((np.abs(got_row_abs[b] - ra) / o.bar_row[b]).max()))
        if worst <= 1.0:
            return pick, worst
        best = min(best, worst)
    return None, best


def folded_attr(name):
    """The form the library runs, in float64: U_p, U_r with the composed bias and Z = W_o0 x_o once; per node the hidden parts
    and the tail on the embeddings, Gacc += w du per stack and Gz += w dz1; then the back-products.  {branch: attr}."""
    c = BY_NAME[name]
    sd, xs32, _ = inputs(name)
    sdt = tp.to_torch(sd, torch.float64, False)
    alphas, weights = quadrature(c)
    pre, G = {}, {}
    if c.path:
        xp = np.asarray(xs32["path"], np.float64)
        W1p = _f(sd, PRE_P + ".0.weight")
        pre["path"] = (xp @ W1p.T, _f(sd, PRE_P + ".0.bias"))
    if c.radio:
        fr = rc.folded_operands(sd, xs32["radio"])
        pre["radio"] = (fr.u, fr.b1c)
    if c.omic:
        xo = np.asarray(xs32["omic"], np.float64)
        W0 = _f(sd, "fc_omic.0.0.weight")
        pre["omic"] = ((W0 @ xo)[None, :], _f(sd, "fc_omic.0.0.bias"))
    for b, (u, _) in pre.items():
        G[b] = np.zeros_like(u)
    for a, w in zip(alphas, weights):
        leaves, emb = {}, {}
        for b, (u, bias) in pre.items():
            z = torch.as_tensor(a * u + bias)
            if b == "omic":
                z = z.requires_grad_()
                leaves[b] = z
                emb[b] = torch.nn.functional.selu(tp._lin(sdt, "fc_omic.1.0", torch.nn.functional.selu(z)))
            else:
                h = torch.relu(z).requires_grad_()
                leaves[b] = h
                emb[b] = _stack_tail(sdt, PRE_P if b == "path" else PRE_R, h, (c.path if b == "path" else c.radio).gated)[0]
        names = list(leaves)
        for b, g in zip(names, torch.autograd.grad(_risk(tail(c, sdt, emb)[0]), [leaves[b] for b in names])):
            g = g.numpy()
            G[b] += w * (g if b == "omic" else g * (leaves[b].detach().numpy() > 0))
    out = {}
    if c.path:
        out["path"] = xp * (G["path"] @ W1p)
    if c.radio:
        r = c.radio
        out["radio"] = (fr.X * ((G["radio"] @ fr.W1) @ fr.Wr)).reshape(r.N, r.nseg, r.kseg).transpose(1, 0, 2)
    if c.omic:
        out["omic"] = xo * (W0.T @ G["omic"][0])
    return out


def float32_gap(name):
    """The float32 check of BOUND: the same forward evaluated in float32 on the CPU (torch) at every node, riders included;
    yields (node, layer, |pre32 - pre64| [n], BOUND [n])."""
    c = BY_NAME[name]
    sd, xs32, _ = inputs(name)
    out = []
    runs = []
    for dt in (torch.float64, torch.float32):
        sdt = tp.to_torch(sd, dt, False)
        T = lambda v: torch.as_tensor(np.array(v)).to(dt)
        runs.append((sdt, {b: ([T(x) for x in v] if b == "radio" else T(v)) for b, v in xs32.items()}))
    fr = rc.folded_operands(sd, xs32["radio"]) if c.radio else None
    for k, a in enumerate(list(quadrature(c)[0]) + [1.0, 0.0]):
        _, pre64, bounds, _ = node_tail(c, sd, runs[0][0], xs32, runs[0][1], a, fr)
        sdt, xs = runs[1]
        a32 = torch.tensor(a, dtype=torch.float32)
        with torch.no_grad():
            emb, _ = embeddings(c, sdt, {b: ([x * a32 for x in v] if b == "radio" else v * a32) for b, v in xs.items()})
            pre32 = tail(c, sdt, emb)[1]
        for lay in LAYERS(len(emb)):
            out.append((k, lay, np.abs(_n(pre32[lay]) - pre64[lay]), bounds[lay]))
    return out
