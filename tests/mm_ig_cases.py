"""Cases, float64 oracle and error bars of the multimodal concat head's integrated-gradients tests (helper module, not
collected by pytest), in the manner of tests/radio_ig_cases.py.  tests/test_mm_ig_cases_cpu.py checks the input conditions
on these very arrays; tests/test_gpu_mm_ig.py runs the kernels on them.

Weights.  Tiers A and B: oracle.inputs._linear / _attn_stack under the model's key names (fc_omic.{0,1}.0,
attention_net_radio, reduce_dim, attention_net_WSI, classifier over the fused row), xavier, bias_std = 0.1 everywhere, so a
wrong alpha, a dropped composed bias b1' and a dropped omic bias all show.  Tier C: oracle.inputs.mm_state_dict(bias_std =
0.1), the shipped 1024-wide stacks, which the model loads.  Inputs: the pathology bag oracle.inputs.bag(seed + 100, N_p, L),
modality m of the radiology bag bag(seed + 200, N_r, kseg, stream = m), the omic vector normal(seed + 300, Gin); draw number
rnd adds 1000 rnd to the seed.

Oracle.  Integrated gradients by the definition, pass by pass: for every node alpha_k (the fp32 value the kernels get) one
torch.autograd pass in float64 over oracle.torch_port.mm_forward on (alpha_k * every input), risk = -sum(S), and
attr = input * sum_k w_k d risk / d(alpha_k input) -- the unfused form, not the folded one the library runs (folded_attr).
Computed once per case (lru_cache) and never modified.

Kinks.  A ReLU unit of the pathology stack is flagged as tests/ig_cases.py flags it, |alpha u + b1| <= (L / 2 + 8) 2^-24
(alpha sum_l |x_il W1_jl| + |b1_j|); one of the radiology stack, behind reduce_dim, as tests/radio_ig_cases.py does
(kink_bound there).  SELU is continuous, but its derivative jumps by JUMP = lambda (alpha_selu - 1) at 0, so an omic unit is
flagged when its float64 pre-activation lies within the summation error of the kernels' fp32 value
(csrc/mmf_amil_fwd.hip):
  layer 1, z1_c = fma(alpha, Z_c, b0_c) with Z_c from ig_omic_z_kernel -- ceil(Gin / 64) fused multiply-adds per lane, 6
    additions in the butterfly, then the fma: e1_c = (ceil(Gin / 64) + 6 + 2) 2^-24 (alpha sum_j |W0_cj x_j| + |b0_c|);
  layer 2, z2_e = sum_c W1_ec h1_c + b1_e in ig_omic_fwd_kernel -- ceil(W0 / 64) per lane, 6 in the butterfly, the bias:
    e2_e = (ceil(W0 / 64) + 7 + 2) 2^-24 (sum_c |W1_ec| |h1_c| + |b1_e|) + sum_c |W1_ec| dh1_c, the first layer's error
    carried through |W_o1|: dh1_c = lambda alpha_selu e1_c (SELU's slope is at most lambda alpha_selu) + 4 2^-24 (|h1_c| +
    lambda alpha_selu) for expf (one ulp), the subtraction and the two factors.
Every bound is evaluated at every node, alpha = 1 and alpha = 0 included.  With it the shipped omic widths [256, 256] draw
a flagged second-layer unit now and then (tier A redraws the vector); the wide layer of 80 -> [1024, 256] drew none on its
seed and stays in tier B all the same: a rougher bound (n 2^-24 of the magnitudes) flags it on every draw.

Allowance of a flagged unit: the whole term that can change.  ReLU: w_k |dh_ij| |W1_j.| * |x_i.| (radiology: |W1 Wr|_j.),
as in the two modules named above.  SELU: JUMP times the unit's gradient path -- layer 1: w_k JUMP |d risk / d h1_c| |W0_c.|
* |x_o|; layer 2: w_k JUMP |d risk / d O_e| (|W1_e.| * |selu'(z1)|) |W0| * |x_o|.  It is added to the bars of the elements
and sums it reaches.  No element's allowance may exceed ALLOW_CAP = 0.1 of max|oracle attr| of its case (else change the
seed, never the cap).

Bars: 1e-4 * max|oracle| per array plus allowance; 1e-4 per risk and per step_risk entry; 1e-4 * sum|attr| on the totals
plus allowance; share_b = abs_b / T from the bars B of modality_abs: (B_b + share_b sum B) / (T - sum B).

Tier A (L = kseg = 32): kink-free by redraw, at most MAX_ROUNDS = 16 rounds, nothing excused: a flagged pathology row is
replaced by the same row of the next draw, a flagged radiology row likewise in all its modalities, a flagged omic vector
whole.  Tier B: the allowance.  Tier C (the shipped widths): against float64 the allowance is as large as the signal, so
these are also held, on the GPU, to infer.mm_integrated_gradients_autograd at 1e-4 * max plus the largest single unit's
term (allow_max / allow_rowmax).

Tier B has no stack of H = 1024, which the single heads' tiers have.  No multimodal call admits it: two branches and F <= 1024 leave a stack at most
512 columns beside another of 512, so tier B runs 512 + 512 = 1024, the widest fused row there is
(tests/test_mm_ig_abi_cpu.py asserts that H = 1024 is refused)."""
import collections
import functools

import numpy as np
import torch

import radio_ig_cases as rc
from oracle import inputs as gen
from oracle import torch_port as tp

U = 2.0 ** -24
BIAS_STD = 0.1
MAX_ROUNDS = 16
ALLOW_CAP = 0.1
SELU_ALPHA, SELU_SCALE = tp._SELU_ALPHA, tp._SELU_SCALE
JUMP = SELU_SCALE * (SELU_ALPHA - 1.0)
PRE_P, PRE_R = "attention_net_WSI", "attention_net_radio"

Path = collections.namedtuple("Path", "L H D gated N")
Radio = collections.namedtuple("Radio", "nseg kseg H D gated N")
Omic = collections.namedtuple("Omic", "Gin W0 We")
Case = collections.namedtuple("Case", "name tier mode path radio omic K n_steps method window_steps seed")


def _c(name, tier, mode, path=None, radio=None, omic=None, K=4, n_steps=20, method="gausslegendre", window_steps=0, seed=31):
    assert (path is not None) == ("path" in mode) and (radio is not None) == ("radio" in mode)
    assert (omic is not None) == ("omic" in mode)
    return Case(name, tier, mode, path and Path(*path), radio and Radio(*radio), omic and Omic(*omic), K, n_steps, method,
                window_steps, seed)


TIER_A = [
    # the shipped hidden widths
    _c("a_rpo_shipped_hidden", "A", "radio_path_omic", (32, 256, 256, True, 65), (4, 32, 256, 256, True, 17), (80, 256, 256)),
    # mixed gates, steps starting mid-tile, N_p != N_r
    _c("a_rp_mixed_gates_n300", "A", "radio_path", (32, 256, 256, False, 300), (2, 32, 256, 256, True, 33)),
    # odd omic widths, F = 320
    _c("a_ro_odd_omic_k1", "A", "radio_omic", None, (3, 32, 256, 256, True, 65), (7, 33, 64), K=1),
    # omic columns first, unequal column widths
    _c("a_po_omic_first_big", "A", "path_omic", (32, 512, 384, True, 17), None, (36, 256, 256)),
    # one row everywhere
    _c("a_rpo_one_row_k32", "A", "radio_path_omic", (32, 256, 128, True, 1), (2, 32, 256, 128, False, 1), (1, 64, 32), K=32),
    # library-chosen windows with the two stacks far apart in size
    _c("a_rpo_far_apart_n4096", "A", "radio_path_omic", (32, 256, 256, True, 4096), (4, 32, 256, 256, True, 150),
       (80, 256, 256), n_steps=4, method="riemann_middle"),
    # the riders alone in the last window
    _c("a_rp_riders_alone", "A", "radio_path", (32, 256, 128, False, 17), (2, 32, 256, 128, False, 17), n_steps=64,
       window_steps=64),
    _c("a_po_one_step_windows", "A", "path_omic", (32, 256, 128, True, 17), None, (7, 33, 64), n_steps=1,
       method="riemann_middle", window_steps=1),
]
TIER_B = [
    _c("b_rpo_l96_omic_big", "B", "radio_path_omic", (96, 256, 128, True, 65), (3, 96, 256, 128, True, 33), (80, 1024, 256)),
    _c("b_rp_l160_f1024_k32", "B", "radio_path", (160, 512, 384, True, 33), (4, 160, 512, 640, True, 33), K=32, n_steps=4,
       method="riemann_middle"),
]
TIER_C = [
    _c("c_rpo_small_gated", "C", "radio_path_omic", (1024, 256, 256, True, 150), (4, 1024, 256, 256, True, 33), (80, 256, 256)),
    _c("c_po_small_ungated", "C", "path_omic", (1024, 256, 256, False, 33), None, (80, 256, 256), n_steps=4,
       method="riemann_middle"),
]
CASES = TIER_A + TIER_B + TIER_C
BY_NAME = {c.name: c for c in CASES}
BRANCHES = ("radio", "path", "omic")


def order(mode):
    """The branches in the fused row's column order (models/model_mm_attention_mil.py:168-187 of the reference)."""
    has = lambda k: k in mode
    if has("radio") and has("path") and not has("omic"):
        return ["radio", "path"]
    if has("radio") and has("omic") and not has("path"):
        return ["radio", "omic"]
    if has("omic") and has("path") and not has("radio"):
        return ["omic", "path"]
    return ["radio", "path", "omic"]


def widths(c):
    return {"radio": c.radio and c.radio.H, "path": c.path and c.path.H, "omic": c.omic and c.omic.We}


def columns(c):
    """{branch: (first column, width)} and F."""
    cols, F = {}, 0
    for b in order(c.mode):
        cols[b] = (F, widths(c)[b])
        F += widths(c)[b]
    return cols, F


quadrature = rc.quadrature


def state_dict(c):
    if c.tier == "C":
        assert c.omic == Omic(80, 256, 256) and (c.radio is None or c.radio[:4] == (4, 1024, 256, 256))
        return gen.mm_state_dict(seed=c.seed, input_dim=80, fusion="concat", gate_path=c.path.gated,
                                 gate_radio=c.radio.gated if c.radio else True, dropout=False, n_classes=c.K, mode=c.mode,
                                 n_mod=4, bias_std=BIAS_STD)
    sd, st = collections.OrderedDict(), 0
    if c.omic:
        st = gen._linear(sd, "fc_omic.0.0", c.omic.W0, c.omic.Gin, c.seed, st, "xavier", BIAS_STD)
        st = gen._linear(sd, "fc_omic.1.0", c.omic.We, c.omic.W0, c.seed, st, "xavier", BIAS_STD)
    if c.radio:
        r = c.radio
        st = gen._attn_stack(sd, PRE_R, (r.kseg, r.H, r.D), r.gated, False, c.seed, st, "xavier", BIAS_STD)
        st = gen._linear(sd, "reduce_dim", r.kseg, r.kseg * r.nseg, c.seed, st, "xavier", BIAS_STD)
    if c.path:
        p = c.path
        st = gen._attn_stack(sd, PRE_P, (p.L, p.H, p.D), p.gated, False, c.seed, st, "xavier", BIAS_STD)
    gen._linear(sd, "classifier", c.K, columns(c)[1], c.seed, st, "xavier", BIAS_STD)
    return sd


def draw(c, rnd):
    """{branch: array} of the generator's draw number rnd: path [N_p x L], radio [nseg x N_r x kseg], omic [Gin]."""
    s = c.seed + 1000 * rnd
    out = {}
    if c.path:
        out["path"] = gen.bag(s + 100, c.path.N, dim=c.path.L)
    if c.radio:
        out["radio"] = np.stack([gen.bag(s + 200, c.radio.N, dim=c.radio.kseg, stream=m) for m in range(c.radio.nseg)])
    if c.omic:
        out["omic"] = gen.normal(s + 300, (c.omic.Gin,))
    return out


def _f(sd, k):
    return np.asarray(sd[k], np.float64)


# ---- kink bounds -------------------------------------------------------------------------------------------------------------
def path_bound(sd, x, a):
    """([N x H] pre-activation at node a, its bound): tests/ig_cases.py's."""
    W1, b1 = _f(sd, PRE_P + ".0.weight"), _f(sd, PRE_P + ".0.bias")
    x = np.asarray(x, np.float64)
    L = x.shape[1]
    return a * (x @ W1.T) + b1, (L // 2 + 8) * U * (a * (np.abs(x) @ np.abs(W1).T) + np.abs(b1))


def selu(z):
    return SELU_SCALE * np.where(z > 0, z, SELU_ALPHA * np.expm1(np.minimum(z, 0)))


def selu_grad(z):
    return SELU_SCALE * np.where(z > 0, 1.0, SELU_ALPHA * np.exp(np.minimum(z, 0)))


def omic_chain(n):
    """Dependent additions of one wave's sum over n terms: ceil(n / 64) per lane and the butterfly's 6."""
    return (n + 63) // 64 + 6


def omic_bounds(sd, x, a):
    """(z1 [W0], e1, z2 [We], e2) at node a: the float64 pre-activations of the two SNN layers and the summation error of the
    kernels' fp32 values (module docstring)."""
    W0, b0, W1, b1 = (_f(sd, k) for k in ("fc_omic.0.0.weight", "fc_omic.0.0.bias", "fc_omic.1.0.weight", "fc_omic.1.0.bias"))
    x = np.asarray(x, np.float64)
    Gin, W0n = W0.shape[1], W0.shape[0]
    z1 = a * (W0 @ x) + b0
    e1 = (omic_chain(Gin) + 2) * U * (a * (np.abs(W0) @ np.abs(x)) + np.abs(b0))
    h1 = selu(z1)
    dh1 = SELU_SCALE * SELU_ALPHA * e1 + 4 * U * (np.abs(h1) + SELU_SCALE * SELU_ALPHA)
    z2 = W1 @ h1 + b1
    e2 = (omic_chain(W0n) + 1 + 2) * U * (np.abs(W1) @ np.abs(h1) + np.abs(b1)) + np.abs(W1) @ dh1
    return z1, e1, z2, e2


def flagged(c, sd, xs, alphas):
    """{branch: bool array} -- path [N_p x H], radio [N_r x H], omic ([W0], [We]): a float64 pre-activation within its bound
    of the kink at some node, the riders alpha = 1 and 0 included."""
    nodes = list(np.asarray(alphas, np.float64)) + [1.0, 0.0]
    out = {}
    if c.path:
        out["path"] = np.zeros((c.path.N, c.path.H), bool)
        for a in nodes:
            u, e = path_bound(sd, xs["path"], a)
            out["path"] |= np.abs(u) <= e
    if c.radio:
        out["radio"] = rc.flagged_units(sd, xs["radio"], alphas)
    if c.omic:
        f1, f2 = np.zeros(c.omic.W0, bool), np.zeros(c.omic.We, bool)
        for a in nodes:
            z1, e1, z2, e2 = omic_bounds(sd, xs["omic"], a)
            f1 |= np.abs(z1) <= e1
            f2 |= np.abs(z2) <= e2
        out["omic"] = (f1, f2)
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(state dict, {branch: fp32 read-only array}, redraw rounds).  Tier A: redrawn until nothing is flagged."""
    c = BY_NAME[name]
    sd = state_dict(c)
    xs = {k: v.copy() for k, v in draw(c, 0).items()}
    rounds = 0
    if c.tier == "A":
        alphas = quadrature(c)[0]
        while True:
            f = flagged(c, sd, xs, alphas)
            bad_p = f["path"].any(axis=1) if c.path else np.zeros(0, bool)
            bad_r = f["radio"].any(axis=1) if c.radio else np.zeros(0, bool)
            bad_o = bool(c.omic) and bool(f["omic"][0].any() or f["omic"][1].any())
            if not (bad_p.any() or bad_r.any() or bad_o):
                break
            rounds += 1
            assert rounds <= MAX_ROUNDS, (name, rounds, int(bad_p.sum()), int(bad_r.sum()), bad_o)
            nxt = draw(c, rounds)
            if bad_p.any():
                xs["path"][bad_p] = nxt["path"][bad_p]
            if bad_r.any():
                xs["radio"][:, bad_r] = nxt["radio"][:, bad_r]
            if bad_o:
                xs["omic"] = nxt["omic"].copy()
    for v in xs.values():
        v.setflags(write=False)
    return sd, xs, rounds


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def _forward(c, sdt, t):
    """mm_forward on {branch: tensor(s)}."""
    return tp.mm_forward(sdt, t.get("radio"), t.get("path"), t.get("omic"), fusion="concat",
                         gate_path=c.path.gated if c.path else True, gate_radio=c.radio.gated if c.radio else True,
                         dropout=False, mode=c.mode)


def _stack_tail(sdt, pre, h, gated):
    A, _ = tp.attn_net(sdt, pre + ".3", h, gated, False, None)
    return torch.softmax(A.T, dim=1) @ h


def _cut(c, sdt, t):
    """mm_forward's arithmetic cut at the activations: {path: (dh, u), radio: (dh, u), omic: (dh1, dO, z1, z2)} and the
    risk at one node."""
    leaves, emb, pre = {}, {}, {}
    if c.path:
        u = tp._lin(sdt, PRE_P + ".0", t["path"])
        h = torch.relu(u).detach().requires_grad_()
        leaves["path"], pre["path"], emb["path"] = [h], u, _stack_tail(sdt, PRE_P, h, c.path.gated)
    if c.radio:
        u = tp._lin(sdt, PRE_R + ".0", tp._lin(sdt, "reduce_dim", torch.cat(list(t["radio"]), dim=1)))
        h = torch.relu(u).detach().requires_grad_()
        leaves["radio"], pre["radio"], emb["radio"] = [h], u, _stack_tail(sdt, PRE_R, h, c.radio.gated)
    if c.omic:
        z1 = tp._lin(sdt, "fc_omic.0.0", t["omic"].unsqueeze(0))
        h1 = torch.nn.functional.selu(z1).detach().requires_grad_()
        z2 = tp._lin(sdt, "fc_omic.1.0", h1)
        O = torch.nn.functional.selu(z2)
        leaves["omic"], pre["omic"], emb["omic"] = [h1, O], (z1, z2), O
    S = tp.surv_head(tp._lin(sdt, "classifier", torch.cat([emb[b] for b in order(c.mode)], dim=1)))[1]
    risk = -S.sum()
    flat = [x for b in order(c.mode) for x in leaves[b]]
    gs = dict(zip([id(x) for x in flat], torch.autograd.grad(risk, flat)))
    out = {}
    for b in order(c.mode):
        g = [gs[id(x)].numpy() for x in leaves[b]]
        out[b] = (g[0], pre[b].detach().numpy()) if b != "omic" else (
            g[0].reshape(-1), g[1].reshape(-1), pre[b][0].detach().numpy().reshape(-1), pre[b][1].detach().numpy().reshape(-1))
    return out, float(risk.detach())


Oracle = collections.namedtuple("Oracle", "attr row_sum row_abs mod_sum mod_abs share total total_abs risk risk_base delta "
                                          "step_risk hazards S Y_hat logits allow allow_max allow_rowmax flagged bar_attr "
                                          "bar_row_sum bar_row_abs bar_mod_abs bar_share bar_total")


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per branch (dicts keyed radio / path / omic, the present ones): attr (radio [nseg x N x kseg], path [N x L], omic
    [Gin]), row_sum / row_abs (radio [nseg x N], path [N]; omic: attr and |attr|), the sums per modality, share, and in
    all; the risks; the head's outputs at alpha = 1; the allowances and the bars.  Tier A carries no allowance."""
    c = BY_NAME[name]
    sd, xs32, _ = inputs(name)
    sdt = tp.to_torch(sd, torch.float64, False)
    T = lambda v: torch.as_tensor(np.array(v)).double()
    xs = {b: ([T(x) for x in v] if b == "radio" else T(v)) for b, v in xs32.items()}
    alphas, weights = quadrature(c)
    allowance = c.tier != "A"
    scale = lambda t, a: [x * a for x in t] if isinstance(t, list) else t * a
    flat = lambda t: [x for b in order(c.mode) for x in (t[b] if b == "radio" else [t[b]])]
    acc = [torch.zeros_like(x) for x in flat(xs)]
    shapes = {b: np.shape(v) for b, v in xs32.items()}
    allow = {b: np.zeros(s) for b, s in shapes.items()}
    allow_max = {b: np.zeros(s) for b, s in shapes.items()}
    allow_rowmax = {b: np.zeros(s[:-1]) for b, s in shapes.items() if b != "omic"}
    flg = {b: np.zeros(shapes[b][-2], bool) for b in shapes if b != "omic"}
    if c.omic:
        flg["omic"] = [np.zeros(c.omic.W0, bool), np.zeros(c.omic.We, bool)]
    if allowance and c.radio:
        fr = rc.folded_operands(sd, xs32["radio"])
        aXr = np.abs(fr.X)
    if allowance and c.path:
        aW1p, axp = np.abs(_f(sd, PRE_P + ".0.weight")), np.abs(np.asarray(xs32["path"], np.float64))
    if allowance and c.omic:
        aW0, aW1o = np.abs(_f(sd, "fc_omic.0.0.weight")), np.abs(_f(sd, "fc_omic.1.0.weight"))
        axo = np.abs(np.asarray(xs32["omic"], np.float64))
    step_risk = []
    for a, w in zip(alphas, weights):
        ti = {b: scale(v, a) for b, v in xs.items()}
        leaves = [x.requires_grad_() for x in flat(ti)]
        risk = -_forward(c, sdt, ti)[1].sum()
        for t, g in zip(acc, torch.autograd.grad(risk, leaves)):
            t += w * g
        step_risk.append(float(risk.detach()))
        if not allowance:
            continue
        cut, r2 = _cut(c, sdt, {b: ([x.detach() for x in v] if b == "radio" else v.detach()) for b, v in ti.items()})
        assert abs(r2 - step_risk[-1]) <= 1e-12                     # the cut forward is mm_forward
        if c.path:
            dh, u = cut["path"]
            u2, e = path_bound(sd, xs32["path"], a)
            assert np.abs(u - u2).max() <= 1e-10 * max(1.0, np.abs(u).max())
            i, j = np.nonzero(np.abs(u) <= e)
            if i.size:
                flg["path"][i] = True
                term = (w * np.abs(dh[i, j]))[:, None] * aW1p[j] * axp[i]
                np.add.at(allow["path"], i, term)
                np.maximum.at(allow_max["path"], i, term)
                np.maximum.at(allow_rowmax["path"], i, term.sum(1))
        if c.radio:
            dh, u = cut["radio"]
            assert np.abs(u - (a * fr.u + fr.b1c)).max() <= 1e-10 * max(1.0, np.abs(u).max())
            i, j = np.nonzero(np.abs(u) <= rc.kink_bound(fr, a))
            if i.size:
                flg["radio"][i] = True
                r = c.radio
                term = (w * np.abs(dh[i, j]))[:, None] * np.abs(fr.WW[j]) * aXr[i]
                term = term.reshape(-1, r.nseg, r.kseg).transpose(1, 0, 2)
                for m in range(r.nseg):
                    np.add.at(allow["radio"][m], i, term[m])
                    np.maximum.at(allow_max["radio"][m], i, term[m])
                    np.maximum.at(allow_rowmax["radio"][m], i, term[m].sum(1))
        if c.omic:
            dh1, dO, z1, z2 = cut["omic"]
            q1, e1, q2, e2 = omic_bounds(sd, xs32["omic"], a)
            assert np.abs(z1 - q1).max() <= 1e-10 * max(1.0, np.abs(z1).max()) and np.abs(z2 - q2).max() <= 1e-10 * max(1.0, np.abs(z2).max())
            for cc in np.nonzero(np.abs(z1) <= e1)[0]:
                flg["omic"][0][cc] = True
                term = w * JUMP * abs(dh1[cc]) * aW0[cc] * axo
                allow["omic"] += term
                np.maximum(allow_max["omic"], term, out=allow_max["omic"])
            for e in np.nonzero(np.abs(z2) <= e2)[0]:
                flg["omic"][1][e] = True
                term = w * JUMP * abs(dO[e]) * ((aW1o[e] * np.abs(selu_grad(z1))) @ aW0) * axo
                allow["omic"] += term
                np.maximum(allow_max["omic"], term, out=allow_max["omic"])
    prod = [(t * x).numpy() for t, x in zip(acc, flat(xs))]
    attr, k = {}, 0
    for b in order(c.mode):
        n = c.radio.nseg if b == "radio" else 1
        attr[b] = np.stack(prod[k:k + n]) if b == "radio" else prod[k]
        k += n
    with torch.no_grad():
        hz, S, Yh, _, MM = _forward(c, sdt, xs)
        logits = tp._lin(sdt, "classifier", MM)
        risk = float(-S.sum())
        base = float(-_forward(c, sdt, {b: scale(v, 0.0) for b, v in xs.items()})[1].sum())
    row_sum = {b: (v.sum(-1) if b != "omic" else v) for b, v in attr.items()}
    row_abs = {b: (np.abs(v).sum(-1) if b != "omic" else np.abs(v)) for b, v in attr.items()}
    mod_sum = {b: float(v.sum()) for b, v in attr.items()}
    mod_abs = {b: float(np.abs(v).sum()) for b, v in attr.items()}
    total, total_abs = sum(mod_sum.values()), sum(mod_abs.values())
    share = {b: v / total_abs for b, v in mod_abs.items()}
    arow = {b: (v.sum(-1) if b != "omic" else v) for b, v in allow.items()}
    bar_attr = {b: 1e-4 * np.abs(v).max() + allow[b] for b, v in attr.items()}
    bar_row_sum = {b: 1e-4 * np.abs(v).max() + arow[b] for b, v in row_sum.items()}
    bar_row_abs = {b: 1e-4 * np.abs(v).max() + arow[b] for b, v in row_abs.items()}
    bar_mod_abs = {b: 1e-4 * v + float(allow[b].sum()) for b, v in mod_abs.items()}
    sumB = sum(bar_mod_abs.values())
    bar_share = {b: (bar_mod_abs[b] + share[b] * sumB) / (total_abs - sumB) if total_abs > sumB else np.inf for b in share}
    bar_total = 1e-4 * total_abs + sum(float(v.sum()) for v in allow.values())
    return Oracle(attr, row_sum, row_abs, mod_sum, mod_abs, share, total, total_abs, risk, base, total - (risk - base),
                  np.asarray(step_risk), hz.numpy().reshape(-1), S.numpy().reshape(-1), int(Yh), logits.numpy().reshape(-1),
                  allow, allow_max, allow_rowmax, flg, bar_attr, bar_row_sum, bar_row_abs, bar_mod_abs, bar_share, bar_total)


def folded_attr(name):
    """The form the library runs, in float64: U_p, U_r with the composed bias, Z = W_o0 x_o once; per node the hidden parts
    and one head over the fused row, Gacc += w du per stack and Gz += w dz1; then the back-products.  {branch: attr}."""
    c = BY_NAME[name]
    sd, xs32, _ = inputs(name)
    sdt = tp.to_torch(sd, torch.float64, False)
    alphas, weights = quadrature(c)
    pre, G = {}, {}
    if c.path:
        xp = np.asarray(xs32["path"], np.float64)
        W1p, b1p = _f(sd, PRE_P + ".0.weight"), _f(sd, PRE_P + ".0.bias")
        pre["path"] = (xp @ W1p.T, b1p)
    if c.radio:
        fr = rc.folded_operands(sd, xs32["radio"])
        pre["radio"] = (fr.u, fr.b1c)
    if c.omic:
        xo = np.asarray(xs32["omic"], np.float64)
        W0, b0 = _f(sd, "fc_omic.0.0.weight"), _f(sd, "fc_omic.0.0.bias")
        pre["omic"] = ((W0 @ xo)[None, :], b0)
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
                emb[b] = _stack_tail(sdt, PRE_P if b == "path" else PRE_R, h, (c.path if b == "path" else c.radio).gated)
        S = tp.surv_head(tp._lin(sdt, "classifier", torch.cat([emb[b] for b in order(c.mode)], dim=1)))[1]
        names = list(leaves)
        for b, g in zip(names, torch.autograd.grad(-S.sum(), [leaves[b] for b in names])):
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
