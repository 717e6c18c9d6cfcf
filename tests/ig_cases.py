"""Cases, float64 oracle and error bars of the integrated-gradients tests (helper module, not collected by pytest).
tests/test_ig_cases_cpu.py checks the input conditions on these very arrays; tests/test_gpu_ig.py runs the kernels on them.

Oracle.  Integrated gradients by the definition, pass by pass: for every node alpha_k (the fp32 value the kernels get) one
torch.autograd pass in float64 over oracle.torch_port.path_forward on (alpha_k * x), risk = -sum(S), and
attr = x * sum_k w_k d risk / d(alpha_k x) -- the unfused form, not the folded one the library runs.  Computed once per case
(lru_cache) and never modified.

Bars.  For each output array 1e-4 * max|oracle| of that array (the relative part of the project's gradient bar; the
absolute 1e-5 floor is dropped: attributions of a 300-row bag are about 1e-3), plus the kink allowance; the three risks
take the project's 1e-4; `total` takes 1e-4 * sum|attr| plus the summed allowance.

Kink allowance.  A hidden unit whose float64 pre-activation alpha_k u_ij + b1_j lies within the projection's summation
bound of zero may fall on the other side of the ReLU in fp32; its gradient then appears or vanishes whole.  The bound is
(n' + 8) * 2^-24 * (alpha_k sum_l |x_il W1_jl| + |b1_j|) with n' = L / 2: the projection's accumulator takes one
v_mfma_f32_32x32x2_f32 -- two products -- per step of its k loop (csrc/mmf_gemm_core.h), a chain of L / 2 dependent
additions (a K-split only shortens it), the 8 for the products, the bias and the expand kernel's fused multiply-add.  For
each such (step, row, unit) the term w_k |dh_ij| |W1_jl| |x_il| (dh from the oracle) is added to the bar of attr[i, l],
its sum over l to the bars of row i's sums.  No element is skipped.  allow_max / allow_rowmax keep the largest single
unit's term per element / per row: what one flipped unit can move, for the comparison of two fp32 routes.

Below the oracle: the admitted-shape cases of tests/abi_shapes.py IG (shape_*), run by tests/test_gpu_ig_shapes.py and checked
by tests/test_ig_shapes_cpu.py -- kink-free by redraw, so with no allowance at all, and periodic where the bag is large."""
import collections
import functools

import numpy as np
import torch

from oracle import inputs as gen
from oracle import torch_port as tp

U = 2.0 ** -24
BIAS_STD = 0.1          # b1 != 0: with b1 = 0 the ReLU pattern is the same at every node and a wrong alpha would go unseen

Case = collections.namedtuple("Case", "name N size gated K n_steps method seed")

SMALL32, BIG32 = (32, 256, 256), (32, 512, 384)     # the two heads' hidden widths behind a 32-wide bag


def _c(name, N, size=SMALL32, gated=True, K=4, n_steps=20, method="gausslegendre", seed=11):
    return Case(name, N, size, gated, K, n_steps, method, seed)


# L = 32: the fp64 comparison is tight (few units near the kink).  N: one row; below a 16-row half block; straddling 16 and
# 32; past one 208 / 224-row tile, so that the steps of a window start mid-tile; 4096: several pooling groups per step.
CASES = [
    _c("n1", 1), _c("n5", 5), _c("n17", 17), _c("n33", 33), _c("n300", 300), _c("n4096", 4096),
    _c("n33_big_ungated_k1", 33, size=BIG32, gated=False, K=1),
    _c("n17_k1_one_step", 17, K=1, n_steps=1),
    _c("n33_four_steps_trapezoid", 33, n_steps=4, method="riemann_trapezoid"),
    _c("n5_big_ungated_middle", 5, size=BIG32, gated=False, n_steps=4, method="riemann_middle"),
]
# L = 1024, the heads as shipped: every row carries an allowance against fp64, so these are also held to the autograd route
# on the GPU at the tight bar
WIDE_CASES = [
    _c("small_gated_n300", 300, size="small"),
    _c("big_ungated_n33_k1", 33, size="big", gated=False, K=1, n_steps=4),
]
CAPPED = ("n300", "n4096")      # at most 10 % of their rows may carry any allowance
BY_NAME = {c.name: c for c in CASES + WIDE_CASES}


def quadrature(c, n_steps=None):
    """The rule's nodes and weights as the fp32 values the library is given, in float64."""
    from multimodalfusion_amd import ops
    a, w = ops.ig_quadrature(c.method, c.n_steps if n_steps is None else n_steps)
    return a.astype(np.float32).astype(np.float64), w.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = BY_NAME[name]
    L = gen.stack_dims(c.size)[0]
    sd = gen.path_state_dict(seed=c.seed, gated=c.gated, size=c.size, n_classes=c.K, dropout=False, bias_std=BIAS_STD)
    return sd, gen.bag(c.seed + 100, c.N, dim=L)


def _risk(sdt, x, gated):
    return -tp.path_forward(sdt, x, gated, False, None)[1].sum()


def _dh(sdt, xi, gated):
    """d risk / d h (the post-ReLU activation) and the pre-activation u at one node: path_forward's arithmetic, cut at h."""
    pre = "attention_net_WSI"
    u = tp._lin(sdt, pre + ".0", xi)
    h = torch.relu(u).detach().requires_grad_()
    A, _ = tp.attn_net(sdt, pre + ".3", h, gated, False, None)
    M = torch.softmax(A.T, dim=1) @ h
    S = tp.surv_head(tp._lin(sdt, "classifier", M))[1]
    (g,) = torch.autograd.grad(-S.sum(), h)
    return g.numpy(), u.detach().numpy(), float(-S.detach().sum())


Oracle = collections.namedtuple("Oracle", "attr row_sum row_abs total total_abs risk risk_base delta step_risk "
                                          "allow allow_max allow_rowmax flagged_rows bar_attr bar_rows bar_total")


@functools.lru_cache(maxsize=None)
def oracle(name, n_steps=None, allowance=True):
    c = BY_NAME[name]
    sd, x32 = inputs(name)
    sdt = tp.to_torch(sd, torch.float64, False)
    x = torch.as_tensor(x32).double()
    alphas, weights = quadrature(c, n_steps)
    W1 = np.abs(np.asarray(sd["attention_net_WSI.0.weight"], np.float64))
    b1 = np.abs(np.asarray(sd["attention_net_WSI.0.bias"], np.float64))
    ax = np.abs(x.numpy())
    L = x.shape[1]
    mag = ax @ W1.T                                   # sum_l |x_il W1_jl|
    acc = torch.zeros_like(x)
    allow, allow_max, allow_rowmax = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape[0])
    flagged = np.zeros(x.shape[0], bool)
    step_risk = []
    for a, w in zip(alphas, weights):
        xi = (x * a).requires_grad_()
        risk = _risk(sdt, xi, c.gated)
        (g,) = torch.autograd.grad(risk, xi)
        acc += w * g
        step_risk.append(float(risk.detach()))
        if not allowance:
            continue
        dh, u, r2 = _dh(sdt, xi.detach(), c.gated)
        assert abs(r2 - step_risk[-1]) <= 1e-12         # the cut forward is path_forward
        near = np.abs(u) <= (L // 2 + 8) * U * (a * mag + b1)
        i, j = np.nonzero(near)
        if i.size:
            flagged[i] = True
            term = (w * np.abs(dh[i, j]))[:, None] * W1[j] * ax[i]
            np.add.at(allow, i, term)
            np.maximum.at(allow_max, i, term)
            np.maximum.at(allow_rowmax, i, term.sum(1))
    attr = (acc * x).numpy()
    with torch.no_grad():
        risk = float(_risk(sdt, x, c.gated))
        base = float(_risk(sdt, torch.zeros_like(x), c.gated))
    row_sum, row_abs = attr.sum(1), np.abs(attr).sum(1)
    total, total_abs = float(attr.sum()), float(np.abs(attr).sum())
    arow = allow.sum(1)
    bar_rows = {"row_sum": 1e-4 * np.abs(row_sum).max() + arow, "row_abs": 1e-4 * np.abs(row_abs).max() + arow}
    return Oracle(attr, row_sum, row_abs, total, total_abs, risk, base, total - (risk - base), np.asarray(step_risk),
                  allow, allow_max, allow_rowmax, flagged, 1e-4 * np.abs(attr).max() + allow, bar_rows,
                  1e-4 * total_abs + float(allow.sum()))


# ---- the admitted-shape cases (tests/abi_shapes.py IG): kink-free inputs, periodic bags, zero allowance ---------------------
# Inputs.  A row is flagged if one of its units has a float64 pre-activation alpha u + b1 within the summation bound above of
# zero at any node of the call, alpha = 1 and alpha = 0 included; a flagged row is replaced by the same row of the generator's
# next draw until none is flagged (tests/cap_cases.py base_bag's manner).  So no case below carries an allowance: the bars are
# 1e-4 * max|oracle| per array, 1e-4 per risk, 1e-4 * sum|attr| on the total, and nothing is excused.
#
# Periodic bags.  Above what a direct oracle affords the bag is a base bag repeated, row i = base[i mod n0], gathered on the
# device (n0 above 256, no multiple of 16).  Pooling sees it as the base bag with multiplicities m_j = #{i < N : i mod n0 = j}:
# the risk at every node is the base bag's with log m_j added to the scores before the softmax, and d risk / d x_j of the base
# row, which its m_j copies share, is m_j times one copy's.  Row i's attribution is x_j (1 / m_j) sum_k w_k d risk_k / d x_j.
# With uniform m_j this is the direct oracle of the repeated bag to 1e-12 (tests/test_ig_shapes_cpu.py).
MAX_ROUNDS = 8
PRE = "attention_net_WSI"
SHAPE_SEED = 41


def shape_cases():
    import abi_shapes as ab
    return ab.accepted(ab.IG, ab.ig_rule)


def shape_by_name(name):
    return {c.name: c for c in shape_cases()}[name]


def shape_quadrature(c):
    """The rule's nodes and weights as fp32 (what the library is given)."""
    from multimodalfusion_amd import ops
    a, w = ops.ig_quadrature(c.method, c.n_steps)
    return a.astype(np.float32), w.astype(np.float32)


def multiplicities(N, n0):
    return np.full(n0, N // n0, np.int64) + (np.arange(n0) < N % n0)


def flagged_units(sd, x, alphas):
    """[n x H] bool: a float64 pre-activation within the projection's summation bound of zero at some node, riders included."""
    W1, b1 = np.asarray(sd[PRE + ".0.weight"], np.float64), np.asarray(sd[PRE + ".0.bias"], np.float64)
    x = np.asarray(x, np.float64)
    u, mag, ab1 = x @ W1.T, np.abs(x) @ np.abs(W1).T, np.abs(b1)
    flag = np.zeros(u.shape, bool)
    for a in list(np.asarray(alphas, np.float64)) + [1.0, 0.0]:
        flag |= np.abs(a * u + b1) <= (x.shape[1] // 2 + 8) * U * (a * mag + ab1)
    return flag


@functools.lru_cache(maxsize=None)
def shape_inputs(name):
    """(state dict, the bag or the base bag [n x L] fp32 read-only, redraw rounds)."""
    c = shape_by_name(name)
    n = c.n0 or c.N
    seed = SHAPE_SEED + c.L + c.H + c.D + c.K
    sd = gen.path_state_dict(seed=seed, gated=c.gated, size=c.size, n_classes=c.K, dropout=False, bias_std=BIAS_STD)
    x = gen.bag(seed + 100, n, dim=c.L).copy()
    alphas = shape_quadrature(c)[0]
    rounds = 0
    rows = np.arange(n)
    while True:
        rows = rows[flagged_units(sd, x[rows], alphas).any(axis=1)]
        if rows.size == 0:
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS, (name, rounds, rows.size)
        x[rows] = gen.bag(seed + 100 + 1000 * rounds, n, dim=c.L)[rows]
    x.setflags(write=False)
    return sd, x, rounds


def _head_m(sdt, xi, gated, logm):
    """path_forward's arithmetic (oracle/torch_port.py) cut at the softmax, where log m is added: (logits, hazards, S, Y_hat)."""
    h = torch.relu(tp._lin(sdt, PRE + ".0", xi))
    A, _ = tp.attn_net(sdt, PRE + ".3", h, gated, False, None)
    s = A.T if logm is None else A.T + logm[None, :]
    logits = tp._lin(sdt, "classifier", torch.softmax(s, dim=1) @ h)
    return (logits,) + tuple(tp.surv_head(logits))


ShapeOracle = collections.namedtuple("ShapeOracle", "attr row_sum row_abs mult total total_abs risk risk_base delta step_risk "
                                                    "logits hazards S Y_hat bar_attr bar_row_sum bar_row_abs bar_total")


def ig_oracle(sd, x32, mult, alphas, weights, gated):
    """Integrated gradients by the definition, in float64, of the bag that holds row j of x32 mult[j] times (None: the bag
    itself, through oracle.torch_port.path_forward): one autograd pass per node; per base row."""
    sdt = tp.to_torch(sd, torch.float64, False)
    x = torch.as_tensor(np.array(x32)).double()
    m = np.ones(x.shape[0]) if mult is None else np.asarray(mult, np.float64)
    logm = None if mult is None else torch.log(torch.as_tensor(m))
    risk_of = (lambda xi: _risk(sdt, xi, gated)) if mult is None else (lambda xi: -_head_m(sdt, xi, gated, logm)[2].sum())
    acc = torch.zeros_like(x)
    step_risk = []
    for a, w in zip(np.asarray(alphas, np.float64), np.asarray(weights, np.float64)):
        xi = (x * float(a)).requires_grad_()
        r = risk_of(xi)
        (g,) = torch.autograd.grad(r, xi)
        acc += float(w) * g
        step_risk.append(float(r.detach()))
    attr = (acc * x).numpy() / m[:, None]
    with torch.no_grad():
        logits, hz, S, Yh = _head_m(sdt, x, gated, logm)
        risk, base = float(risk_of(x)), float(risk_of(torch.zeros_like(x)))
        assert abs(risk + float(S.sum())) <= 1e-12
    row_sum, row_abs = attr.sum(1), np.abs(attr).sum(1)
    total, total_abs = float(m @ row_sum), float(m @ row_abs)
    return ShapeOracle(attr, row_sum, row_abs, m, total, total_abs, risk, base, total - (risk - base), np.asarray(step_risk),
                       logits.numpy().reshape(-1), hz.numpy().reshape(-1), S.numpy().reshape(-1), int(Yh), 1e-4 * np.abs(attr).max(),
                       1e-4 * np.abs(row_sum).max(), 1e-4 * np.abs(row_abs).max(), 1e-4 * total_abs)


@functools.lru_cache(maxsize=None)
def shape_oracle(name):
    """The oracle of one admitted-shape case, computed once and left unchanged."""
    c = shape_by_name(name)
    sd, x, _ = shape_inputs(name)
    a, w = shape_quadrature(c)
    return ig_oracle(sd, x, multiplicities(c.N, c.n0) if c.n0 else None, a, w, c.gated)
