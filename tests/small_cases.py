"""Inputs, float64 references and error bounds of the small-op tables of tests/abi_shapes.py (helper module, not collected
by pytest).  tests/test_abi_shapes_cpu.py checks the input conditions on these very arrays and pins the vectorised
restatements to the ports; tests/test_gpu_small_shapes.py runs the kernels on them.

Every reference is float64 on the CPU from the same fp32 inputs, computed once per case (lru_cache) and never modified.
A backward reference takes the forward reference's output rounded to fp32 -- what the backward kernel is given -- and
derives the activation derivative and the dropout mask from it as the kernel does, in float64: no unit sits on the wrong
side of a ReLU / SELU kink, and no element is left out of a comparison.

Bars.  Where the suite already holds a bar for an op the tests use it for shapes within the sizes it was set on (cited at
each use).  Beyond them: the summation bound.  An output that is a sum of n fp32 terms t_i is off by at most
(n' + 8) * 2^-24 * sum|t_i|, n' the longest add chain the element sees in the kernel (read from the code, stated at each
use), the 8 for the few-ulp transcendentals and products that make a term (csrc/mmf_common.h:58).  Where a term is itself
computed from an earlier sum, that sum's bound times the term's derivative is added.  The reference computes sum|t_i|."""
import functools
import math

import numpy as np
import torch

import abi_shapes as ab
from oracle import inputs as gen
from oracle import stage2_port as s2
from oracle import torch_port as tp

U = 2.0 ** -24
SEED, SITE, P_DROP = 321, 1, 0.25
SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
f64 = np.float64


def T(a):
    return torch.as_tensor(np.asarray(a)).double()


def r32(a):
    """A float64 reference output as the fp32 array the next kernel is given."""
    return np.asarray(a, f64).astype(np.float32)


def act_ref(v, act):
    return {0: lambda v: v, 1: lambda v: np.maximum(v, 0), 2: np.tanh, 3: lambda v: 1 / (1 + np.exp(-v)),
            4: lambda v: SELU_SCALE * np.where(v > 0, v, SELU_ALPHA * np.expm1(np.minimum(v, 0)))}[act](v)


def act_grad_from_y(y, act):
    """csrc/mmf_mlp.hip:29-37 in float64."""
    return {0: lambda y: np.ones_like(y), 1: lambda y: (y > 0).astype(f64), 2: lambda y: 1 - y * y, 3: lambda y: y * (1 - y),
            4: lambda y: np.where(y > 0, SELU_SCALE, y + SELU_SCALE * SELU_ALPHA)}[act](y)


def alpha_affine(p):
    """csrc/mmf_mlp.hip:41-47 in float64: (a, b, alpha')."""
    alpha_p = -SELU_ALPHA * SELU_SCALE
    a = 1.0 / math.sqrt((alpha_p * alpha_p * p + 1.0) * (1.0 - p))
    return a, -a * alpha_p * p, alpha_p


def drop_fwd(y, keep, kind, p=P_DROP):
    if kind == 0:
        return y
    if kind == 1:
        return np.where(keep, y / (1 - p), 0.0)
    a, b, alpha_p = alpha_affine(p)
    return a * np.where(keep, y, alpha_p) + b


def drop_bwd(yd, keep, kind, p=P_DROP):
    """csrc/mmf_mlp.hip:56-63 in float64: (d out / d y, y recovered from the dropped output)."""
    yd = np.asarray(yd, f64)
    if kind == 0:
        return np.ones_like(yd), yd
    if kind == 1:
        return np.where(keep, 1 / (1 - p), 0.0), np.where(keep, yd * (1 - p), 0.0)
    a, b, _ = alpha_affine(p)
    return np.where(keep, a, 0.0), np.where(keep, (yd - b) / a, 0.0)


def prod_others(h):
    """P[b, t, j] = prod_{u <= j, u != t} (1 - h[b, u]) for j >= t, else 0: -dS_j / dh_t, without a division."""
    B, K = h.shape
    P = np.zeros((B, K, K), f64)
    for t in range(K):
        run = np.ones(B, f64)
        for u in range(t):
            run = run * (1 - h[:, u])
        for j in range(t, K):
            if j > t:
                run = run * (1 - h[:, j])
            P[:, t, j] = run
    return P


def top_two_gap(logits):
    if logits.shape[1] < 2:
        return np.inf
    s = np.sort(np.asarray(logits, f64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def _steep(B, K):
    return np.where((np.arange(K)[None, :] + np.arange(B)[:, None]) % 2 == 0, 30.0, -30.0).astype(np.float32)


# ---- survival head -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_inputs(c):
    feat = gen.normal(11, (c.B, c.F), stream=c.B + c.K)
    Wk = gen.normal(12, (c.K, c.F), stream=c.K, std=1.0 / np.sqrt(c.F))
    bk = gen.normal(13, (c.K,), stream=1, std=0.3)
    if c.steep:
        bk = (bk + _steep(1, c.K)[0]).astype(np.float32)
    return dict(feat=feat, Wk=Wk, bk=bk, gH=gen.normal(14, (c.B, c.K), stream=2), gS=gen.normal(15, (c.B, c.K), stream=3))


def _head_within(c):
    return c.B <= 16 and c.K <= 8 and c.F <= 256        # tests/test_gpu_radio_small.py:100-103


@functools.lru_cache(maxsize=None)
def head_ref(c):
    """tp.surv_head on the float64 logits; the backward from the fp32 hazards."""
    i = head_inputs(c)
    feat, Wk, bk = (np.asarray(i[k], f64) for k in ("feat", "Wk", "bk"))
    logits = feat @ Wk.T + bk
    hz, S, Yh = (t.numpy() for t in tp.surv_head(T(logits)))
    out = dict(logits=logits, hazards=hz, S=S, Y_hat=Yh.reshape(-1))
    # lane chain of F / 64 terms, wave_sum (6), the bias
    b_z = (-(-c.F // 64) + 6 + 1 + 8) * U * (np.abs(feat) @ np.abs(Wk).T + np.abs(bk))
    b_h = b_z / 4 + 8 * U
    bar = dict(logits=b_z)
    if _head_within(c):                                  # tests/test_gpu_radio_small.py:119-120
        bar.update(hazards=np.full_like(hz, 1e-5), S=np.full_like(S, 1e-5))
    else:                                                # |dS_j / dh_u| <= 1: the hazards' errors add up along the product
        bar.update(hazards=b_h, S=np.cumsum(b_h, 1) + (np.arange(c.K) + 9) * U * S)
    h = np.asarray(r32(hz), f64)
    gH, gS = np.asarray(i["gH"], f64), np.asarray(i["gS"], f64)
    P = prod_others(h)
    dh = gH - np.einsum("bj,btj->bt", gS, P)
    hh = h * (1 - h)
    dz = dh * hh
    out.update(dfeat=dz @ Wk, dWk=dz.T @ feat, dbk=dz.sum(0), h32=r32(hz))
    if _head_within(c):                                  # tests/test_gpu_radio_small.py:123
        bar.update({k: 1e-5 + 1e-4 * np.abs(out[k]) for k in ("dfeat", "dWk", "dbk")})
    else:                                                # dz: K products of up to K factors, summed; then sums over K or B
        e_dz = (3 * c.K + 8) * U * (np.abs(gH) + np.einsum("bj,btj->bt", np.abs(gS), P)) * hh
        a_dz = np.abs(dz)
        bar.update(dfeat=(c.K + 8) * U * (a_dz @ np.abs(Wk)) + e_dz @ np.abs(Wk),
                   dWk=(c.B + 8) * U * (a_dz.T @ np.abs(feat)) + e_dz.T @ np.abs(feat),
                   dbk=(c.B + 8) * U * a_dz.sum(0) + e_dz.sum(0))
    return out, bar


# ---- nll_surv --------------------------------------------------------------------------------------------------------------
NLL_ALPHA, NLL_EPS = 0.4, 1e-7


@functools.lru_cache(maxsize=None)
def nll_inputs(c):
    z = gen.normal(21, (c.B, c.K), stream=c.B, std=1.5)
    hz = (1 / (1 + np.exp(-z.astype(f64)))).astype(np.float32)
    S = np.cumprod(1 - hz.astype(f64), 1).astype(np.float32)
    b = np.arange(c.B)
    Y = ((b * 3) % c.K).astype(np.int64)
    cc = ((b // c.K) % 2).astype(np.float32)
    if c.bad_row >= 0:
        Y[c.bad_row] = c.K
    return dict(hazards=hz, S=S, Y=Y, c=cc)


@functools.lru_cache(maxsize=None)
def nll_ref(c):
    """tp.nll_loss over the rows with a label in range, as a mean over all B rows; NaN loss if any label is out of range."""
    i = nll_inputs(c)
    good = np.flatnonzero((i["Y"] >= 0) & (i["Y"] < c.K))
    h, S = T(i["hazards"]).requires_grad_(True), T(i["S"]).requires_grad_(True)
    loss = tp.nll_loss(h[good], S[good], torch.as_tensor(i["Y"][good]), torch.as_tensor(i["c"][good]), alpha=NLL_ALPHA,
                       eps=NLL_EPS) * (len(good) / c.B)
    loss.backward()
    out = dict(loss=float(loss.detach()) if len(good) == c.B else float("nan"), gH=h.grad.numpy(), gS=S.grad.numpy(), good=good)
    # tests/test_gpu_radio_small.py:118 (B <= 16); beyond: a thread's chain of B / 256 rows, then thread 0 adds 256 partials
    if c.B <= 16:
        b_loss = 1e-5
    else:
        hh, SS, Y, rows = np.asarray(i["hazards"], f64), np.asarray(i["S"], f64), i["Y"], good
        sp = np.where(Y[rows] == 0, 1.0, SS[rows, np.maximum(Y[rows] - 1, 0)])
        terms = (np.abs(np.log(np.maximum(sp, NLL_EPS))) + np.abs(np.log(np.maximum(hh[rows, Y[rows]], NLL_EPS)))
                 + np.abs(np.log(np.maximum(SS[rows, Y[rows]], NLL_EPS))))
        b_loss = (-(-c.B // 256) + 256 + 8) * U * float(terms.sum()) / c.B
    # gradients: tests/test_gpu_radio_small.py:123 up to its B = 16.  They carry 1 / B, so beyond that each element is judged
    # against itself: one term, (1 - c) / h / B or (1 - alpha) c / S / B -- 1 / B, a division and two products, 8 ulp; an
    # element the loss does not reach is exactly 0.  (No input near eps: tests/test_abi_shapes_cpu.py.)
    if c.B <= 16:
        bar = dict(loss=b_loss, gH=1e-5 + 1e-4 * np.abs(out["gH"]), gS=1e-5 + 1e-4 * np.abs(out["gS"]))
    else:
        bar = dict(loss=b_loss, gH=8 * U * np.abs(out["gH"]), gS=8 * U * np.abs(out["gS"]))
    return out, bar


# ---- Cox ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cox_inputs(c):
    u = gen.uniform01(31, c.B, stream=c.B % 97)
    times = (np.floor(u * max(c.B // 2, 2)) + 1).astype(f64)               # ties at every B above 2
    if c.B == 2:
        times = np.array([2.0, 1.0])
    cens = np.ones(c.B, np.float32) if c.all_censored else (gen.uniform01(32, c.B, stream=3) < 0.3).astype(np.float32)
    return dict(risks=gen.normal(33, (c.B,), stream=c.B % 89, std=0.7), times=times, c=cens)


def cox_vectorised(risks, times, c):
    """utils/loss_utils.py:124-139 through sorted cumulative sums: (loss, d_risks, D, terms, w sums), all float64.
    D_i = sum_{t_j >= t_i} exp(r_j); loss = -mean((r_i - log D_i) (1 - c_i));
    d_k = -((1 - c_k) - exp(r_k) sum_{t_i <= t_k} (1 - c_i) / D_i) / B."""
    r, t, unc = np.asarray(risks, f64), np.asarray(times, f64), 1 - np.asarray(c, f64)
    B = len(r)
    e = np.exp(r)
    order = np.argsort(t, kind="stable")
    ts = t[order]
    suffix = np.cumsum(e[order][::-1])[::-1]
    D = suffix[np.searchsorted(ts, t, side="left")]
    terms = (r - np.log(D)) * unc
    prefix = np.cumsum((unc / D)[order])
    acc = prefix[np.searchsorted(ts, t, side="right") - 1]
    return -terms.sum() / B, -(unc - e * acc) / B, D, terms, e * acc


@functools.lru_cache(maxsize=None)
def cox_ref(c):
    i = cox_inputs(c)
    loss, d, D, terms, eacc = cox_vectorised(i["risks"], i["times"], i["c"])
    unc = 1 - np.asarray(i["c"], f64)
    if c.B < 1000:                                       # tests/test_gpu_radio_small.py:155-156, set on B up to 300
        bar = dict(loss=1e-5, d_risks=1e-6 + 1e-4 * np.abs(d))
    else:
        # a risk set D_i: a chain of B adds, so log D_i is off by (B + 8) u; the loss: B / 256 rows a thread, then 256 partials.
        # d_k: w_i = unc_i / D_i carries D_i's error, and acc_k is another chain of B
        bar = dict(loss=(-(-c.B // 256) + 256 + 8) * U * float(np.abs(terms).sum()) / c.B + (c.B + 8) * U * float(unc.sum()) / c.B,
                   d_risks=(2 * (c.B + 8) + 8) * U * (unc + eacc) / c.B)
    return dict(loss=float(loss), d_risks=d, D=D), bar


# ---- ranking loss ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rank_inputs(c):
    B = c.B
    risks = gen.normal(41, (B,), stream=B % 83)
    if c.kind == "many":
        times = np.floor(gen.uniform01(42, B, stream=1) * 20).astype(f64)
        cens = (gen.uniform01(43, B, stream=2) < 0.3).astype(np.float32)
    elif c.kind == "none":
        times, cens = np.arange(1.0, B + 1), np.ones(B, np.float32)
    elif c.kind == "one":                                # the only event is the last but one in time: one later sample
        times, cens = np.arange(1.0, B + 1), np.ones(B, np.float32)
        cens[B - 2] = 0
    elif c.kind == "tied":
        times, cens = np.array([1.0, 1.0, 2.0, 2.0, 2.0, 3.0]), np.array([0, 0, 0, 1, 0, 0], np.float32)
    else:                                                # equal risks
        times, cens = np.array([3.0, 1.0, 2.0, 6.0, 5.0, 4.0]), np.zeros(B, np.float32)
        risks = np.array([0.25, 0.25, 0.25, -1.0, 0.5, 0.25], np.float32)
    return dict(risks=risks, times=times, c=cens)


def rank_vectorised(risks, times, c, phi, reduction):
    """utils/loss_utils.py:58-101 over the pair matrix: x is the more risky of {x, y} iff t_x < t_y and x had its event (the
    two branches of the index-ordered rule exclude each other).  -> (loss, d_risks, pairs, sum of phi, A_i = the sum of
    |d phi| over the pairs of sample i), torch float64."""
    r = T(risks).requires_grad_(True)
    t, ev = torch.as_tensor(np.asarray(times, f64)), (1 - T(c)) != 0
    M = (t[:, None] < t[None, :]) & ev[:, None]
    n = int(M.sum())
    diff = r[:, None] - r[None, :]
    v = torch.sigmoid(diff) if phi in (0, "sigmoid") else torch.relu(diff)
    tot = (v * M).sum()
    if n == 0:
        return 0.0, np.zeros(len(risks)), 0, 0.0, np.zeros(len(risks))
    loss = -(tot / n) if reduction in (0, "mean") else -tot
    loss.backward()
    with torch.no_grad():
        d = v * (1 - v) if phi in (0, "sigmoid") else (diff > 0).double()
        A = (d * M).sum(1) + (d * M).sum(0)
    return float(loss.detach()), r.grad.numpy(), n, float(tot.detach()), A.numpy()


@functools.lru_cache(maxsize=None)
def rank_ref(c):
    i = rank_inputs(c)
    loss, d, n, tot, A = rank_vectorised(i["risks"], i["times"], i["c"], c.phi, c.reduction)
    if c.reduction == 0 and c.B <= 300:                  # tests/test_gpu_stage2.py:95-96: mean reduction, B up to 300
        bar = dict(loss=1e-5, d_risks=np.full(c.B, 1e-6))
    else:
        # thread i: a chain of B pairs for each of its B / 256 samples, then the 8 levels of the tree; d_i: a chain of B
        scale = 0.0 if n == 0 else 1.0 / n if c.reduction == 0 else 1.0
        bar = dict(loss=(c.B * -(-c.B // 256) + 8 + 8) * U * tot * scale, d_risks=(c.B + 8) * U * A * scale)
    return dict(loss=loss, d_risks=d, pairs=n), bar


# ---- hazards ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def haz_inputs(c):
    z = gen.normal(51, (c.B, c.K), stream=c.B % 79 + c.K, std=1.5)
    if c.steep:
        z = (z + _steep(c.B, c.K)).astype(np.float32)
    if c.K > 1:                                          # argmax unambiguous: lift the top logit of a row that is nearly tied
        srt = np.sort(z, 1)
        near = (srt[:, -1] - srt[:, -2]) < 1e-2
        z[near, np.argmax(z[near], 1)] += np.float32(0.05)
    return dict(logits=z, gH=gen.normal(52, (c.B, c.K), stream=1), gS=gen.normal(53, (c.B, c.K), stream=2),
                gR=gen.normal(54, (c.B,), stream=3))


@functools.lru_cache(maxsize=None)
def haz_ref(c):
    """oracle.stage2_port.heads on the float64 logits; the backward from the fp32 hazards."""
    i = haz_inputs(c)
    z = np.asarray(i["logits"], f64)
    risk, hz, S = (t.numpy() for t in s2.heads(T(z)))
    out = dict(hazards=hz, S=S, risk=risk, Y_hat=np.argmax(z, 1), h32=r32(hz))
    within = c.B <= 32 and c.K <= 4                      # the stage-2 models: tests/test_gpu_stage2.py:55-58, :60
    if within:
        bar = dict(hazards=np.full_like(hz, 1e-4), S=np.full_like(S, 1e-4), risk=np.full_like(risk, 1e-4))
    else:                                                # h: a few ulp; S_j: j products, |dS_j / dh_u| <= 1; risk: a chain of K
        b_h = 8 * U * hz
        b_S = np.cumsum(b_h, 1) + (np.arange(c.K) + 9) * U * S
        bar = dict(hazards=b_h, S=b_S, risk=b_S.sum(1) + (c.K + 8) * U * S.sum(1))
    h = np.asarray(out["h32"], f64)
    gH = np.asarray(i["gH"], f64) if c.gH else np.zeros_like(h)
    gS = (np.asarray(i["gS"], f64) if c.gS else np.zeros_like(h)) - (np.asarray(i["gR"], f64)[:, None] if c.gR else 0.0)
    P = prod_others(h)
    hh = h * (1 - h)
    out["dlogits"] = (gH - np.einsum("bj,btj->bt", gS, P)) * hh
    if within:
        bar["dlogits"] = np.full_like(h, 2e-5 + 2e-4 * float(np.abs(out["dlogits"]).max()))
    else:                                                # K products of up to K factors, a chain of K
        bar["dlogits"] = (3 * c.K + 8) * U * (np.abs(gH) + np.einsum("bj,btj->bt", np.abs(gS), P)) * hh
    return out, bar


# ---- highway mix -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def highway_inputs(c):
    zn = gen.normal(62, (c.n,), stream=2)
    zn[3::7] = 0.0                                       # exactly on the ReLU kink: relu 0, derivative 0
    return dict(zg=gen.normal(61, (c.n,), stream=1, std=2.0), zn=zn, zl=gen.normal(63, (c.n,), stream=3),
                dy=gen.normal(64, (c.n,), stream=4))


@functools.lru_cache(maxsize=None)
def highway_ref(c):
    zg, zn, zl, dy = (np.asarray(v, f64) for v in (highway_inputs(c)[k] for k in ("zg", "zn", "zl", "dy")))
    g, rn = 1 / (1 + np.exp(-zg)), np.maximum(zn, 0)
    out = dict(y=g * rn + (1 - g) * zl, dzg=dy * (rn - zl) * g * (1 - g), dzn=np.where(zn > 0, dy * g, 0.0), dzl=dy * (1 - g))
    # elementwise, whatever n: the stage-2 models' bars, tests/test_gpu_stage2.py:55 and :60
    bar = dict(y=np.full(c.n, 1e-4))
    bar.update({k: np.full(c.n, 2e-5 + 2e-4 * float(np.abs(out[k]).max())) for k in ("dzg", "dzn", "dzl")})
    return out, bar


# ---- batch norm --------------------------------------------------------------------------------------------------------------
BN_EPS, BN_MOM = 1e-5, 0.1


@functools.lru_cache(maxsize=None)
def bn_inputs(c):
    x = gen.normal(71, (c.B, c.F), stream=c.B % 73 + 1)
    if c.shifted:
        x = (8.0 + x.astype(f64) / 8.0).astype(np.float32)
    return dict(x=x, res=gen.normal(72, (c.B, c.F), stream=2), gamma=(1 + 0.1 * gen.normal(73, (c.F,), stream=3)).astype(np.float32),
                beta=gen.normal(74, (c.F,), stream=4, std=0.1), rm=gen.normal(75, (c.F,), stream=5, std=0.1),
                rv=(1 + 0.1 * np.abs(gen.normal(76, (c.F,), stream=6))).astype(np.float32), dy=gen.normal(77, (c.B, c.F), stream=7),
                keep=gen.keep_mask(SEED, SITE, c.B, c.F, c.drop_p) if c.drop_p > 0 else np.ones((c.B, c.F), bool))


def _bn_forward(c, dtype):
    """torch's batch_norm + residual + activation + dropout in `dtype` -> (y, running_mean, running_var)."""
    i = bn_inputs(c)
    t = lambda k: torch.as_tensor(i[k]).to(dtype).clone()        # batch_norm updates the running statistics in place
    rm, rv = (t("rm"), t("rv")) if c.running else (None, None)
    v = torch.nn.functional.batch_norm(t("x"), rm, rv, t("gamma") if c.affine else None, t("beta") if c.affine else None,
                                       c.training, BN_MOM, BN_EPS)
    if c.res:
        v = v + t("res")
    v = [lambda v: v, torch.relu, torch.tanh, torch.sigmoid, torch.selu][c.act](v)
    if c.drop_p > 0:
        v = v * torch.as_tensor(i["keep"]).to(dtype) / (1 - c.drop_p)
    return v, rm, rv


def _bn_backward(c, dtype, y32, dy):
    """dpre from the fp32 forward output as the kernel derives it, then autograd through torch's batch_norm in `dtype`
    -> (dx, dres = dpre, dgamma, dbeta)."""
    i = bn_inputs(c)
    dydy, y = drop_bwd(y32, i["keep"], 1 if c.drop_p > 0 else 0, c.drop_p)
    dpre = torch.as_tensor(np.asarray(dy, f64) * dydy * act_grad_from_y(y, c.act)).to(dtype)
    t = lambda k: torch.as_tensor(i[k]).to(dtype).clone()        # batch_norm updates the running statistics in place
    x = t("x").requires_grad_(True)
    gamma = (t("gamma") if c.affine else torch.ones(c.F, dtype=dtype)).requires_grad_(True)
    beta = torch.zeros(c.F, dtype=dtype, requires_grad=True)
    rm, rv = (t("rm"), t("rv")) if c.running else (None, None)
    torch.nn.functional.batch_norm(x, rm, rv, gamma, beta, c.training, BN_MOM, BN_EPS).backward(dpre)
    return dict(dx=x.grad.numpy(), dres=dpre.numpy(), dgamma=gamma.grad.numpy(), dbeta=beta.grad.numpy())


@functools.lru_cache(maxsize=None)
def bn_ref(c):
    i = bn_inputs(c)
    x = np.asarray(i["x"], f64)
    y, rm, rv = _bn_forward(c, torch.float64)
    if c.training:
        mean, var = x.mean(0), x.var(0)
    else:
        mean, var = np.asarray(i["rm"], f64), np.asarray(i["rv"], f64)
    invstd = 1 / np.sqrt(var + BN_EPS)
    out = dict(y=y.numpy(), save_mean=mean, save_invstd=invstd, y32=r32(y.numpy()))
    if c.running:
        out.update(running_mean=rm.numpy(), running_var=rv.numpy())
    out.update(_bn_backward(c, torch.float64, out["y32"], i["dy"]))
    # the stage-2 models (B = 32): outputs 1e-4 (tests/test_gpu_stage2.py:55-58), gradients 2e-5 + 2e-4 max|ref| (:60),
    # statistics rtol 1e-5, atol 1e-6 (:64)
    stat = lambda k: 1e-6 + 1e-5 * np.abs(out[k])
    bar = dict(y=np.full_like(x, 1e-4), save_mean=stat("save_mean"), save_invstd=stat("save_invstd"))
    if c.running:
        bar.update(running_mean=stat("running_mean"), running_var=stat("running_var"))
    bar.update({k: np.full_like(out[k], 2e-5 + 2e-4 * float(np.abs(out[k]).max())) for k in ("dx", "dres", "dgamma", "dbeta")})
    if c.B > 32:
        bar = _bn_sum_bounds(c, out)
    if c.shifted:
        # a feature far from zero: the larger of the project's bar and 4 x the error of torch's own fp32 CPU batch_norm
        # against the same float64 reference -- a different summation order deserves that much and no more
        y_f, rm_f, rv_f = _bn_forward(c, torch.float32)
        got = dict(y=y_f.numpy(), running_mean=rm_f.numpy(), running_var=rv_f.numpy(), **_bn_backward(c, torch.float32, out["y32"], i["dy"]))
        for k, v in got.items():
            bar[k] = np.maximum(bar[k], 4 * float(np.abs(np.asarray(v, f64) - out[k]).max()))
    return out, bar


def _bn_sum_bounds(c, out):
    """The summation bound for a training batch beyond the stage-2 B = 32: every per-feature sum is a chain of B."""
    i = bn_inputs(c)
    B, n = c.B, c.B + 8
    x, dy = np.asarray(i["x"], f64), np.asarray(i["dy"], f64)
    g = np.asarray(i["gamma"], f64) if c.affine else np.ones(c.F)
    be = np.asarray(i["beta"], f64) if c.affine else np.zeros(c.F)
    res = np.asarray(i["res"], f64) if c.res else 0.0
    mean, invstd = out["save_mean"], out["save_invstd"]
    d = x - mean
    v = (d * d).sum(0)
    e_mean = n * U * np.abs(x).sum(0) / B
    e_v = n * U * v + 2 * np.abs(d).sum(0) * e_mean + B * e_mean ** 2
    rho = 0.5 * e_v / (v + B * BN_EPS) + 4 * U                                   # relative error of invstd
    xhat = d * invstd
    scale = 1.06 / (1 - c.drop_p)                                                # Lipschitz constant of the activations, dropout scale
    bar = dict(save_mean=e_mean, save_invstd=rho * invstd,
               y=scale * (np.abs(g) * (invstd * e_mean + np.abs(xhat) * rho) + 8 * U * (np.abs(g * xhat) + np.abs(be) + np.abs(res))))
    if c.running:
        bar.update(running_mean=BN_MOM * e_mean + 4 * U * (np.abs(i["rm"]) + np.abs(mean)),
                   running_var=BN_MOM * e_v / (B - 1) + 4 * U * (np.abs(i["rv"]) + v / (B - 1)))
    # backward: mean and invstd arrive rounded to fp32, the reference keeps them in float64
    dpre = out["dres"]
    dydy = np.where(i["keep"], 1 / (1 - c.drop_p), 0.0)
    e_dpre = 8 * U * np.abs(dpre) + 2 * U * np.abs(dy * dydy)
    e_xhat = invstd * U * (np.abs(mean) + 2 * np.abs(x)) + 4 * U * np.abs(xhat)
    b_dbeta = n * U * np.abs(dpre).sum(0) + e_dpre.sum(0)
    b_dgamma = n * U * np.abs(dpre * xhat).sum(0) + (e_dpre * np.abs(xhat) + np.abs(dpre) * e_xhat).sum(0)
    s_d, s_dx = dpre.sum(0), (dpre * xhat).sum(0)
    b_dx = np.abs(g) * invstd * (e_dpre + b_dbeta / B + np.abs(xhat) * b_dgamma / B + e_xhat * np.abs(s_dx) / B
                                + 8 * U * (np.abs(dpre) + np.abs(s_d) / B + np.abs(xhat * s_dx) / B))
    bar.update(dres=e_dpre, dbeta=b_dbeta, dgamma=b_dgamma, dx=b_dx)
    return bar


# ---- Adam + L1 ---------------------------------------------------------------------------------------------------------------
ADAM_HP = dict(lr=np.float32(2e-4), b1=np.float32(0.9), b2=np.float32(0.999), eps=np.float32(1e-8))


@functools.lru_cache(maxsize=None)
def adam_inputs(c, round_=0):
    """w, g, m, v of step c.step + round_: g, m and g' share a sign (m and v do not cancel), |g| >= 0.5; the last elements
    element and, from n = 4, element 1 are pad-like: w = +0 and -0 with g = m = v = 0.  The mask has a 0 and a 1 on live
    elements of a tail of three, and (drawn) of the vector part."""
    n = c.n
    sign = np.where(gen.uniform01(81, n, stream=1) < 0.5, -1.0, 1.0)
    g = (sign * (0.5 + gen.uniform01(82, n, stream=2 + round_))).astype(np.float32)
    w = gen.normal(83, (n,), stream=3, std=0.1)
    m = (g * (0.05 + 0.4 * gen.uniform01(84, n, stream=4))).astype(np.float32)
    v = (g.astype(f64) ** 2 * (0.5 + gen.uniform01(85, n, stream=5))).astype(np.float32)
    mask = (gen.uniform01(86, n, stream=6) < 0.5).astype(np.float32)
    zeros = np.zeros(n, bool)
    if n >= 3:
        zeros[n - 1] = True
    if n >= 4:
        zeros[1] = True
    for a in (g, w, m, v):
        a[zeros] = 0.0
    if n >= 4:
        w[1] = -0.0
    if n % 4 == 3:
        mask[n - 3], mask[n - 2] = 0.0, 1.0
    return dict(w=w, g=g, m=m, v=v, mask=mask, zeros=zeros)


def adam_step_ref(c, w, g, m, v, mask, step):
    """torch.optim.Adam in float64 on g + l1 * mask * sign(w), from the given fp32 state -> (w, m, v) and the bars:
    m and v relative at 16 * 2^-24; w at one ulp of w plus 16 ulp of the update."""
    hp = {k: float(x) for k, x in ADAM_HP.items()}
    wd, l1 = float(np.float32(c.wd)), float(np.float32(c.l1))
    p = torch.nn.Parameter(T(w))
    opt = torch.optim.Adam([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=T(m).clone(), exp_avg_sq=T(v).clone())
    p.grad = T(g) + l1 * (T(mask) if c.mask else 1.0) * torch.sign(T(w))
    opt.step()
    st = opt.state[p]
    w1, m1, v1 = p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    update = np.asarray(w, f64) - w1
    ulp_w = np.spacing(np.abs(np.asarray(w1, np.float32))).astype(f64)
    return dict(w=w1, m=m1, v=v1), dict(w=ulp_w + 16 * U * np.abs(update), m=16 * U * np.abs(m1), v=16 * U * np.abs(v1))


# ---- abs_sum -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abs_sum_inputs(c):
    return gen.normal(91, (c.n,), stream=c.n % 71)


@functools.lru_cache(maxsize=None)
def abs_sum_ref(c):
    s = float(np.abs(np.asarray(abs_sum_inputs(c), f64)).sum())
    return s, (ab.abs_sum_chain(c.n) + 8) * U * s


# ---- dense backward ------------------------------------------------------------------------------------------------------------
def dense_row_seeds(c):
    return [100 + 7 * b for b in range(c.B)]


@functools.lru_cache(maxsize=None)
def dense_inputs(c):
    p = P_DROP if c.drop_kind else 0.0
    if not c.drop_kind:
        keep = np.ones((c.B, c.N), bool)
    elif c.rows:          # row b draws the mask a one-row call with its own seed draws (include/mmf_amil.h mmf_dense_forward_rows)
        keep = np.concatenate([gen.keep_mask(s, SITE, 1, c.N, p) for s in dense_row_seeds(c)], 0)
    else:
        keep = gen.keep_mask(SEED, SITE, c.B, c.N, p)
    return dict(x=gen.normal(101, (c.B, c.K), stream=c.K), W=gen.normal(102, (c.N, c.K), stream=c.N % 67, std=1.0 / np.sqrt(c.K)),
                b=gen.normal(103, (c.N,), stream=1, std=0.1), dy=gen.normal(104, (c.B, c.N), stream=2), keep=keep, p=p)


@functools.lru_cache(maxsize=None)
def dense_ref(c):
    i = dense_inputs(c)
    x, W, b, dy = (np.asarray(i[k], f64) for k in ("x", "W", "b", "dy"))
    pre = x @ W.T + b
    y_act = act_ref(pre, c.act)
    y32 = r32(drop_fwd(y_act, i["keep"], c.drop_kind, i["p"]))
    dydy, y = drop_bwd(y32, i["keep"], c.drop_kind, i["p"])
    dpre = dy * dydy * act_grad_from_y(y, c.act)
    out = dict(y32=y32, y_act=y_act, y_rec=y, dpre=dpre, dx=dpre @ W, dW=dpre.T @ x, db=dpre.sum(0))
    # every case lies beyond the sizes of tests/test_gpu_omic_mm.py:144-159 (B <= 128, N <= 512): the summation bound.
    # dpre: a few ulp of itself; SELU's negative side adds the fp32 constant scale * alpha to y, and AlphaDropout recovers y
    # as (yd - b) / a: absolute errors of a few ulp of the operands, whatever is left of the difference
    a_aff, b_aff, _ = alpha_affine(i["p"]) if c.drop_kind == 2 else (1.0, 0.0, 0.0)
    e_y = 4 * U * (np.abs(y32) + abs(b_aff)) / a_aff if c.drop_kind == 2 else 0.0
    e_act = {0: 0.0, 1: 0.0, 4: np.where(y > 0, 0.0, e_y + 4 * U * SELU_SCALE * SELU_ALPHA)}[c.act]
    e_dpre = 8 * U * np.abs(dpre) + np.abs(dy * dydy) * e_act
    fused = ab.dense_bwd_path(c).startswith("fused")
    n_dx = -(-c.N // 16) + 4 if fused else c.N // 2 + 2          # four slices of N / 4, four accumulators each | two accumulators
    aW, ax = np.abs(W), np.abs(x)
    bar = dict(dx=(n_dx + 8) * U * (np.abs(dpre) @ aW) + e_dpre @ aW, dW=(c.B + 8) * U * (np.abs(dpre).T @ ax) + e_dpre.T @ ax,
               db=(c.B + 8) * U * np.abs(dpre).sum(0) + e_dpre.sum(0), dpre=e_dpre)
    return out, bar


# ==== the dense forward, gate_mul, kron and xreduce (tests/test_gpu_tail_shapes.py) ==========================================
def _drop_out_bar(e_y, y, yd, kind, p):
    """The bar of drop(y) from the bar e_y of y: nn.Dropout divides by 1 - p, AlphaDropout is a * y + b -- the error of y
    scaled, plus 8 ulp of what the last operation adds up (|a y| + |b| for the affine form)."""
    if kind == 0:
        return e_y
    if kind == 1:
        return e_y / (1 - p) + 8 * U * np.abs(yd)
    a, b, alpha_p = alpha_affine(p)
    return a * e_y + 8 * U * (np.abs(a * y) + abs(b) + abs(a * alpha_p))


# ---- dense forward -------------------------------------------------------------------------------------------------------------
def dense_fwd_row_seeds(c):
    return [100 + 7 * b for b in range(c.B)]


@functools.lru_cache(maxsize=None)
def dense_fwd_inputs(c):
    p = c.drop_p if c.drop_kind else 0.0
    if not c.drop_kind:
        keep = np.ones((c.B, c.N), bool)
    elif c.rows:          # row b: the mask a one-row call with seed_b draws at index n (include/mmf_amil.h mmf_dense_forward_rows)
        keep = np.concatenate([gen.keep_mask(s, SITE, 1, c.N, p) for s in dense_fwd_row_seeds(c)], 0)
    else:
        keep = gen.keep_mask(SEED, SITE, c.B, c.N, p)
    return dict(x=gen.normal(111, (c.B, c.K), stream=c.K), W=gen.normal(112, (c.N, c.K), stream=c.N % 67, std=1.0 / np.sqrt(c.K)),
                b=gen.normal(113, (c.N,), stream=1, std=0.3), keep=keep, p=p)


def dense_fwd_chain(K):
    """The longest add chain of one output of dense_fwd_kernel: accumulator a0 takes K / 256 unrolled rounds and up to three
    tail steps, then (a0 + a1) + (a2 + a3), wave_sum (6) and the bias."""
    return K // 256 + 3 + 2 + 6 + 1


@functools.lru_cache(maxsize=None)
def dense_fwd_ref(c):
    i = dense_fwd_inputs(c)
    x, W = np.asarray(i["x"], f64), np.asarray(i["W"], f64)
    b = np.asarray(i["b"], f64) if c.bias else np.zeros(c.N)
    pre = x @ W.T + b
    e_pre = (dense_fwd_chain(c.K) + 8) * U * (np.abs(x) @ np.abs(W).T + np.abs(b))
    y = act_ref(pre, c.act)
    # |act'| <= 1 for none / relu / tanh / sigmoid; SELU: scale above zero, scale * alpha * e^v <= scale * alpha below
    slope = {0: 1.0, 1: 1.0, 2: 1.0, 3: 0.25, 4: SELU_SCALE * SELU_ALPHA}[c.act]
    e_y = slope * e_pre + (8 * U * (np.abs(y) + (SELU_SCALE * SELU_ALPHA if c.act == 4 else 0.0)) if c.act >= 2 else 0.0)
    yd = drop_fwd(y, i["keep"], c.drop_kind, i["p"])
    return dict(y=yd, y_act=y), dict(y=_drop_out_bar(e_y, y, yd, c.drop_kind, i["p"]))


# ---- gate_mul ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_mul_inputs(c):
    return dict(z=gen.normal(121, (c.n,), stream=c.n % 61, std=2.0), h=gen.normal(122, (c.n,), stream=1), g=gen.normal(123, (c.n,), stream=2))


@functools.lru_cache(maxsize=None)
def gate_mul_ref(c):
    i = gate_mul_inputs(c)
    z, h, g = (np.asarray(i[k], f64) for k in ("z", "h", "g"))
    s = 1 / (1 + np.exp(-z))
    out = dict(o=s * h, dz=g * h * s * (1 - s), dh=g * s)
    # single terms: 8 ulp; dz holds 1 - s, where the 4 ulp of s (expf, the add, the division) are absolute: |g h| 4U s on top
    bar = dict(o=8 * U * np.abs(out["o"]), dh=8 * U * np.abs(out["dh"]), dz=8 * U * np.abs(out["dz"]) + np.abs(g * h) * 4 * U * s)
    return out, bar


# ---- kron ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kron_inputs(c):
    S = c.dim + 1
    o = [gen.normal(131 + t, (c.B, c.dim), stream=c.dim % 59) for t in range(c.m)]
    keep = gen.keep_mask(SEED, SITE, c.B, S ** c.m, c.drop_p) if c.drop_p > 0 else np.ones((c.B, S ** c.m), bool)
    return dict(o=o, g=gen.normal(135, (c.B, S ** c.m), stream=c.m), keep=keep)


@functools.lru_cache(maxsize=None)
def kron_ref(c):
    i = kron_inputs(c)
    S = c.dim + 1
    ext = [np.concatenate([np.asarray(o, f64), np.ones((c.B, 1))], 1) for o in i["o"]]
    scale = np.where(i["keep"], 1 / (1 - c.drop_p), 0.0) if c.drop_p > 0 else np.ones((c.B, S ** c.m))
    letters = "ijk"[:c.m]
    full = np.einsum(",".join("b" + l for l in letters) + "->b" + letters, *ext).reshape(c.B, -1)
    out = dict(out=full * scale)
    bar = dict(out=8 * U * np.abs(out["out"]))
    gs = (np.asarray(i["g"], f64) * scale).reshape((c.B,) + (S,) * c.m)
    n_chain = -(-(S ** (c.m - 1)) // 64) + 6            # a lane's share of the others, then wave_sum
    for t in range(c.m):
        rest = [ext[u] for u in range(c.m) if u != t]
        rl = [letters[u] for u in range(c.m) if u != t]
        spec = "b" + letters + "," + ",".join("b" + l for l in rl) + "->b" + letters[t]
        out[f"d{t}"] = np.einsum(spec, gs, *rest)[:, :c.dim]
        bar[f"d{t}"] = (n_chain + 8) * U * np.einsum(spec, np.abs(gs), *[np.abs(r) for r in rest])[:, :c.dim]
    return out, bar


# ---- xreduce -----------------------------------------------------------------------------------------------------------------------
XR_KEYS = ("Wh", "bh", "Wz", "bz", "Wo", "bo")


@functools.lru_cache(maxsize=None)
def xreduce_inputs(c):
    m, B, dim, S = c.m, c.B, c.dim, c.sdim
    st = (dim + 3 * S) % 53
    i = dict(v=[gen.normal(141 + t, (B, dim), stream=st) for t in range(m)],
             Wh=[gen.normal(145 + t, (S, dim), stream=st, std=1 / np.sqrt(dim)) for t in range(m)],
             bh=[0.5 + gen.normal(149 + t, (S,), stream=st, std=0.3) for t in range(m)],      # shifted: a one-unit stage still has a live unit
             Wz=[gen.normal(153 + t, (S, m * dim), stream=st, std=1 / np.sqrt(m * dim)) for t in range(m)],
             bz=[gen.normal(157 + t, (S,), stream=st, std=0.3) for t in range(m)],
             Wo=[gen.normal(161 + t, (S, S), stream=st, std=1 / np.sqrt(S)) for t in range(m)],
             bo=[0.5 + gen.normal(165 + t, (S,), stream=st, std=0.3) for t in range(m)],
             d_o=[gen.normal(169 + t, (B, S), stream=st) for t in range(m)])
    # site t of the seed, element b * sdim + j (csrc/mmf_mlp.hip site_drop)
    i["keep"] = [gen.keep_mask(SEED, t, B, S, c.drop_p) if c.drop_p > 0 else np.ones((B, S), bool) for t in range(m)]
    return i


def _wave_dot_chain(dim):
    return 4 * (-(-dim // 256))                # a lane's rounds, four adds each (three inside the float4, one onto acc)


@functools.lru_cache(maxsize=None)
def xreduce_ref(c):
    i = xreduce_inputs(c)
    m, B, dim, S, p = c.m, c.B, c.dim, c.sdim, c.drop_p
    A = lambda k: [np.asarray(a, f64) for a in i[k]]
    v, Wh, bh, Wz, bz, Wo, bo, d_o = (A(k) for k in ("v", "Wh", "bh", "Wz", "bz", "Wo", "bo", "d_o"))
    vcat = np.concatenate(v, 1)
    nh, nz = _wave_dot_chain(dim) + 7, m * (_wave_dot_chain(dim) + 1) + 7          # + wave_sum (6) + the bias
    out, bar = {}, {}
    for t in range(m):
        hp = v[t] @ Wh[t].T + bh[t]
        h = np.maximum(hp, 0)
        e_h = (nh + 8) * U * (np.abs(v[t]) @ np.abs(Wh[t]).T + np.abs(bh[t]))
        z = vcat @ Wz[t].T + bz[t]
        e_z = (nz + 8) * U * (np.abs(vcat) @ np.abs(Wz[t]).T + np.abs(bz[t]))
        s = 1 / (1 + np.exp(-z))
        gm = s * h
        e_gm = 8 * U * np.abs(gm) + h * s * (1 - s) * e_z + s * e_h
        op = gm @ Wo[t].T + bo[t]
        e_op = (S + 1 + 8) * U * (np.abs(gm) @ np.abs(Wo[t]).T + np.abs(bo[t])) + e_gm @ np.abs(Wo[t]).T
        o = np.maximum(op, 0)
        od = np.where(i["keep"][t], o / (1 - p), 0.0) if p > 0 else o
        out.update({f"h{t}": h, f"z{t}": z, f"gm{t}": gm, f"o{t}": od, f"hp{t}": hp, f"op{t}": op})
        bar.update({f"h{t}": e_h, f"z{t}": e_z, f"gm{t}": e_gm, f"o{t}": np.where(i["keep"][t], e_op / (1 - p) + 8 * U * np.abs(od), 0.0)})
    # backward, from the forward outputs rounded to fp32 (what the kernel is given)
    h32, z32, gm32, o32 = ([r32(out[f"{k}{t}"]) for t in range(m)] for k in ("h", "z", "gm", "o"))
    out.update(h32=h32, z32=z32, gm32=gm32, o32=o32)
    dz, dph, e_dz, e_dph = [], [], [], []
    for t in range(m):
        hh, zz, gg, oo = (np.asarray(a[t], f64) for a in (h32, z32, gm32, o32))
        dydy = np.where(i["keep"][t], 1 / (1 - p), 0.0) if p > 0 else np.ones((B, S))
        dpo = d_o[t] * dydy * (oo > 0)
        e_dpo = 8 * U * np.abs(dpo)
        dgm = dpo @ Wo[t]
        e_dgm = (S + 8) * U * (np.abs(dpo) @ np.abs(Wo[t])) + e_dpo @ np.abs(Wo[t])
        s = 1 / (1 + np.exp(-zz))
        dz.append(dgm * hh * s * (1 - s))
        e_dz.append(8 * U * np.abs(dz[t]) + e_dgm * np.abs(hh) * s * (1 - s) + np.abs(dgm * hh) * 4 * U * s)
        dph.append(np.where(hh > 0, dgm * s, 0.0))
        e_dph.append(np.where(hh > 0, 8 * U * np.abs(dph[t]) + e_dgm * s, 0.0))
        out[f"dWo{t}"], bar[f"dWo{t}"] = dpo.T @ gg, (B + 8) * U * (np.abs(dpo).T @ np.abs(gg)) + e_dpo.T @ np.abs(gg)
        out[f"dbo{t}"], bar[f"dbo{t}"] = dpo.sum(0), (B + 8) * U * np.abs(dpo).sum(0) + e_dpo.sum(0)
        out[f"dbh{t}"], bar[f"dbh{t}"] = dph[t].sum(0), (B + 8) * U * np.abs(dph[t]).sum(0) + e_dph[t].sum(0)
        out[f"dbz{t}"], bar[f"dbz{t}"] = dz[t].sum(0), (B + 8) * U * np.abs(dz[t]).sum(0) + e_dz[t].sum(0)
        out[f"dWh{t}"], bar[f"dWh{t}"] = dph[t].T @ v[t], (B + 8) * U * (np.abs(dph[t]).T @ np.abs(v[t])) + e_dph[t].T @ np.abs(v[t])
        out[f"dWz{t}"], bar[f"dWz{t}"] = dz[t].T @ vcat, (B + 8) * U * (np.abs(dz[t]).T @ np.abs(vcat)) + e_dz[t].T @ np.abs(vcat)
    for t in range(m):      # dv_t = dph_t Wh_t + sum_i dz_i Wz_i[:, block t]: chains of S, then the m partial sums onto acc
        blk = slice(t * dim, (t + 1) * dim)
        out[f"dv{t}"] = dph[t] @ Wh[t] + sum(dz[u] @ Wz[u][:, blk] for u in range(m))
        mag = np.abs(dph[t]) @ np.abs(Wh[t]) + sum(np.abs(dz[u]) @ np.abs(Wz[u][:, blk]) for u in range(m))
        bar[f"dv{t}"] = (S + m + 8) * U * mag + e_dph[t] @ np.abs(Wh[t]) + sum(e_dz[u] @ np.abs(Wz[u][:, blk]) for u in range(m))
    return out, bar


XR_FWD_KEYS = ("h", "z", "gm", "o")
XR_BWD_KEYS = ("dv", "dWh", "dbh", "dWz", "dbz", "dWo", "dbo")


# ---- the omic step (mmf_maxnet_cox_step) ---------------------------------------------------------------------------------------
MX_SEED = 4242
MX_SPREAD, MX_BIAS = 1.2, 2.0          # the largest |x . W^T| of a layer after scaling W; |b| in units of that spread


def _selu_drop(pre, keep, p):
    y = act_ref(pre, 4)
    return y, (drop_fwd(y, keep, 2, p) if p > 0 else y)


@functools.lru_cache(maxsize=None)
def maxstep_inputs(c):
    """A state dict of the case's own: in each layer the weights are scaled so that the largest |in . W^T| of the float64
    reference is MX_SPREAD, and feature n has the bias (-1)^n (layer 0) or -(-1)^n (layer 1) times MX_BIAS spreads.  Every
    pre-activation then lies between 1 and 3 spreads from zero on its feature's side: far from SELU's kink, both branches
    in every row, and the negative ones above -3.6, where y + scale * alpha is well above its rounding."""
    B, G, p = c.B, c.G, c.p_drop
    x = gen.normal(201, (B, G), stream=G % 47)
    sign = np.where(np.arange(256) % 2 == 0, 1.0, -1.0)
    W0 = gen.normal(202, (256, G), stream=G % 43)
    W0 = (W0 * (MX_SPREAD / np.abs(np.asarray(x, f64) @ np.asarray(W0, f64).T).max())).astype(np.float32)
    s0 = np.abs(np.asarray(x, f64) @ np.asarray(W0, f64).T).max()
    b0 = (sign * MX_BIAS * s0).astype(np.float32)
    seed = (MX_SEED + c.word) & 0xFFFFFFFF
    keep0 = gen.keep_mask(seed, 0, B, 256, p) if p > 0 else np.ones((B, 256), bool)
    keep1 = gen.keep_mask(seed, 1, B, 256, p) if p > 0 else np.ones((B, 256), bool)
    _, y0d = _selu_drop(np.asarray(x, f64) @ np.asarray(W0, f64).T + b0, keep0, p)
    W1 = gen.normal(203, (256, 256), stream=B % 41)
    W1 = (W1 * (MX_SPREAD / np.abs(y0d @ np.asarray(W1, f64).T).max())).astype(np.float32)
    s1 = np.abs(y0d @ np.asarray(W1, f64).T).max()
    b1 = (-sign * MX_BIAS * s1).astype(np.float32)
    Wc = gen.normal(204, (1, 256), stream=3, std=1 / 16)
    bc = np.array([0.1], np.float32)
    u = gen.uniform01(205, B, stream=B % 37)
    times = (np.argsort(np.argsort(u)) + 1).astype(f64)                     # distinct
    cens = (gen.uniform01(206, B, stream=5) < 0.3).astype(np.float32)
    if c.censor == "none":
        cens[:] = 0
    elif c.censor == "all":
        cens[:] = 1
    elif c.censor == "tied":
        times = (np.floor(u * 3) + 1).astype(f64)
        cens[0] = 0
    elif c.censor == "last event":
        cens[:] = 1
        cens[int(np.argmax(times))] = 0
    prior = {k: gen.normal(210 + j, shape, stream=1, std=0.01) for j, (k, shape) in enumerate(
        dict(dW0=(256, G), db0=(256,), dW1=(256, 256), db1=(256,), dWc=(1, 256), dbc=(1,)).items())} if c.accumulate else None
    return dict(x=x, W0=W0, b0=b0, W1=W1, b1=b1, Wc=Wc, bc=bc, times=times, c=cens, keep0=keep0, keep1=keep1, prior=prior)


def maxstep_state_dict(i):
    return {"fc_omic.0.0.weight": i["W0"], "fc_omic.0.0.bias": i["b0"], "fc_omic.1.0.weight": i["W1"], "fc_omic.1.0.bias": i["b1"],
            "classifier.weight": i["Wc"], "classifier.bias": i["bc"]}


def _selu_bars(pre, e_pre, y, yd, keep, p):
    """Bars of y = selu(pre) and of its AlphaDropout from the bar of pre: SELU's slope (scale above zero, scale * alpha *
    e^v below, taken at the near end of the bar) times e_pre, and 8 ulp of what the last operation adds up."""
    SA = SELU_SCALE * SELU_ALPHA
    slope = np.where(pre > 0, SELU_SCALE, SA * np.exp(np.minimum(pre + e_pre, 0)))
    e_y = slope * e_pre + 8 * U * (np.abs(y) + np.where(pre > 0, 0.0, SA))
    if p == 0:
        return e_y, e_y
    a, b, alpha_p = alpha_affine(p)
    return e_y, np.where(keep, a * e_y, 0.0) + 8 * U * (np.abs(a * np.where(keep, y, alpha_p)) + abs(b))


def _selu_grad_bars(y, e_y, yd, keep, p):
    """(dydy, selu'(y), bar of selu'(y)) as the kernel derives them from its own dropped output: y recovered as (yd - b) / a,
    then y + scale * alpha below zero -- the error of y, 4 ulp of the recovery's operands and of the constant."""
    SA = SELU_SCALE * SELU_ALPHA
    if p > 0:
        a, b, _ = alpha_affine(p)
        dydy, e_rec = np.where(keep, a, 0.0), e_y + 4 * U * (np.abs(yd) + abs(b)) / a
    else:
        dydy, e_rec = np.ones_like(y), e_y
    sg = np.where(y > 0, SELU_SCALE, y + SA)
    return dydy, sg, np.where(y > 0, 0.0, e_rec + 4 * U * SA)


@functools.lru_cache(maxsize=None)
def maxstep_ref(c):
    """-> (out, bar, facts).  out: risk, loss and the six gradients (of loss * loss_scale, on top of the prior values under
    accumulate) in float64; bar: the summation bound of each, cut at the bar tests/test_gpu_maxnet_step.py:30-35 holds
    (1e-5 max(1, |loss|); 1e-4 on risks; 1e-5 + 1e-4 max|g| on gradients).  Under accumulate the cut applies to the gradient's
    own error, and the one rounding of the add onto the known value, 2^-24 (|prior| + |g|), comes on top: that case's bar may
    sit that much above the existing one.  Chains, read from csrc/mmf_maxnet.hip:
      layer 0   four accumulators of G / 4 k each, up to three more steps on the first in a ragged chunk, (0 + 1) + (2 + 3), bias
      layer 1   four accumulators of 64, the two adds, the bias: 67         risk  wave_sum (6), the four waves (3), bc: 10
      D_i       four accumulators over B / 4 members, three tail steps, two adds      loss  wave_sum, four waves, 1 / B: 10
      a_k       64 threads over B / 64 members each, six shuffles            dbc   wave_sum, four waves: 9
      dWc       a workgroup's four rows, the shares in eight interleaved sums of NW / 8, three adds
      dy0       four accumulators of 64, two adds: 66        dW1  two accumulators over B / 2 rows, one add
      db1, db0  16 lanes over B / 16 rows, four shuffles      dW0  256 / G parts over B / parts rows each, then the parts in order"""
    i = maxstep_inputs(c)
    B, G, p = c.B, c.G, c.p_drop
    x, W0, b0, W1, b1, Wc, bc = (np.asarray(i[k], f64) for k in ("x", "W0", "b0", "W1", "b1", "Wc", "bc"))
    Wc = Wc.reshape(-1)
    k0, k1 = i["keep0"], i["keep1"]
    # forward
    pre0 = x @ W0.T + b0
    e_pre0 = (G // 4 + 3 + 3 + 8) * U * (np.abs(x) @ np.abs(W0).T + np.abs(b0))
    y0, y0d = _selu_drop(pre0, k0, p)
    e_y0, e_y0d = _selu_bars(pre0, e_pre0, y0, y0d, k0, p)
    pre1 = y0d @ W1.T + b1
    e_pre1 = (67 + 8) * U * (np.abs(y0d) @ np.abs(W1).T + np.abs(b1)) + e_y0d @ np.abs(W1).T
    y1, y1d = _selu_drop(pre1, k1, p)
    e_y1, e_y1d = _selu_bars(pre1, e_pre1, y1, y1d, k1, p)
    risk = y1d @ Wc + bc[0]
    e_risk = (10 + 8) * U * (np.abs(y1d) @ np.abs(Wc) + abs(bc[0])) + e_y1d @ np.abs(Wc)
    # Cox
    t, unc = np.asarray(i["times"], f64), 1 - np.asarray(i["c"], f64)
    R = (t[None, :] >= t[:, None]).astype(f64)                              # R[i, j] = t_j >= t_i
    et = np.exp(risk)
    e_et = et * (e_risk + 4 * U)
    D = R @ et
    e_D = (-(-B // 4) + 3 + 2 + 8) * U * D + R @ e_et
    lterm = (risk - np.log(D)) * unc
    e_l = unc * (e_risk + e_D / D + 4 * U * np.abs(np.log(D)) + 4 * U * np.abs(risk - np.log(D)))
    loss = -lterm.sum() / B
    e_loss = ((10 + 8) * U * np.abs(lterm).sum() + e_l.sum()) / B
    wq = unc / D
    e_wq = wq * (e_D / D + 4 * U)
    acc = R.T @ wq                                                          # a_k = sum_i [t_k >= t_i] w_i
    e_acc = (-(-B // 64) + 6 + 8) * U * acc + R.T @ e_wq
    ls = float(np.float32(c.loss_scale))
    dr = -(unc - et * acc) / B * ls
    e_dr = (et * e_acc + acc * e_et + 8 * U * (unc + et * acc)) / B * ls
    # backward
    NW = ab.maxstep_workgroups(B)
    g = dict(dbc=np.array([dr.sum()]), dWc=(dr @ y1d)[None, :])
    e = dict(dbc=np.array([(9 + 8) * U * np.abs(dr).sum() + e_dr.sum()]),
             dWc=((4 + NW // 8 + 3 + 8) * U * (np.abs(dr) @ np.abs(y1d)) + e_dr @ np.abs(y1d) + np.abs(dr) @ e_y1d)[None, :])
    dydy1, sg1, e_sg1 = _selu_grad_bars(y1, e_y1, y1d, k1, p)
    dpre1 = dr[:, None] * Wc[None, :] * dydy1 * sg1
    e_dpre1 = np.abs(Wc[None, :] * dydy1) * (e_dr[:, None] * np.abs(sg1) + np.abs(dr)[:, None] * e_sg1) + 8 * U * np.abs(dpre1)
    n_db = -(-B // 16) + 4
    g["db1"], e["db1"] = dpre1.sum(0), (n_db + 8) * U * np.abs(dpre1).sum(0) + e_dpre1.sum(0)
    g["dW1"] = dpre1.T @ y0d
    e["dW1"] = (B // 2 + 2 + 8) * U * (np.abs(dpre1).T @ np.abs(y0d)) + e_dpre1.T @ np.abs(y0d) + np.abs(dpre1).T @ e_y0d
    dy0 = dpre1 @ W1
    e_dy0 = (66 + 8) * U * (np.abs(dpre1) @ np.abs(W1)) + e_dpre1 @ np.abs(W1)
    dydy0, sg0, e_sg0 = _selu_grad_bars(y0, e_y0, y0d, k0, p)
    dpre0 = dy0 * dydy0 * sg0
    e_dpre0 = np.abs(dydy0) * (e_dy0 * np.abs(sg0) + np.abs(dy0) * e_sg0) + 8 * U * np.abs(dpre0)
    g["db0"], e["db0"] = dpre0.sum(0), (n_db + 8) * U * np.abs(dpre0).sum(0) + e_dpre0.sum(0)
    parts = 256 // G
    g["dW0"], e["dW0"] = dpre0.T @ x, (-(-B // parts) + parts + 8) * U * (np.abs(dpre0).T @ np.abs(x)) + e_dpre0.T @ np.abs(x)
    out = dict(risk=risk, loss=float(loss))
    bar = dict(risk=np.minimum(e_risk, 1e-4), loss=min(float(e_loss), 1e-5 * max(1.0, abs(float(loss)))))
    for k in g:
        old = 1e-5 + 1e-4 * float(np.abs(g[k]).max())
        if c.accumulate:                                                    # one more add, onto the known value
            prior = np.asarray(i["prior"][k], f64)
            out[k], bar[k] = prior + g[k], np.minimum(e[k], old) + U * (np.abs(prior) + np.abs(g[k]))
        else:
            out[k], bar[k] = g[k], np.minimum(e[k], old)
    facts = dict(kink0=float((np.abs(pre0) / e_pre0).min()), kink1=float((np.abs(pre1) / e_pre1).min()),
                 branches=[bool((q > 0).any() and (q < 0).any()) for q in (pre0, pre1)], min_pre=float(min(pre0.min(), pre1.min())),
                 masks=[bool(k.any() and not k.all()) for k in (k0, k1)], loose={k: float((e[k] > 1e-5 + 1e-4 * np.abs(g[k]).max()).mean()) for k in g},
                 pure=dict(loss=float(loss), **g))
    return out, bar, facts


MX_GRADS = ("dW0", "db0", "dW1", "db1", "dWc", "dbc")
