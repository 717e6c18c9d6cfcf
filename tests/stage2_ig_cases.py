"""Cases, float64 oracle and error bars of the stage-2 integrated-gradients tests (helper module, not collected by pytest).
tests/test_stage2_ig_cases_cpu.py checks the caps and BOUND on these very arrays; tests/test_gpu_stage2_ig.py runs the
kernels on them.

Weights: oracle.stage2_port.state_dict_for over the shapes of the model's own state_dict (the classes fix the widths);
inputs: oracle.stage2_port.batch_for, the three [P x 256] embeddings (forward evaluates the modality a late type's mode
drops too; it gets no alpha and no gradient).

Oracle.  Integrated gradients by the definition: for every node alpha_k (the fp32 value the kernels get) one autograd pass
in float64 over oracle.stage2_port.forward (imported; m["train"] = False, masks = None) on alpha_k * every present input,
the P patients as the batch (a row's risk depends on that row alone), attr = input * sum_k w_k d risk / d(alpha_k input).
Computed once per case (lru_cache) and never modified.

ReLU kinks, the rule of tests/mm_tensor_ig_cases.py: a unit whose float64 pre-activation lies within BOUND of 0 at a
(patient, node) is FLAGGED, and for a (patient, node) with f flagged units the oracle holds the node's gradient under all 2^f
assignments of those units' derivatives (the forward recomputed with the ReLU's mask forced: y = u * mask, so the forward
value moves by at most |u| <= BOUND).  The GPU result of a patient must lie within the plain bar -- 1e-4 * max|oracle| per
array, 1e-4 per risk -- of ONE combination of per-node assignments, the same for every array of the call (match).  Caps,
conditions on the committed seeds and never to be changed: at most NODE_CAP = 3 flagged units per (patient, node) and
CASE_CAP = 10 per case; the seeds were picked so that the float64 forward alone stays within both.

BOUND, from the kernels' code (csrc/mmf_stage2_ig.hip; kronecker: csrc/mmf_mlp.hip as tests/mm_tensor_ig_cases.py reads it),
U = 2^-24, a worst case without cancellation: d U (sum |w x| + |b|) with d the dependent roundings on the longest path.
  fcnn     y = s (alpha Uj + b0) + t.  stage2_fold_fwd_kernel: a lane adds ceil(kin / 64) fused products, the butterfly 6:
           d = ceil(kin / 64) + 6, + 2 slack, on alpha sum |W0 v|; the constants' row is 0 W + b0, one rounding, + 1 slack;
           the sweep's two fused multiply-adds and s, t themselves (a division, a square root, a product, a difference: 4
           ulps of |s u| and of |bias| + |mean s|, which t = bias - mean s is rounded against).
                                  BOUND = U (|s| (alpha (d + 2) sum |W0 v| + 2 |b0|) + 4 (|s u| + |bias| + |mean s|))
  highway  zn = alpha Un + cn, Un = (v . s1) Wn^T, cn = t1 Wn^T + bn: the operand v s1 carries 4 ulps (s1's three and the
           product), t1 four of |bias1| + |mean1 s1|, the constants' sum d + 1 and 2 slack, the sweep's fused multiply-add
           one of |zn| and one slack:
             BOUND = U (alpha (d + 6) sum |Wn s1 v| + (d + 3) (sum |Wn t1| + |bn|) + 4 sum |Wn| (|bias1| + |mean1 s1|) + 2 |zn|)
           the same for zg and zl of layer 0 with their weights.  Layers >= 1 (dense_fwd_kernel, csrc/mmf_mlp.hip: per lane
           ceil(K / 256) products and additions into four accumulators, two additions to join them, the butterfly 6, the
           bias: d = 2 ceil(K / 256) + 9, + 2 slack) on the mix x = g relu(zn) + (1 - g) zl of the layer before, whose own
           error -- dz_g |relu(zn) - zl| / 4 + dz_n g + dz_l (1 - g) + 6 U (|g relu(zn)| + |(1 - g) zl|): the sigmoid's slope,
           expf, the division, two products and the sum -- is carried behind W in squares, as tests/mm_tensor_ig_cases.py does.
  kronecker  h_i, o_i, e1, e2 as tail_bounds of tests/mm_tensor_ig_cases.py (dim = 256: it = 1; the classifier has no ReLU),
           the embedding's own error being the expansion's one rounding, U |alpha v|, carried in squares as there.
BOUND is a derived estimate with a measured margin: tests/test_stage2_ig_cases_cpu.py holds it against a float32 evaluation
of the same forward on the CPU at every unit, node and patient and prints the largest ratio.
"""
import collections
import contextlib
import functools
import itertools

import numpy as np
import torch

from oracle import stage2_port as sp

U = 2.0 ** -24
NODE_CAP, CASE_CAP = 3, 10

Case = collections.namedtuple("Case", "name family train_type mode P K n_steps method seed n_layers", defaults=(1,))

CASES = [
    Case("nll_early_fcnn_rpo", "nll", "early-fcnn", "radio_path_omic", 5, 4, 20, "gausslegendre", 11),
    Case("nll_late_fcnn_rpo_k32", "nll", "late-fcnn", "radio_path_omic", 33, 32, 4, "gausslegendre", 12),
    Case("nll_early_highway_rpo", "nll", "early-highway", "radio_path_omic", 2, 4, 20, "gausslegendre", 13),
    Case("nll_late_highway_rpo_k1", "nll", "late-highway", "radio_path_omic", 5, 1, 20, "gausslegendre", 14),
    Case("nll_kronecker_rpo_5x20", "nll", "kronecker", "radio_path_omic", 5, 4, 20, "gausslegendre", 15),
    Case("nll_kronecker_rp_3x20", "nll", "kronecker", "radio_path", 3, 4, 20, "gausslegendre", 16),
    Case("nll_late_fcnn_po_one_node", "nll", "late-fcnn", "path_omic", 1, 4, 1, "gausslegendre", 17),
    Case("nll_early_highway_ro_p33", "nll", "early-highway", "radio_omic", 33, 4, 20, "gausslegendre", 18),
    Case("nll_late_highway_rp_k32_n64", "nll", "late-highway", "radio_path", 2, 32, 64, "gausslegendre", 19),
    Case("cox_early_fcnn_rp_p33", "cox", "early-fcnn", "radio_path", 33, 1, 20, "gausslegendre", 20),
    Case("cox_late_fcnn_rpo_n64", "cox", "late-fcnn", "radio_path_omic", 5, 1, 64, "gausslegendre", 21),
    Case("cox_early_highway_po_p1", "cox", "early-highway", "path_omic", 1, 1, 20, "gausslegendre", 22),
    Case("cox_late_highway_ro_middle", "cox", "late-highway", "radio_omic", 2, 1, 4, "riemann_middle", 23),
    Case("cox_kronecker_ro_p1_k1", "cox", "kronecker", "radio_omic", 1, 1, 4, "gausslegendre", 24),
    Case("cox_late_fcnn_ro", "cox", "late-fcnn", "radio_omic", 2, 1, 20, "gausslegendre", 25),
    Case("cox_early_fcnn_po", "cox", "early-fcnn", "path_omic", 2, 1, 4, "gausslegendre", 26),
    # n_layers = 2, once per highway type: 5 * 22 rows are one window, 33 * 6 = 198 rows too; 13 * 22 = 286 rows are two
    # windows of 256 and 30 rows, the first of which ends inside patient 11
    Case("nll_early_highway_rpo_deep", "nll", "early-highway", "radio_path_omic", 5, 4, 20, "gausslegendre", 27, 2),
    Case("cox_late_highway_rp_deep", "cox", "late-highway", "radio_path", 33, 1, 4, "gausslegendre", 28, 2),
    Case("nll_late_highway_po_deep_two_windows", "nll", "late-highway", "path_omic", 13, 32, 20, "gausslegendre", 29, 2),
]
BY_NAME = {c.name: c for c in CASES}
ALL3 = ("radio", "path", "omic")


def names(mode):
    return sp.pick(mode, *ALL3)


def quadrature(c):
    """The rule's nodes and weights as the kernels get them: rounded once to fp32."""
    from multimodalfusion_amd import ops
    a, w = ops.ig_quadrature(c.method, c.n_steps)
    return a.astype(np.float32), w.astype(np.float32)


def make_model(c):
    """The drop-in model of the case on the CPU, the case's weights loaded, in eval mode."""
    from multimodalfusion_amd.models import coxranking_models_pretrained as cm
    from multimodalfusion_amd.models import nll_models_pretrained as nm
    cls = (nm if c.family == "nll" else cm).multimodal_pretrained
    model = cls(n_classes=c.K, mode=c.mode, train_type=c.train_type, n_layers=c.n_layers)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = sp.state_dict_for(shapes, c.seed)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return model.eval(), sd


def meta(c):
    return dict(family=c.family, kind="mm", train_type=c.train_type, mode=c.mode, B=c.P, K=c.K, n_layers=c.n_layers, train=False,
                x_seed=9000 + c.seed)


def inputs(c):
    """{radio, path, omic: [P x 256] fp32}."""
    hs, _, _, _ = sp.batch_for(meta(c))
    return dict(zip(ALL3, hs))


def sites(c):
    """The ReLU calls of oracle.stage2_port.forward in their order: (site name, modality it belongs to or None); a Highway
    calls once per layer, so its site stands n_layers times in a row."""
    tt, ns = c.train_type, names(c.mode)
    if tt == "early-fcnn":
        return [("fcnn", None)]
    if tt == "early-highway":
        return [("highway", None)] * c.n_layers
    if tt == "late-fcnn":
        return [("layer_" + {"radio": "MRI", "path": "WSI", "omic": "omic"}[n], n) for n in ALL3]
    if tt == "late-highway":
        return [("highway_" + n, n) for n in ALL3 for _ in range(c.n_layers)]
    m = len(ns)
    return [(f"{k}{i}", None) for i in range(m) for k in ("h", "o")] + [("e1", None), ("e2", None)]


@contextlib.contextmanager
def relu_hook(record, force):
    """torch.relu replaced for the block: call i's input goes to record[i]; force = {i: [(row, unit, 0 or 1)]} sets the
    mask of those entries (y = u * mask)."""
    orig, n = torch.relu, [0]

    def relu(u):
        i = n[0]
        n[0] += 1
        record.append(u.detach())
        if force and i in force:
            mask = (u > 0).to(u.dtype).detach().clone()
            for r, j, bit in force[i]:
                mask[r, j] = float(bit)
            return u * mask
        return orig(u)

    torch.relu = relu
    try:
        yield
    finally:
        torch.relu = orig


def _risk(c, sd64, xs):
    m = meta(c)
    risk, hz, S = sp.forward(sd64, m, [xs["radio"], xs["path"], xs["omic"]], None)
    return risk.reshape(-1), hz, S


def node_pass(c, sd64, x64, a, force=None):
    """One autograd pass at node a over the batch: (risk [P], {name: grad [P x 256]}, [pre-activation per ReLU call])."""
    ns = names(c.mode)
    xs = {n: (x64[n] * float(a)).requires_grad_() if n in ns else x64[n] for n in ALL3}
    rec = []
    with relu_hook(rec, force):
        risk, _, _ = _risk(c, sd64, xs)
    g = torch.autograd.grad(risk.sum(), [xs[n] for n in ns])
    return risk.detach().numpy(), {n: t.numpy() for n, t in zip(ns, g)}, [r.numpy() for r in rec]


def _bn(sd, prefix):
    """(s, t, |bias| + |mean s|: what t = bias - mean s is rounded against) of an eval-mode BatchNorm1d."""
    s = sd[prefix + ".weight"].astype(np.float64) / np.sqrt(sd[prefix + ".running_var"].astype(np.float64) + 1e-5)
    b, ms = sd[prefix + ".bias"].astype(np.float64), sd[prefix + ".running_mean"].astype(np.float64) * s
    return s, b - ms, np.abs(b) + np.abs(ms)


def carry(W, d):
    return np.sqrt((d * d) @ (W * W).T)


def bounds(c, sd, x, a, pre):
    """BOUND per ReLU call, [P x n] each (module docstring); a call of a modality the mode drops gets None."""
    f = lambda k: sd[k].astype(np.float64)
    ns, tt, a = names(c.mode), c.train_type, float(a)
    xv = {n: x[n].astype(np.float64) for n in ALL3}
    cat = np.concatenate([xv[n] for n in ns], 1)
    out = []
    if "fcnn" in tt:
        for i, (site, mod) in enumerate(sites(c)):
            if mod is not None and mod not in ns:
                out.append(None)
                continue
            pfx = "classifier" if mod is None else site
            xin = cat if mod is None else xv[mod]
            W0, b0 = f(pfx + ".0.weight"), f(pfx + ".0.bias")
            s, t, tm = _bn(sd, pfx + ".1")
            d = (W0.shape[1] + 63) // 64 + 6
            u = (pre[i] - t) / s
            out.append(U * (np.abs(s) * (a * (d + 2) * (np.abs(xin) @ np.abs(W0).T) + 2 * np.abs(b0))
                            + 4 * (np.abs(s * u) + tm)))
        return out
    if "highway" in tt:
        L, st = c.n_layers, sites(c)
        sig = lambda z: 1.0 / (1.0 + np.exp(-z))
        for i in range(0, len(st), L):
            site, mod = st[i]
            if mod is not None and mod not in ns:
                out += [None] * L
                continue
            xin = cat if mod is None else xv[mod]
            s1, t1, tm1 = _bn(sd, site + ".bn1")
            d = (xin.shape[1] + 63) // 64 + 6
            z, e = {}, {}
            for g in ("gate", "nonlinear", "linear"):
                Wg, bg = f(f"{site}.{g}.0.weight"), f(f"{site}.{g}.0.bias")
                z[g] = a * ((xin * s1) @ Wg.T) + t1 @ Wg.T + bg
                e[g] = U * (a * (d + 6) * (np.abs(xin * s1) @ np.abs(Wg).T) + (d + 3) * (np.abs(t1) @ np.abs(Wg).T + np.abs(bg))
                            + 4 * (tm1 @ np.abs(Wg).T) + 2 * np.abs(z[g]))
            out.append(e["nonlinear"])
            for l in range(1, L):
                gt, rn = sig(z["gate"]), np.maximum(z["nonlinear"], 0.0)
                x = gt * rn + (1 - gt) * z["linear"]
                ex = (e["gate"] * np.abs(rn - z["linear"]) / 4 + e["nonlinear"] * gt + e["linear"] * (1 - gt)
                      + 6 * U * (np.abs(gt * rn) + np.abs((1 - gt) * z["linear"])))
                dl = 2 * ((x.shape[1] + 255) // 256) + 11
                for g in ("gate", "nonlinear", "linear"):
                    Wg, bg = f(f"{site}.{g}.{l}.weight"), f(f"{site}.{g}.{l}.bias")
                    z[g] = x @ Wg.T + bg
                    e[g] = dl * U * (np.abs(x) @ np.abs(Wg).T + np.abs(bg)) + carry(Wg, ex)
                out.append(e["nonlinear"])
        return out
    m = len(ns)
    v = a * cat
    dv = U * np.abs(v)
    do, op = [], []
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    for i in range(m):
        Wh, bh = f(f"xfusion.reduce.{i}.0.0.weight"), f(f"xfusion.reduce.{i}.0.0.bias")
        Wz, bz = f(f"xfusion.reduce.{i}.1.0.weight"), f(f"xfusion.reduce.{i}.1.0.bias")
        Wo, bo = f(f"xfusion.reduce.{i}.2.0.weight"), f(f"xfusion.reduce.{i}.2.0.bias")
        vi, dvi = v[:, 256 * i:256 * i + 256], dv[:, 256 * i:256 * i + 256]
        bh_ = 14 * U * (np.abs(vi) @ np.abs(Wh).T + np.abs(bh)) + carry(Wh, dvi)
        dz = (14 + m) * U * (np.abs(v) @ np.abs(Wz).T + np.abs(bz)) + carry(Wz, dv)
        h = np.maximum(pre[2 * i], 0.0)
        gm = sig(v @ Wz.T + bz) * h
        dgm = (dz / 4 + 4 * U) * np.abs(h) + bh_ + U * np.abs(gm)
        bo_ = 19 * U * (np.abs(gm) @ np.abs(Wo).T + np.abs(bo)) + carry(Wo, dgm)
        out += [bh_, bo_]
        P = v.shape[0]
        do.append(np.concatenate([bo_, np.zeros((P, 1))], 1))
        op.append(np.concatenate([np.maximum(pre[2 * i + 1], 0.0), np.ones((P, 1))], 1))
    P = v.shape[0]
    kr = op[0]
    for o in op[1:]:
        kr = (kr[:, :, None] * o[:, None, :]).reshape(P, -1)
    dkr = np.zeros_like(kr)
    for t in range(m):
        term = np.ones((P, 1))
        for s_ in range(m):
            term = (term[:, :, None] * (do[s_] if s_ == t else np.abs(op[s_]))[:, None, :]).reshape(P, -1)
        dkr += term
    NQ = (17 ** (m - 1) + 63) // 64
    W, bb = f("xfusion.encoder1.0.weight"), f("xfusion.encoder1.0.bias")
    b1 = (28 + NQ) * U * (np.abs(kr) @ np.abs(W).T + np.abs(bb)) + carry(W, dkr)
    W, bb = f("xfusion.encoder2.0.weight"), f("xfusion.encoder2.0.bias")
    x2 = np.concatenate([np.maximum(pre[2 * m], 0.0), v], 1)
    K2 = W.shape[1]
    b2 = (((K2 + 63) // 64 + 3) // 4 + 12) * U * (np.abs(x2) @ np.abs(W).T + np.abs(bb)) + carry(W, np.concatenate([b1, dv], 1))
    return out + [b1, b2]


Oracle = collections.namedtuple("Oracle", "attr mod_sum mod_abs risk risk_base step_risk hazards S grads alt flagged")


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The float64 oracle of a case.  attr {name: [P x 256]}; mod_sum, mod_abs [P x m]; risk, risk_base [P]; step_risk
    [P x n]; hazards, S [P x K] or None; grads [n]{name: [P x 256]}; alt {(p, k): [(assignment bits, {name: grad row})]} for
    every (patient, node) with flagged units; flagged {(p, k): [(call, unit)]}."""
    c = BY_NAME[name]
    _, sd = make_model(c)
    sd64 = {k: torch.as_tensor(v).double() if v.dtype != np.int64 else torch.as_tensor(v) for k, v in sd.items()}
    x = inputs(c)
    x64 = {n: torch.as_tensor(v).double() for n, v in x.items()}
    ns = names(c.mode)
    al, wt = quadrature(c)
    grads, step_risk, flagged, alt = [], [], {}, {}
    for k, a in enumerate(al):
        risk, g, pre = node_pass(c, sd64, x64, a)
        bd = bounds(c, sd, x, a, pre)
        for i, b in enumerate(bd):
            if b is None:
                continue
            for p, j in zip(*np.nonzero(np.abs(pre[i]) <= b)):
                flagged.setdefault((int(p), k), []).append((i, int(j)))
        grads.append(g)
        step_risk.append(risk)
        here = {pk: fl for pk, fl in flagged.items() if pk[1] == k}
        if here:
            fmax = max(len(fl) for fl in here.values())
            assert fmax <= NODE_CAP, (name, k, fmax)
            for bits in range(2 ** fmax):
                force = {}
                for (p, _), fl in here.items():
                    for b_, (i, j) in enumerate(fl):
                        force.setdefault(i, []).append((p, j, (bits >> b_) & 1))
                _, gf, _ = node_pass(c, sd64, x64, a, force)
                for (p, _), fl in here.items():
                    if bits < 2 ** len(fl):
                        alt.setdefault((p, k), []).append((bits, {n: gf[n][p].copy() for n in ns}))
    with torch.no_grad():
        risk1, hz, S = _risk(c, sd64, x64)
        zero = {n: torch.zeros_like(v) if n in ns else v for n, v in x64.items()}
        risk0, _, _ = _risk(c, sd64, zero)
    attr = {n: x[n].astype(np.float64) * sum(float(w) * g[n] for w, g in zip(wt, grads)) for n in ns}
    mod_sum = np.stack([attr[n].sum(1) for n in ns], 1)
    mod_abs = np.stack([np.abs(attr[n]).sum(1) for n in ns], 1)
    return Oracle(attr, mod_sum, mod_abs, risk1.numpy(), risk0.numpy(), np.stack(step_risk, 1),
                  None if hz is None else hz.numpy(), None if S is None else S.numpy(), grads, alt, flagged)


def bars(o):
    """The plain bars: 1e-4 * max|oracle| per array."""
    return ({n: 1e-4 * np.abs(a).max() for n, a in o.attr.items()}, 1e-4 * np.abs(o.mod_sum).max(),
            1e-4 * np.abs(o.mod_abs).max())


def match(name, got_attr, got_sum, got_abs, patients=None):
    """Whether every patient's GPU rows -- attr {name: [P x 256]}, mod_sum, mod_abs [P x m] -- lie within the plain bars of
    ONE combination of assignments of that patient's flagged (patient, node)s, the same for all arrays.  patients: the
    oracle's patient of each given row (default: all, in order).  Returns (ok, worst ratio to the bar of the matched
    combinations)."""
    c, o = BY_NAME[name], oracle(name)
    ns = names(c.mode)
    _, wt = quadrature(c)
    bar_attr, bar_sum, bar_abs = bars(o)
    worst, ok = 0.0, True
    for r, p in enumerate(range(c.P) if patients is None else patients):
        nodes = sorted(k for (q, k) in o.alt if q == p)
        best = np.inf
        for choice in itertools.product(*[range(len(o.alt[(p, k)])) for k in nodes]):
            pick = dict(zip(nodes, choice))
            ratio = 0.0
            sums, abss = [], []
            for n in ns:
                acc = np.zeros(256)
                for k in range(c.n_steps):
                    g = o.alt[(p, k)][pick[k]][1][n] if k in pick else o.grads[k][n][p]
                    acc += float(wt[k]) * g
                a = inputs(c)[n][p].astype(np.float64) * acc
                ratio = max(ratio, np.abs(got_attr[n][r] - a).max() / bar_attr[n]) if got_attr is not None else ratio
                sums.append(a.sum())
                abss.append(np.abs(a).sum())
            ratio = max(ratio, np.abs(got_sum[r] - np.array(sums)).max() / bar_sum, np.abs(got_abs[r] - np.array(abss)).max() / bar_abs)
            best = min(best, ratio)
            if best <= 1.0:
                break
        worst = max(worst, best)
        ok = ok and best <= 1.0
    return ok, worst


def float32_gap(name):
    """The largest |pre32 - pre64| / BOUND over every ReLU unit, node and patient of the case: the float32 CPU evaluation of
    the same forward against the float64 one."""
    c = BY_NAME[name]
    _, sd = make_model(c)
    x = inputs(c)
    ns = names(c.mode)
    worst = 0.0
    for a in quadrature(c)[0]:
        pres = []
        for dt in (torch.float64, torch.float32):
            sdt = {k: torch.as_tensor(v).to(dt) if v.dtype != np.int64 else torch.as_tensor(v) for k, v in sd.items()}
            xs = {n: torch.as_tensor(v).to(dt) * (torch.tensor(a, dtype=dt) if n in ns else 1) for n, v in x.items()}
            rec = []
            with relu_hook(rec, None), torch.no_grad():
                _risk(c, sdt, xs)
            pres.append([r.double().numpy() for r in rec])
        bd = bounds(c, sd, x, a, pres[0])
        for p64, p32, b in zip(pres[0], pres[1], bd):
            if b is not None:
                worst = max(worst, float((np.abs(p32 - p64) / b).max()))
    return worst
