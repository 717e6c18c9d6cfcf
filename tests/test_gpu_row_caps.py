"""GPU: the attention stack at the row caps it admits (tests/abi_shapes.py stack_row_cap): operands that end just below
2 GiB, byte offsets with bit 30 set, tile plans of half a million to two million rows -- the fp32, bf16x3 and bf16-storage
one-bag steps, a grouped training window and a grouped forward-only window, the stand-alone scorer, and the scores of a
train-mode step whose mask indices run to 2^29.

Inputs and oracle stay small (tests/cap_cases.py): a base bag of a few hundred rows repeated on the device, the float64
oracle of the base bag with row multiplicities.  Every call goes through ctypes on guarded buffers (Guard of
tests/test_gpu_abi_shapes.py) with a workspace of exactly *_workspace_bytes; every case runs twice and must give identical
bits; A_raw is compared for every one of the N rows, on the device; no element is excused.

Bars: compare() of tests/test_gpu_path.py for fp32 (scores, hazards, S, M 1e-4, loss 1e-5, gradients 1e-5 + 1e-4 max|g|),
compare_bf16()'s against the bf16 oracle for bf16 storage (scores and M 5e-3 with the 99th percentile of the scores below
2e-4, hazards 2e-3, loss 1e-3, gradients 1 % in norm, the analytically zero ones 1e-4 abs; S, which compare_bf16 leaves
out, K * 2e-3: S_k is a product of k factors 1 - hazard_j in [0, 1]).  Each quantity's worst error over its bar is printed
(`ROWCAP ...` lines; DESIGN.md 7p holds the table)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import abi_shapes as ab
import cap_cases as cc
import launch_plans as lp
from test_gpu_abi_shapes import Guard, _lib, _p, _stream
from test_gpu_bf16 import ZERO_GRADS
from test_gpu_path import DEV

pytestmark = pytest.mark.gpu
PRE = cc.PRE


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(dtype).to(DEV)


def _names(c, dropout=False):
    att = PRE + ".3"
    if c.gated:
        return dict(W1=PRE + ".0.weight", b1=PRE + ".0.bias", Wa=att + ".attention_a.0.weight", ba=att + ".attention_a.0.bias",
                    Wb=att + ".attention_b.0.weight", bb=att + ".attention_b.0.bias", Wc=att + ".attention_c.weight",
                    bc=att + ".attention_c.bias")
    last = 3 if dropout else 2
    return dict(W1=PRE + ".0.weight", b1=PRE + ".0.bias", Wa=att + ".module.0.weight", ba=att + ".module.0.bias",
                Wc=att + f".module.{last}.weight", bc=att + f".module.{last}.bias")


class Call:
    """The device side of one case: weights, the repeated bag, the descriptor."""

    def __init__(self, c, p_drop=0.0, trace=None):
        from multimodalfusion_amd import _lib as m
        self.c, self.m, self.l = c, m, _lib()
        self.sd, base, _ = cc.base_bag(c.name)
        self.bf16 = c.chain == "bf16"
        self.names = _names(c, c.chain == "train")
        self.W = {k: _dev(self.sd[n]).contiguous() for k, n in self.names.items()}
        self.Wk, self.bk = _dev(self.sd["classifier.weight"]), _dev(self.sd["classifier.bias"])
        L, H, D = c.size
        self.idx = torch.arange(c.N, device=DEV) % c.n0
        b = _dev(cc.xq(c.name), torch.bfloat16) if self.bf16 else _dev(base)
        self.x = b.index_select(0, self.idx).contiguous()          # row i = base[i mod n0], never on the host
        assert self.x.shape == (c.N, H if c.chain == "scorer" else L) and self.x.data_ptr() % 16 == 0
        W = self.W
        self.desc = m.AmilDesc(N=c.N, L=L, H=H, D=D, gated=1 if c.gated else 0, W1=_p(W["W1"]), b1=_p(W["b1"]), Wa=_p(W["Wa"]),
                               ba=_p(W["ba"]), Wb=_p(W.get("Wb")), bb=_p(W.get("bb")), Wc=_p(W["Wc"]), bc=_p(W["bc"]),
                               p_h=p_drop, p_att=p_drop, seed=cc.MASK_SEED, seed_dev=None, trace=trace, concurrent=0,
                               gemm=c.gemm, sync=None, sync_words=0)

    def grads(self, g, dx=None):
        c = self.c
        L, H, D = c.size
        shapes = dict(dW1=(H, L), db1=(H,), dWa=(D, H), dba=(D,), dWc=(1, D), dbc=(1,))
        if c.gated:
            shapes.update(dWb=(D, H), dbb=(D,))
        if c.chain == "scorer":
            del shapes["dW1"], shapes["db1"]
        t = {k: g.alloc(s, name=k) for k, s in shapes.items()}
        st = self.m.AmilGrads(dW1=_p(t.get("dW1")), db1=_p(t.get("db1")), dWa=_p(t["dWa"]), dba=_p(t["dba"]), dWb=_p(t.get("dWb")),
                              dbb=_p(t.get("dbb")), dWc=_p(t["dWc"]), dbc=_p(t["dbc"]), dx=_p(dx))
        return t, st

    def head(self, g, G=1):
        K = cc.K
        t = dict(logits=g.alloc((G, K), name="logits"), hazards=g.alloc((G, K), name="hazards"), S=g.alloc((G, K), name="S"),
                 Y_hat=g.alloc((G,), torch.int64, name="Y_hat"), risk=g.alloc((G,), name="risk"))
        return t, self.m.SurvHead(Wk=_p(self.Wk), bk=_p(self.bk), K=K, logits=_p(t["logits"]), hazards=_p(t["hazards"]),
                                  S=_p(t["S"]), Y_hat=_p(t["Y_hat"]), risk=_p(t["risk"]))

    def target(self, g, ys, cs, scale=1.0, grads=True):
        G, H = len(ys), self.c.size[1]
        self.Y, self.cen = torch.tensor(ys, dtype=torch.int64, device=DEV), torch.tensor(cs, dtype=torch.float32, device=DEV)
        t = dict(loss=g.alloc((G,), name="loss"))
        if grads:
            t.update(dWk=g.alloc((cc.K, H), name="dWk"), dbk=g.alloc((cc.K,), name="dbk"))
        return t, self.m.NllTarget(Y=_p(self.Y), c=_p(self.cen), alpha=cc.ALPHA, eps=1e-7, loss_scale=scale, loss=_p(t["loss"]),
                                   dWk=_p(t.get("dWk")), dbk=_p(t.get("dbk")), accumulate=0)


def _finish(g, outs):
    torch.cuda.synchronize()
    for k, t in outs.items():
        g.written(t, k)
    g.check()


def _nll_step(call, ws, nbytes):
    """One mmf_amil_nll_step into fresh guarded outputs; the workspace (guarded, exactly nbytes) is the caller's."""
    c, l = call.c, call.l
    g = Guard()
    m = cc.meta(c)
    gt, gs = call.grads(g)
    ht, hs = call.head(g)
    tt, ts = call.target(g, [m["y"]], [float(m["c"])])
    A = g.alloc((c.N,), name="A_raw")
    rc = l.mmf_amil_nll_step(C.byref(call.desc), _p(call.x), 1 if call.bf16 else 0, _p(ws), nbytes, C.byref(hs), C.byref(ts),
                             _p(A), C.byref(gs), _stream())
    assert rc == ab.OK, rc
    outs = dict(gt, **ht, **tt, A_raw=A)
    _finish(g, outs)
    return outs


def _infer(call):
    """mmf_amil[_bf16]_infer on a workspace of its own exact size: M [H] and the scores again."""
    c, l = call.c, call.l
    L, H, D = c.size
    q, f = ((l.mmf_amil_bf16_infer_workspace_bytes, l.mmf_amil_bf16_infer) if call.bf16 else
            (l.mmf_amil_infer_workspace_bytes, l.mmf_amil_infer))
    nbytes = q(c.N, L, H, D, 1 if c.gated else 0)
    g = Guard()
    ws = g.alloc(nbytes, torch.uint8, name="infer workspace")
    M, A = g.alloc((1, H), name="M"), g.alloc((c.N,), name="A_raw (infer)")
    assert f(C.byref(call.desc), _p(call.x), _p(ws), nbytes, _p(M), _p(A), _stream()) == ab.OK
    _finish(g, dict(M=M, A_infer=A))
    return M, A


def _same_bits(a, b, tag):
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{tag}: {k} differs between two runs of the same call"


class Report:
    """Every quantity's worst error over its bar: printed, then asserted together."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, what, err, bar):
        err, bar = float(err), float(bar)
        self.rows.append((what, err, bar))
        print(f"ROWCAP {self.case:32s} {what:44s} err {err:.3e}  bar {bar:.3e}  err/bar {err / bar:.3f}")

    def done(self):
        bad = [(w, e, b) for w, e, b in self.rows if not e <= b]
        assert not bad, (self.case, bad)


def _scores(rep, what, A, ref_base, idx, bar):
    """All N scores against the base rows' float64 scores tiled, on the device."""
    ref = torch.as_tensor(np.asarray(ref_base, np.float64).reshape(-1)).to(DEV)
    d = (A.double().reshape(-1) - ref[idx]).abs()
    assert bool(torch.isfinite(d).all())
    rep.add(what + f" (all {A.numel()} rows)", d.max(), bar)
    return d


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _check_grads(rep, call, outs, grads, tag=""):
    names = dict(call.names, Wk="classifier.weight", bk="classifier.bias")
    for k, t in outs.items():
        if not k.startswith("d"):
            continue
        r = grads[names[k[1:]]]
        rep.add(tag + "grad " + k, np.abs(_np(t).reshape(r.shape) - r).max(), 1e-5 + 1e-4 * max(float(np.abs(r).max()), 1e-30))


def _check_f32(rep, call, outs, ref, M=None, tag=""):
    rep.add(tag + "loss", abs(float(outs["loss"][0]) - float(ref["loss"])), 1e-5)
    rep.add(tag + "hazards", np.abs(_np(outs["hazards"]) - ref["hazards"]).max(), 1e-4)
    rep.add(tag + "S", np.abs(_np(outs["S"]) - ref["S"]).max(), 1e-4)
    rep.add(tag + "risk + sum S", abs(float(outs["risk"][0]) + float(ref["S"].sum())), 1e-4 * cc.K)
    if M is not None:
        rep.add(tag + "M", np.abs(_np(M) - ref["M"]).max(), 1e-4)
    _check_grads(rep, call, outs, ref["grads"], tag)


def _workspace(call, query, *args):
    nbytes = query(*args)
    g = Guard()
    return g, g.alloc(nbytes, torch.uint8, name="workspace"), nbytes


# =======================================================================================================================
# fp32 one-bag: mmf_amil_nll_step, MMF_GEMM_F32 and MMF_GEMM_BF16X3
# =======================================================================================================================
@pytest.mark.parametrize("c", cc.F32, ids=lambda c: c.name)
def test_f32_step_at_the_row_cap(c):
    from multimodalfusion_amd._lib import KernelTrace
    L, H, D = c.size
    shipped = c.size == cc.SMALL
    tr = KernelTrace() if shipped else None
    call = Call(c, trace=tr.handle if tr else None)
    gw, ws, nbytes = _workspace(call, call.l.mmf_amil_workspace_bytes, c.N, L, H, D, 1 if c.gated else 0)
    a = _nll_step(call, ws, nbytes)
    gw.check()
    if shipped:
        # the plan: wide projection and K-dh tiles, 256 x 256 split-K TN tiles (tests/launch_plans.py, pinned to the library's
        # planner by tests/test_launch_plans_cpu.py), and the kernels of the gemm mode, none of the other's -- but for K-dh:
        # its split-operand form exists only with K-prep fused in (csrc/mmf_amil_bwd.hip plan_bwd_dh, DH_SPLIT_WIDE), and
        # 524,287 rows are 2,341 row tiles, above the 512 K-prep takes inside K-dh, so K-prep is a launch of its own and K-dh
        # the exact-fp32 wide kernel in both modes
        names = set(tr.dump())
        plan = lp.plan(c.N, "small", True)
        assert {("linear", "wide"), ("dh", "wide"), ("tn", 256)} <= {k[:2] for k in plan} and ("dh", "prep", "own launch") in plan, plan
        split = {"linear_nt_split_kernel", "gate_fwd_split_kernel", "tn_split_kernel"}
        plain = {"linear_nt_kernel", "gate_fwd_kernel", "tn_kernel"}
        assert (split if c.gemm else plain) <= names and not (plain if c.gemm else split) & names, names
        assert {"bwd_prep_kernel", "bwd_dh_kernel", "reduce_kernel"} <= names and "bwd_dh_split_kernel" not in names, names
        call.desc.trace = None
        tr.close()
    b = _nll_step(call, ws, nbytes)
    gw.check()
    _same_bits(a, b, c.name)
    M, A_inf = _infer(call)
    ref = cc.oracle(c.name)
    rep = Report(c.name)
    _scores(rep, "A_raw", a["A_raw"], ref["A_raw"], call.idx, 1e-4)
    _scores(rep, "A_raw of mmf_amil_infer", A_inf, ref["A_raw"], call.idx, 1e-4)
    _check_f32(rep, call, a, ref, M)
    rep.done()


# =======================================================================================================================
# bf16 storage: mmf_amil_nll_step with x_bf16
# =======================================================================================================================
@pytest.mark.parametrize("c", cc.BF16, ids=lambda c: c.name)
def test_bf16_step_at_the_row_cap(c):
    L, H, D = c.size
    call = Call(c)
    gw, ws, nbytes = _workspace(call, call.l.mmf_amil_bf16_workspace_bytes, c.N, L, H, D, 1 if c.gated else 0)
    a = _nll_step(call, ws, nbytes)
    b = _nll_step(call, ws, nbytes)
    gw.check()
    _same_bits(a, b, c.name)
    M, A_inf = _infer(call)
    ref = cc.oracle_bf16(c.name)
    rep = Report(c.name)
    for what, A in (("A_raw", a["A_raw"]), ("A_raw of mmf_amil_bf16_infer", A_inf)):
        d = _scores(rep, what, A, ref["A_raw"], call.idx, 5e-3)
        rep.add(what + " 99th percentile", d.kthvalue(int(0.99 * c.N)).values, 2e-4)
    rep.add("loss", abs(float(a["loss"][0]) - float(ref["loss"])), 1e-3)
    rep.add("hazards", np.abs(_np(a["hazards"]) - ref["hazards"]).max(), 2e-3)
    rep.add("S", np.abs(_np(a["S"]) - ref["S"]).max(), cc.K * 2e-3)
    rep.add("M", np.abs(_np(M) - ref["M"]).max(), 5e-3)
    names = dict(call.names, Wk="classifier.weight", bk="classifier.bias")
    for k, t in a.items():
        if not k.startswith("d"):
            continue
        r = ref["grads"][names[k[1:]]]
        if names[k[1:]].endswith(ZERO_GRADS):
            rep.add("grad " + k + " (analytically 0)", np.abs(_np(t)).max(), 1e-4)
            continue
        rep.add("grad " + k + " (norm)", np.linalg.norm(_np(t).reshape(r.shape) - r), 1e-2 * np.linalg.norm(r) + 1e-6)
    rep.done()


# =======================================================================================================================
# windows: mmf_amil_nll_step_group and mmf_amil_infer_group over sum N at the cap
# =======================================================================================================================
def _group(call):
    c = call.c
    sizes = [p * c.n0 for p in c.periods]
    G = len(sizes)
    offs = (C.c_int64 * (G + 1))(*np.concatenate([[0], np.cumsum(sizes)]).tolist())
    seeds = (C.c_uint32 * G)(*range(1, G + 1))
    return sizes, G, offs, seeds, call.m.BagGroup(G=G, offsets=offs, seeds=seeds)


def test_grouped_training_window_at_the_row_cap():
    c = cc.GROUP
    L, H, D = c.size
    call = Call(c)
    sizes, G, offs, seeds, grp = _group(call)
    l = call.l
    gw, ws, nbytes = _workspace(call, l.mmf_amil_group_workspace_bytes, offs, G, L, H, D, 1 if c.gated else 0)
    scale = 1.0 / G

    def run():
        g = Guard()
        gt, gs = call.grads(g)
        ht, hs = call.head(g, G)
        tt, ts = call.target(g, [b % cc.K for b in range(G)], [float(b % 2) for b in range(G)], scale)
        A = g.alloc((c.N,), name="A_raw")
        rc = l.mmf_amil_nll_step_group(C.byref(call.desc), C.byref(grp), _p(call.x), _p(ws), nbytes, C.byref(hs), C.byref(ts), _p(A),
                                       C.byref(gs), _stream())
        assert rc == ab.OK, rc
        outs = dict(gt, **ht, **tt, A_raw=A)
        _finish(g, outs)
        return outs
    a, b = run(), run()
    gw.check()
    _same_bits(a, b, c.name)
    refs = cc.oracle(c.name)
    rep = Report(c.name + " (train)")
    _scores(rep, "A_raw", a["A_raw"], refs[0]["A_raw"], call.idx, 1e-4)          # every bag starts on a period: row i is base[i mod n0]
    for bag, ref in enumerate(refs):
        one = {k: a[k][bag:bag + 1] for k in ("loss", "hazards", "S", "risk")}
        _check_f32(rep, call, one, ref, tag=f"bag {bag} ({sizes[bag]} rows) ")
    gsum = {k: sum(scale * r["grads"][k] for r in refs) for k in refs[0]["grads"]}
    _check_grads(rep, call, a, gsum, tag="summed ")
    rep.done()


def test_grouped_inference_window_at_the_row_cap():
    c = cc.GROUP
    L, H, D = c.size
    call = Call(c)
    sizes, G, offs, seeds, grp = _group(call)
    l = call.l
    gw, ws, nbytes = _workspace(call, l.mmf_amil_group_infer_workspace_bytes, offs, G, L, H, D, 1 if c.gated else 0, 0)

    def run():
        g = Guard()
        ht, hs = call.head(g, G)
        tt, ts = call.target(g, [b % cc.K for b in range(G)], [float(b % 2) for b in range(G)], grads=False)
        A, M = g.alloc((c.N,), name="A_raw"), g.alloc((G, H), name="M")
        rc = l.mmf_amil_infer_group(C.byref(call.desc), C.byref(grp), _p(call.x), 0, _p(ws), nbytes, C.byref(hs), C.byref(ts), _p(M),
                                    _p(A), _stream())
        assert rc == ab.OK, rc
        outs = dict(ht, **tt, A_raw=A, M=M)
        _finish(g, outs)
        return outs
    a, b = run(), run()
    gw.check()
    _same_bits(a, b, c.name)
    refs = cc.oracle(c.name)
    rep = Report(c.name + " (infer)")
    _scores(rep, "A_raw", a["A_raw"], refs[0]["A_raw"], call.idx, 1e-4)
    for bag, ref in enumerate(refs):
        one = {k: a[k][bag:bag + 1] for k in ("loss", "hazards", "S", "risk")}
        _check_f32(rep, call, one, ref, M=a["M"][bag:bag + 1], tag=f"bag {bag} ({sizes[bag]} rows) ")
    rep.done()


# =======================================================================================================================
# the scorer: mmf_attn_net_forward / _backward
# =======================================================================================================================
def test_scorer_at_the_row_cap():
    c = cc.SCORER
    _, H, D = c.size
    call = Call(c)
    l = call.l
    ref = cc.scorer_oracle(c.name)
    gA = _dev(ref["gA"]).index_select(0, call.idx).contiguous()
    gw, ws, nbytes = _workspace(call, l.mmf_attn_net_workspace_bytes, c.N, H, D, 1)

    def run():
        g = Guard()
        A, dx = g.alloc((c.N,), name="A"), g.alloc((c.N, H), name="dx")
        gt, gs = call.grads(g, dx)
        assert l.mmf_attn_net_forward(C.byref(call.desc), _p(call.x), _p(ws), nbytes, _p(A), _stream()) == ab.OK
        assert l.mmf_attn_net_backward(C.byref(call.desc), _p(call.x), _p(ws), nbytes, _p(gA), C.byref(gs), _stream()) == ab.OK
        outs = dict(gt, A=A, dx=dx)
        _finish(g, outs)
        return outs
    a = run()
    first, last = a["dx"][:cc.EDGE_ROWS].clone(), a["dx"][-cc.EDGE_ROWS:].clone()
    A1 = a["A"].clone()
    g1 = {k: v.clone() for k, v in a.items() if k.startswith("d") and k != "dx"}
    del a
    torch.cuda.empty_cache()
    b = run()
    gw.check()
    _same_bits(dict(g1, A=A1, first=first, last=last), dict({k: b[k] for k in g1}, A=b["A"], first=b["dx"][:cc.EDGE_ROWS],
                                                            last=b["dx"][-cc.EDGE_ROWS:]), c.name)
    rep = Report(c.name)
    _scores(rep, "A", b["A"], ref["A"], call.idx, 1e-4)
    dxr = ref["dx"]
    tol = 1e-5 + 1e-4 * float(np.abs(dxr).max())
    rows_last = (np.arange(c.N - cc.EDGE_ROWS, c.N) % c.n0)
    rep.add(f"dx, first {cc.EDGE_ROWS} rows", np.abs(_np(first) - dxr[np.arange(cc.EDGE_ROWS) % c.n0]).max(), tol)
    rep.add(f"dx, last {cc.EDGE_ROWS} rows", np.abs(_np(last) - dxr[rows_last]).max(), tol)
    names = call.names
    for k, t in g1.items():
        r = ref["grads"][names[k[1:]]]
        rep.add("grad " + k, np.abs(_np(t).reshape(r.shape) - r).max(), 1e-5 + 1e-4 * float(np.abs(r).max()))
    rep.done()


# =======================================================================================================================
# train mode, scores only: the mask indices of rows near 2^21 against the host restatement of the hash
# =======================================================================================================================
def test_train_mode_scores_at_the_row_cap():
    c = cc.TRAIN
    L, H, D = c.size
    call = Call(c, p_drop=cc.P_DROP)
    gw, ws, nbytes = _workspace(call, call.l.mmf_amil_workspace_bytes, c.N, L, H, D, 0)
    a = _nll_step(call, ws, nbytes)
    b = _nll_step(call, ws, nbytes)
    gw.check()
    _same_bits(a, b, c.name)
    rep = Report(c.name)
    E = cc.EDGE_ROWS
    for what, rows, got in ((f"A_raw, first {E} rows", np.arange(E), a["A_raw"][:E]),
                            (f"A_raw, last {E} rows", np.arange(c.N - E, c.N), a["A_raw"][-E:])):
        rep.add(what, np.abs(_np(got) - cc.train_scores(c.name, rows)).max(), 1e-4)
    for k, t in a.items():
        assert bool(torch.isfinite(t.float()).all()), k
    rep.done()
