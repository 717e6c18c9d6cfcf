"""GPU: the single-workgroup and one-thread-per-element half of the C ABI over the shapes it admits (tests/abi_shapes.py,
the section below XFUSION), not only the dimensions of the three shipped models -- the survival head up to its cap
B * K = 256, nll_surv, Cox up to B = 8192 and the ranking loss across their 256-thread stride loops, the hazard head up
to K = 32 with every optional pointer NULL, the highway mix, batch norm in training and eval mode, the Adam + L1 step
through its scalar tail, abs_sum around its 512 x 256 grid, and the dense backward on both sides of the fused launch's
cap (the three-launch fallback).  Each entry point is called through ctypes on the inputs of tests/small_cases.py and
judged against that module's float64 reference at the bar it derives there (the suite's own bar within the sizes it was
set on, the summation bound beyond).  Forward and backward are separate tests: a backward kernel is given the
reference's forward output rounded to fp32, so no element is left out of any comparison.

Every output, gradient, scratch array and in-place array is a Guard view (tests/test_gpu_abi_shapes.py): after a call
every output word has been written and every band is intact; a refused call leaves everything canary and in-place
arrays bit-identical.  Each accepted case runs twice and must give identical bits.  Each comparison prints its worst
error / bar ratio (SMALL-ERR lines; DESIGN.md holds the measured table)."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_shapes as ab
import small_cases as sc
from test_gpu_abi_shapes import Guard, _id, _lib, _p, _stream
from test_gpu_path import DEV, _t

pytestmark = pytest.mark.gpu
f = C.c_float


class _Dev:
    """Device copies of the inputs of one call, alive until the call has been issued on torch's stream (a temporary would be
    freed, and its block handed to the next input, before the call is even made)."""

    def __init__(self):
        self.held = []

    def __call__(self, a, dtype=torch.float32):
        self.held.append(_t(a, dtype))
        return _p(self.held[-1])


def _acc(table, rule):
    return ab.accepted(table, rule)


def _ref(table, rule):
    return ab.refused(table, rule)


def _held(g, a, name, dtype=torch.float32, skew=0):
    """A guarded view holding the array a: an in-place argument, or an input that must come back bit-identical."""
    a = np.asarray(a)
    t = g.alloc(a.shape, dtype, skew=skew, name=name)
    t.copy_(torch.as_tensor(a).to(dtype))
    return t


def _twice(run):
    """Run an accepted case twice: {name: tensor} of guarded outputs, checked written and in bounds, identical bits."""
    outs = []
    for _ in range(2):
        g = Guard()
        rc, out = run(g)
        torch.cuda.synchronize()
        assert rc == ab.OK, rc
        g.check()
        for k, t in out.items():
            g.written(t, k)
        outs.append(out)
    for k in outs[0]:
        assert torch.equal(Guard.words(outs[0][k]), Guard.words(outs[1][k])), f"{k}: two runs differ"
    return {k: t.detach().cpu().numpy() for k, t in outs[0].items()}


def _refused(run, want):
    g = Guard()
    rc, out = run(g)
    torch.cuda.synchronize()
    assert rc == want != ab.OK, (rc, want)
    for k, t in out.items():
        g.untouched(t, k)
    g.check()


def _judge(op, c, got, ref, bar, keys):
    """Every element of every key within its bar; prints the worst error / bar ratio of each key first."""
    worst = []
    for k in keys:
        a, r = np.asarray(got[k], np.float64).reshape(-1), np.asarray(ref[k], np.float64).reshape(-1)
        b = np.broadcast_to(np.asarray(bar[k], np.float64), np.asarray(ref[k]).shape).reshape(-1)
        assert a.shape == r.shape, (k, a.shape, r.shape)
        err = np.abs(a - r)
        err[np.isnan(err)] = np.inf
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / b)
        j = int(np.argmax(ratio))
        print(f"SMALL-ERR | {op} | {c.why.split(':')[0][:60]} | {k} | err {err[j]:.3e} | bar {b[j]:.3e} | ratio {ratio[j]:.3f}")
        worst.append((k, j, float(err[j]), float(b[j]), float(ratio[j])))
    for k, j, e, b, ratio in worst:
        assert ratio <= 1.0, f"{op} {k}[{j}]: error {e:.3e} above the bar {b:.3e}"


# ---- survival head -------------------------------------------------------------------------------------------------------
def _head_fwd(c, g):
    d = _Dev()
    i = sc.head_inputs(c)
    out = dict(logits=g.alloc((c.B, c.K), name="logits"), hazards=g.alloc((c.B, c.K), name="hazards"),
               S=g.alloc((c.B, c.K), name="S"), Y_hat=g.alloc((c.B,), torch.int64, name="Y_hat"))
    rc = _lib().mmf_surv_head_forward(d(i["feat"]), d(i["Wk"]), d(i["bk"]), c.B, c.F, c.K, _p(out["logits"]),
                                      _p(out["hazards"]), _p(out["S"]), _p(out["Y_hat"]), _stream())
    return rc, out


def _head_bwd(c, g, h32=None):
    d = _Dev()
    i = sc.head_inputs(c)
    h32 = np.zeros((c.B, c.K), np.float32) if h32 is None else h32
    out = dict(dfeat=g.alloc((c.B, c.F), name="dfeat"), dWk=g.alloc((c.K, c.F), name="dWk"), dbk=g.alloc((c.K,), name="dbk"))
    rc = _lib().mmf_surv_head_backward(d(i["gH"]), d(i["gS"]), d(h32), d(i["feat"]), d(i["Wk"]),
                                       c.B, c.F, c.K, _p(out["dfeat"]), _p(out["dWk"]), _p(out["dbk"]), _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.HEAD, ab.head_rule), ids=_id)
def test_surv_head_forward(c):
    ref, bar = sc.head_ref(c)
    got = _twice(lambda g: _head_fwd(c, g))
    _judge("surv_head_forward", c, got, ref, bar, ("logits", "hazards", "S"))
    assert np.array_equal(got["Y_hat"], ref["Y_hat"])


@pytest.mark.parametrize("c", _acc(ab.HEAD, ab.head_rule), ids=_id)
def test_surv_head_backward(c):
    ref, bar = sc.head_ref(c)
    got = _twice(lambda g: _head_bwd(c, g, ref["h32"]))
    _judge("surv_head_backward", c, got, ref, bar, ("dfeat", "dWk", "dbk"))


@pytest.mark.parametrize("c", _ref(ab.HEAD, ab.head_rule), ids=_id)
def test_surv_head_refusals_write_nothing(c):
    _refused(lambda g: _head_fwd(c, g), ab.head_rule(c))
    _refused(lambda g: _head_bwd(c, g), ab.head_rule(c))


# ---- nll_surv --------------------------------------------------------------------------------------------------------------
def _nll(c, g):
    d = _Dev()
    i = sc.nll_inputs(c)
    shape = (max(c.B, 1), c.K)
    out = dict(loss=g.alloc((1,), name="loss"), gH=g.alloc(shape, name="g_hazards"), gS=g.alloc(shape, name="g_S"))
    rc = _lib().mmf_nll_surv(d(i["hazards"]), d(i["S"]), d(i["Y"], torch.int64), d(i["c"]), c.B, c.K,
                             f(sc.NLL_ALPHA), f(sc.NLL_EPS), _p(out["loss"]), _p(out["gH"]), _p(out["gS"]), _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.NLL, ab.nll_rule), ids=_id)
def test_nll_surv(c):
    ref, bar = sc.nll_ref(c)
    got = _twice(lambda g: _nll(c, g))
    if c.bad_row >= 0:                 # NaN loss, that row's gradients exactly zero, every other row judged below
        assert np.isnan(got["loss"][0]) and np.isnan(ref["loss"])
        assert not got["gH"][c.bad_row].any() and not got["gS"][c.bad_row].any()
        _judge("nll_surv", c, got, ref, bar, ("gH", "gS"))
    else:
        got["loss"] = got["loss"][0]
        _judge("nll_surv", c, got, ref, bar, ("loss", "gH", "gS"))


@pytest.mark.parametrize("c", _ref(ab.NLL, ab.nll_rule), ids=_id)
def test_nll_surv_refusals_write_nothing(c):
    _refused(lambda g: _nll(c, g), ab.nll_rule(c))


# ---- Cox ---------------------------------------------------------------------------------------------------------------------
def _cox(c, g):
    d = _Dev()
    i = sc.cox_inputs(c) if ab.cox_rule(c) == ab.OK else dict(risks=np.zeros(c.B, np.float32), times=np.zeros(c.B), c=np.zeros(c.B, np.float32))
    out = dict(loss=g.alloc((1,), name="loss"), d_risks=g.alloc((c.B,), name="d_risks"))
    rc = _lib().mmf_cox_surv(d(i["risks"]), d(i["times"], torch.float64), d(i["c"]), c.B, _p(out["loss"]),
                             _p(out["d_risks"]), _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.COX, ab.cox_rule), ids=_id)
def test_cox_surv(c):
    ref, bar = sc.cox_ref(c)
    got = _twice(lambda g: _cox(c, g))
    got["loss"] = got["loss"][0]
    _judge("cox_surv", c, got, ref, bar, ("loss", "d_risks"))
    if c.all_censored:
        assert got["loss"] == 0 and not got["d_risks"].any()


@pytest.mark.parametrize("c", _ref(ab.COX, ab.cox_rule), ids=_id)
def test_cox_surv_refusals_write_nothing(c):
    _refused(lambda g: _cox(c, g), ab.cox_rule(c))


# ---- ranking loss ----------------------------------------------------------------------------------------------------------
def _rank(c, g):
    d = _Dev()
    i = sc.rank_inputs(c)
    out = dict(loss=g.alloc((1,), name="loss"), d_risks=g.alloc((c.B,), name="d_risks"))
    rc = _lib().mmf_ranking_loss(d(i["risks"]), d(i["times"], torch.float64), d(i["c"]), c.B, c.phi, c.reduction,
                                 _p(out["loss"]), _p(out["d_risks"]), _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.RANK, ab.rank_rule), ids=_id)
def test_ranking_loss(c):
    ref, bar = sc.rank_ref(c)
    got = _twice(lambda g: _rank(c, g))
    got["loss"] = got["loss"][0]
    _judge("ranking_loss", c, got, ref, bar, ("loss", "d_risks"))
    if ref["pairs"] == 0:
        assert got["loss"] == 0 and not got["d_risks"].any()


@pytest.mark.parametrize("c", _ref(ab.RANK, ab.rank_rule), ids=_id)
def test_ranking_loss_refusals_write_nothing(c):
    _refused(lambda g: _rank(c, g), ab.rank_rule(c))


# ---- hazards ---------------------------------------------------------------------------------------------------------------
def _haz_fwd(c, g):
    d = _Dev()
    i = sc.haz_inputs(c)
    K = max(c.K, 1)
    out = dict(hazards=g.alloc((c.B, K), name="hazards"), S=g.alloc((c.B, K), name="S"))
    if c.Y_hat:
        out["Y_hat"] = g.alloc((c.B,), torch.int64, name="Y_hat")
    if c.risk:
        out["risk"] = g.alloc((c.B,), name="risk")
    rc = _lib().mmf_hazards_forward(d(i["logits"]) if c.K else d(np.zeros(4, np.float32)), c.B, c.K, _p(out["hazards"]),
                                    _p(out["S"]), _p(out.get("Y_hat")), _p(out.get("risk")), _stream())
    return rc, out


def _haz_bwd(c, g, h32=None):
    d = _Dev()
    i = sc.haz_inputs(c)
    K = max(c.K, 1)
    h32 = np.zeros((c.B, K), np.float32) if h32 is None else h32
    out = dict(dlogits=g.alloc((c.B, K), name="dlogits"))
    opt = lambda on, k: d(i[k]) if on and c.K else None
    rc = _lib().mmf_hazards_backward(opt(c.gH, "gH"), opt(c.gS, "gS"), opt(c.gR, "gR"), d(h32), c.B, c.K, _p(out["dlogits"]),
                                     _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.HAZ, ab.haz_rule), ids=_id)
def test_hazards_forward(c):
    ref, bar = sc.haz_ref(c)
    got = _twice(lambda g: _haz_fwd(c, g))
    _judge("hazards_forward", c, got, ref, bar, ("hazards", "S") + (("risk",) if c.risk else ()))
    if c.Y_hat:
        assert np.array_equal(got["Y_hat"], ref["Y_hat"])


@pytest.mark.parametrize("c", _acc(ab.HAZ, ab.haz_rule), ids=_id)
def test_hazards_backward(c):
    ref, bar = sc.haz_ref(c)
    got = _twice(lambda g: _haz_bwd(c, g, ref["h32"]))
    _judge("hazards_backward", c, got, ref, bar, ("dlogits",))
    if not (c.gH or c.gS or c.gR):
        assert not got["dlogits"].any()


@pytest.mark.parametrize("c", _ref(ab.HAZ, ab.haz_rule), ids=_id)
def test_hazards_refusals_write_nothing(c):
    _refused(lambda g: _haz_fwd(c, g), ab.haz_rule(c))
    _refused(lambda g: _haz_bwd(c, g), ab.haz_rule(c))


# ---- highway mix -------------------------------------------------------------------------------------------------------------
def _hw_fwd(c, g):
    d = _Dev()
    n = max(c.n, 1)
    i = sc.highway_inputs(ab.Highway(n))
    out = dict(y=g.alloc((n,), name="y"))
    return _lib().mmf_highway_mix_forward(d(i["zg"]), d(i["zn"]), d(i["zl"]), c.n, _p(out["y"]), _stream()), out


def _hw_bwd(c, g):
    d = _Dev()
    n = max(c.n, 1)
    i = sc.highway_inputs(ab.Highway(n))
    out = {k: g.alloc((n,), name=k) for k in ("dzg", "dzn", "dzl")}
    rc = _lib().mmf_highway_mix_backward(d(i["dy"]), d(i["zg"]), d(i["zn"]), d(i["zl"]), c.n, _p(out["dzg"]),
                                         _p(out["dzn"]), _p(out["dzl"]), _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.HIGHWAY, ab.highway_rule), ids=_id)
def test_highway_mix(c):
    ref, bar = sc.highway_ref(ab.Highway(c.n))
    _judge("highway_mix_forward", c, _twice(lambda g: _hw_fwd(c, g)), ref, bar, ("y",))
    got = _twice(lambda g: _hw_bwd(c, g))
    _judge("highway_mix_backward", c, got, ref, bar, ("dzg", "dzn", "dzl"))
    on_kink = sc.highway_inputs(ab.Highway(c.n))["zn"] == 0
    assert not got["dzn"][on_kink].any()


@pytest.mark.parametrize("c", _ref(ab.HIGHWAY, ab.highway_rule), ids=_id)
def test_highway_mix_refusals_write_nothing(c):
    _refused(lambda g: _hw_fwd(c, g), ab.highway_rule(c))
    _refused(lambda g: _hw_bwd(c, g), ab.highway_rule(c))


# ---- batch norm --------------------------------------------------------------------------------------------------------------
def _bn_fwd(c, g):
    d = _Dev()
    i = sc.bn_inputs(c)
    out = dict(y=g.alloc((c.B, c.F), name="y"), save_mean=g.alloc((c.F,), name="save_mean"), save_invstd=g.alloc((c.F,), name="save_invstd"))
    stats = dict(running_mean=_held(g, i["rm"], "running_mean"), running_var=_held(g, i["rv"], "running_var")) if c.running else {}
    opt = lambda on, k: d(i[k]) if on else None
    rc = _lib().mmf_batchnorm_forward(d(i["x"]), opt(c.res, "res"), opt(c.affine, "gamma"), opt(c.affine, "beta"),
                                      _p(stats.get("running_mean")), _p(stats.get("running_var")), c.B, c.F, int(c.training),
                                      f(sc.BN_EPS), f(sc.BN_MOM), c.act, f(c.drop_p), sc.SEED, sc.SITE, None, _p(out["y"]),
                                      _p(out["save_mean"]), _p(out["save_invstd"]), _stream())
    return rc, out, stats


@pytest.mark.parametrize("c", _acc(ab.BN, ab.bn_rule), ids=_id)
def test_batchnorm_forward(c):
    ref, bar = sc.bn_ref(c)

    def run(g):
        rc, out, stats = _bn_fwd(c, g)
        return rc, {**out, **stats}
    got = _twice(run)
    _judge("batchnorm_forward", c, got, ref, bar, ("y", "save_mean", "save_invstd") + (("running_mean", "running_var") if c.running else ()))
    if not c.training:                 # eval mode reads the running statistics and leaves them alone
        i = sc.bn_inputs(c)
        assert np.array_equal(got["running_mean"], i["rm"]) and np.array_equal(got["running_var"], i["rv"])


@pytest.mark.parametrize("c", _acc(ab.BN, ab.bn_rule), ids=_id)
def test_batchnorm_backward(c):
    ref, bar = sc.bn_ref(c)
    i = sc.bn_inputs(c)

    def run(g):
        d = _Dev()
        out = dict(dx=g.alloc((c.B, c.F), name="dx"))
        if c.dres:
            out["dres"] = g.alloc((c.B, c.F), name="dres")
        if c.dgb:
            out.update(dgamma=g.alloc((c.F,), name="dgamma"), dbeta=g.alloc((c.F,), name="dbeta"))
        rc = _lib().mmf_batchnorm_backward(d(i["dy"]), d(ref["y32"]), d(i["x"]), d(i["gamma"]) if c.affine else None,
                                           d(sc.r32(ref["save_mean"])), d(sc.r32(ref["save_invstd"])), c.B, c.F,
                                           int(c.training), c.act, f(c.drop_p), sc.SEED, sc.SITE, None, _p(out["dx"]),
                                           _p(out.get("dres")), _p(out.get("dgamma")), _p(out.get("dbeta")), _stream())
        return rc, out
    got = _twice(run)
    _judge("batchnorm_backward", c, got, ref, bar, tuple(got))


@pytest.mark.parametrize("c", _ref(ab.BN, ab.bn_rule), ids=_id)
def test_batchnorm_refusals_write_nothing(c):
    c = ab.Bn(c.B, c.F, c.training, running=True, why=c.why)          # with running statistics: they must stay as they are
    g = Guard()
    rc, out, stats = _bn_fwd(c, g)
    torch.cuda.synchronize()
    assert rc == ab.bn_rule(c) == ab.ERR_SHAPE
    for k, t in out.items():
        g.untouched(t, k)
    i = sc.bn_inputs(c)
    assert np.array_equal(stats["running_mean"].cpu().numpy(), i["rm"]) and np.array_equal(stats["running_var"].cpu().numpy(), i["rv"])
    g.check()


# ---- Adam + L1 ---------------------------------------------------------------------------------------------------------------
def _adam(c, g, state, step, skew=0):
    """One call from `state` (numpy w, g, m, v, mask) -> (rc, guarded w, m, v, g)."""
    d = _Dev()
    w = _held(g, state["w"], "w", skew=skew)
    t = dict(w=w, m=_held(g, state["m"], "m"), v=_held(g, state["v"], "v"), g=_held(g, state["g"], "g"))
    hp = sc.ADAM_HP
    rc = _lib().mmf_adam_l1_step(_p(t["w"]), _p(t["g"]), _p(t["m"]), _p(t["v"]), c.n, f(hp["lr"]), f(hp["b1"]), f(hp["b2"]), f(hp["eps"]),
                                 f(c.wd), f(c.l1), d(state["mask"]) if c.mask else None, step, _stream())
    return rc, t


def _adam_checked(c, state, step):
    """One step from `state`, twice, against torch's Adam in float64 from the same fp32 state; -> the kernel's new state."""
    got = _twice(lambda g: _adam(c, g, state, step))
    assert np.array_equal(got["g"].view(np.int32), np.asarray(state["g"]).view(np.int32)), "the step changed g"
    ref, bar = sc.adam_step_ref(c, state["w"], state["g"], state["m"], state["v"], state["mask"], step)
    _judge(f"adam_l1_step (step {step})", c, got, ref, bar, ("w", "m", "v"))
    z = state["zeros"]                 # pad-like elements: w = +-0, g = m = v = 0 stay exactly zero whatever l1 is
    for k in ("w", "m", "v"):
        assert not got[k][z].any(), f"{k}: a zero element moved"
    return got


@pytest.mark.parametrize("c", _acc(ab.ADAM, ab.adam_rule), ids=_id)
def test_adam_l1_step(c):
    _adam_checked(c, sc.adam_inputs(c), c.step)


def test_adam_l1_three_steps_carry_m_and_v():
    """Steps 1, 2, 3 from m = v = 0 with m, v and w carried over on the device's own fp32 values, a new gradient each step:
    every step judged from the state it started from; the pad-like elements stay exactly zero throughout."""
    c = [c for c in ab.ADAM if c.n == 1027][0]
    state = dict(sc.adam_inputs(c))
    state["m"], state["v"] = np.zeros(c.n, np.float32), np.zeros(c.n, np.float32)
    for step in (1, 2, 3):
        state["g"] = sc.adam_inputs(c, step)["g"]
        got = _adam_checked(c, state, step)
        state.update(w=got["w"], m=got["m"], v=got["v"])


@pytest.mark.parametrize("c", _ref(ab.ADAM, ab.adam_rule), ids=_id)
def test_adam_l1_refusals_write_nothing(c):
    state = sc.adam_inputs(c)
    g = Guard()
    rc, t = _adam(c, g, state, c.step, skew=1 if c.misalign else 0)
    torch.cuda.synchronize()
    assert rc == ab.adam_rule(c) != ab.OK
    for k in ("w", "m", "v", "g"):
        assert np.array_equal(t[k].cpu().numpy().view(np.int32), np.asarray(state[k]).view(np.int32)), k
    g.check()


# ---- abs_sum -----------------------------------------------------------------------------------------------------------------
def _abs_sum(c, g):
    w = _t(sc.abs_sum_inputs(ab.AbsSum(max(c.n, 1))))
    out = dict(partials=g.alloc((512,), name="partials"), out=g.alloc((1,), name="out"))
    return _lib().mmf_abs_sum(_p(w), c.n, _p(out["partials"]), _p(out["out"]), _stream()), out


@pytest.mark.parametrize("c", _acc(ab.ABS_SUM, ab.abs_sum_rule), ids=_id)
def test_abs_sum(c):
    ref, bar = sc.abs_sum_ref(c)
    got = _twice(lambda g: _abs_sum(c, g))
    _judge("abs_sum", c, dict(out=got["out"][0]), dict(out=ref), dict(out=bar), ("out",))


@pytest.mark.parametrize("c", _ref(ab.ABS_SUM, ab.abs_sum_rule), ids=_id)
def test_abs_sum_refusals_write_nothing(c):
    _refused(lambda g: _abs_sum(c, g), ab.abs_sum_rule(c))


# ---- dense backward ------------------------------------------------------------------------------------------------------------
def _dense_bwd(c, g, y32=None):
    d = _Dev()
    from multimodalfusion_amd import ops
    ok = ab.dense_bwd_rule(c) == ab.OK
    i = sc.dense_inputs(c if ok else ab.DenseBwd(c.B, c.K, c.N))
    y32 = np.zeros((c.B, c.N), np.float32) if y32 is None else y32
    out = dict(dpre=g.alloc((c.B, c.N), name="dpre scratch"), dW=g.alloc((c.N, c.K), name="dW"))
    if c.dx:
        out["dx"] = g.alloc((c.B, c.K), name="dx")
    if c.db:
        out["db"] = g.alloc((c.N,), name="db")
    tx, tW = _t(i["x"]), _t(i["W"])
    if c.rows:                         # y and dy as columns of wider matrices, NaN around them
        ld = c.N + abs(c.rows)
        wide = torch.full((2, c.B, ld), float("nan"), device=DEV)
        off = abs(c.rows) // 2
        wide[0, :, off:off + c.N], wide[1, :, off:off + c.N] = _t(i["dy"]), _t(y32)
        base = ops.dropout_row_base(sc.dense_row_seeds(c), DEV)
        ldy = ld if c.rows > 0 else c.N - 1
        rc = _lib().mmf_dense_backward_rows(_p(wide[0, :, off:]), ldy, _p(wide[1, :, off:]), ldy, _p(tx), _p(tW), c.B, c.K, c.N, c.act,
                                            c.drop_kind, f(i["p"]), sc.SITE, None, _p(base), _p(out["dpre"]), _p(out.get("dx")),
                                            _p(out["dW"]), _p(out.get("db")), _stream())
    else:
        rc = _lib().mmf_dense_backward(d(i["dy"]), d(y32), _p(tx), _p(tW), c.B, c.K, c.N, c.act, c.drop_kind, f(i["p"]),
                                       sc.SEED, sc.SITE, None, _p(out["dpre"]), _p(out.get("dx")), _p(out["dW"]), _p(out.get("db")),
                                       _stream())
    return rc, out


@pytest.mark.parametrize("c", _acc(ab.DENSE_BWD, ab.dense_bwd_rule), ids=_id)
def test_dense_backward(c):
    ref, bar = sc.dense_ref(c)
    def run(g):
        rc, out = _dense_bwd(c, g, ref["y32"])
        if ab.dense_bwd_path(c).startswith("fused"):       # the one-launch form rebuilds dpre in LDS: the header says the
            torch.cuda.synchronize()                        # scratch stays untouched
            g.untouched(out.pop("dpre"), "dpre scratch")
        return rc, out
    got = _twice(run)
    _judge("dense_backward", c, got, ref, bar, tuple(got))


@pytest.mark.parametrize("c", _ref(ab.DENSE_BWD, ab.dense_bwd_rule), ids=_id)
def test_dense_backward_refusals_write_nothing(c):
    _refused(lambda g: _dense_bwd(c, g), ab.dense_bwd_rule(c))
