"""GPU: mmf_amil_ig over every shape, row count and window plan it admits (tests/abi_shapes.py IG) against the float64 oracle
of tests/ig_cases.py (shape_oracle): integrated gradients by the definition, one autograd pass per node, on kink-free inputs --
no allowance, nothing excused.  A case above what a direct oracle affords is a base bag repeated on the device (row i =
base[i mod n0]) against the base rows' oracle with multiplicities; the comparison then runs on the device, in float64, over
every row and element, so that a 2 GiB array never reaches the host.

Every call goes through ctypes on guarded buffers (Guard of tests/test_gpu_abi_shapes.py: NaN canaries in the workspace and in
every output, each buffer between guard bands of its own) with a workspace of exactly mmf_amil_ig_workspace_bytes; every case
runs twice and must give identical bits.  Bars (tests/ig_cases.py): 1e-4 * max|oracle| per array, 1e-4 on each risk and on
the optional head outputs, 1e-4 * sum|attr| on the total and on the completeness gap.  Each quantity's worst error over its bar
is printed (`IGSHAPE ...` lines; DESIGN.md 7r holds the table) before anything is asserted.

The launch list: KernelTrace names kernels, not tiles.  The window count is asserted through it (one ig_expand_kernel and
one ig_head_kernel per window, one ig_fold_kernel per window that folds a step); which tile the attribution GEMM takes is
asserted on the restated rule (abi_shapes.attr_tile, the case's tags)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import abi_shapes as ab
import ig_cases as ic
from test_gpu_abi_shapes import Guard, _lib, _p, _stream
from test_gpu_path import DEV

pytestmark = pytest.mark.gpu
PRE = ic.PRE
CASES = ic.shape_cases()
CHUNK = 1 << 16          # rows of attr compared at a time


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(dtype).to(DEV).contiguous()


class Call:
    """The device side of one case: weights, the bag (repeated on the device where the case is periodic), the descriptor."""

    def __init__(self, c):
        from multimodalfusion_amd import _lib as m
        from multimodalfusion_amd import ops
        self.c, self.m, self.l = c, m, _lib()
        sd, base, _ = ic.shape_inputs(c.name)
        names = ([".0", ".3.attention_a.0", ".3.attention_b.0", ".3.attention_c"] if c.gated else [".0", ".3.module.0", None, ".3.module.2"])
        stack = []
        for n in names:
            stack += [None, None] if n is None else [_dev(sd[PRE + n + ".weight"]), _dev(sd[PRE + n + ".bias"])]
        self.Wk, self.bk = _dev(sd["classifier.weight"]), _dev(sd["classifier.bias"])
        self.stack, (self.Wk, self.bk), H, D = ops._stack_operands(tuple(stack), c.L, (self.Wk, self.bk), "bag", fused_head=True)
        assert (H, D) == (c.H, c.D) and self.Wk.shape[0] == c.K
        b = _dev(base)
        if c.n0:
            self.idx = torch.arange(c.N, device=DEV) % c.n0
            self.x = b.index_select(0, self.idx).contiguous()       # row i = base[i mod n0], never on the host
        else:
            self.idx, self.x = None, b
        assert self.x.shape == (c.N, c.L) and self.x.data_ptr() % 16 == 0
        self.a, self.w = ic.shape_quadrature(c)
        self.desc = ops._amil_desc(self.stack, c.N, c.L, c.H, c.D, c.gated, 0.0, 0.0, 0, None)
        self.nbytes = self.l.mmf_amil_ig_workspace_bytes(c.N, c.L, c.H, c.D, 1 if c.gated else 0, c.n_steps, c.window_steps)
        assert self.nbytes > 0
        self.gw = Guard()
        self.ws = self.gw.alloc(self.nbytes, torch.uint8, name="workspace")

    def run(self, trace=None):
        """One mmf_amil_ig into fresh guarded outputs."""
        c, m = self.c, self.m
        g = Guard()
        out = dict(row_sum=g.alloc((c.N,), name="row_sum"), row_abs=g.alloc((c.N,), name="row_abs"),
                   risk_x=g.alloc((1,), name="risk_x"), risk_base=g.alloc((1,), name="risk_base"),
                   step_risk=g.alloc((c.n_steps,), name="step_risk"))
        if c.attr:
            out["attr"] = g.alloc((c.N, c.L), name="attr")
        head = {}
        if c.K in (5, 32):
            head = dict(logits=g.alloc((c.K,), name="logits"), hazards=g.alloc((c.K,), name="hazards"), S=g.alloc((c.K,), name="S"),
                        Y_hat=g.alloc((1,), torch.int64, name="Y_hat"), risk=g.alloc((1,), name="risk"))
        sh = m.SurvHead(Wk=_p(self.Wk), bk=_p(self.bk), K=c.K, logits=_p(head.get("logits")), hazards=_p(head.get("hazards")),
                        S=_p(head.get("S")), Y_hat=_p(head.get("Y_hat")), risk=_p(head.get("risk")))
        fp = C.POINTER(C.c_float)
        ig = m.IgDesc(n_steps=c.n_steps, alpha=self.a.ctypes.data_as(fp), weight=self.w.ctypes.data_as(fp),
                      window_steps=c.window_steps, row_sum=out["row_sum"].data_ptr(), row_abs=out["row_abs"].data_ptr(),
                      attr=out["attr"].data_ptr() if c.attr else None, risk_x=out["risk_x"].data_ptr(),
                      risk_base=out["risk_base"].data_ptr(), step_risk=out["step_risk"].data_ptr())
        self.desc.trace = trace
        rc = self.l.mmf_amil_ig(C.byref(self.desc), _p(self.x), _p(self.ws), self.nbytes, C.byref(sh), C.byref(ig), _stream())
        self.desc.trace = None
        assert rc == ab.OK, rc
        out.update(head)
        torch.cuda.synchronize()
        for k, t in out.items():
            g.written(t, k)
        g.check()
        self.gw.check()
        return out


class Report:
    """Every quantity's worst error over its bar: printed, then asserted together."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, what, err, bar):
        err, bar = float(err), float(bar)
        self.rows.append((what, err, bar))
        print(f"IGSHAPE {self.case:40s} {what:30s} err {err:.3e}  bar {bar:.3e}  err/bar {err / bar:.3f}")

    def done(self):
        bad = [(w, e, b) for w, e, b in self.rows if not e <= b]
        assert not bad, (self.case, bad)


def _rows_err(got, ref_base, idx):
    """max |got - ref| over every row, in float64 on the device; ref_base is per base row."""
    ref = torch.as_tensor(np.ascontiguousarray(ref_base, np.float64)).to(DEV)
    worst = torch.zeros((), dtype=torch.float64, device=DEV)
    n = got.shape[0]
    for r0 in range(0, n, CHUNK):
        r = ref[r0:r0 + CHUNK] if idx is None else ref.index_select(0, idx[r0:r0 + CHUNK])
        d = (got[r0:r0 + CHUNK].double() - r).abs().max()
        worst = torch.where(torch.isnan(d), d, torch.maximum(worst, d))
        if bool(torch.isnan(worst)):
            break
    return float(worst)


def _expected_launches(c):
    w = ab.ig_windows(c)
    return {"ig_expand_kernel": len(w), "ig_head_kernel": len(w), "ig_fold_kernel": sum(1 for q0, _, nfold in w if nfold > 0 or q0 == 0),
            "gemm_nn_attr_kernel": 1, "ig_rows_kernel": 1}


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_case_matches_the_oracle(c):
    from multimodalfusion_amd._lib import KernelTrace
    o = ic.shape_oracle(c.name)
    call = Call(c)
    tr = KernelTrace()
    try:
        a = call.run(tr.handle)
        launches = {k: v[0] for k, v in tr.dump().items()}
    finally:
        tr.close()
    b = call.run()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{c.name}: {k} differs between two runs of the same call"
    del b
    print(f"IGSHAPE {c.name} launches {sorted(launches.items())}")
    want = _expected_launches(c)
    assert {k: launches.get(k, 0) for k in want} == want, (launches, want)
    assert not any("tn_kernel" in n or "reduce" in n or n == "gemm_nn_kernel" for n in launches), sorted(launches)

    rep = Report(c.name)
    idx = call.idx
    rep.add("row_sum (every row)", _rows_err(a["row_sum"], o.row_sum, idx), o.bar_row_sum)
    rep.add("row_abs (every row)", _rows_err(a["row_abs"], o.row_abs, idx), o.bar_row_abs)
    if c.attr:
        rep.add("attr (every element)", _rows_err(a["attr"], o.attr, idx), o.bar_attr)
    total = float(a["row_sum"].double().sum())
    risk, base = float(a["risk_x"][0]), float(a["risk_base"][0])
    rep.add("total", abs(total - o.total), o.bar_total)
    rep.add("risk_x", abs(risk - o.risk), 1e-4)
    rep.add("risk_base", abs(base - o.risk_base), 1e-4)
    rep.add("step_risk", np.abs(a["step_risk"].double().cpu().numpy() - o.step_risk).max(), 1e-4)
    rep.add("completeness gap", abs((total - (risk - base)) - o.delta), o.bar_total)
    if c.K in (5, 32):
        for k, ref in (("logits", o.logits), ("hazards", o.hazards), ("S", o.S)):
            rep.add(k, np.abs(a[k].double().cpu().numpy() - ref).max(), 1e-4)
        rep.add("risk of the head", abs(float(a["risk"][0]) - o.risk), 1e-4)
        assert float(a["risk"][0]) == risk
        top = np.sort(o.logits)[::-1]
        if top[0] - top[1] > 2e-4:
            assert int(a["Y_hat"][0]) == o.Y_hat
    assert bool((a["row_abs"] >= a["row_sum"].abs() * (1 - 1e-6)).all())
    rep.done()
