"""GPU: every one-call training step on poisoned memory, against the fp64 oracle (the bf16 oracle for a bf16 bag).

The steps take their outputs, workspaces and write-mode gradients from torch.empty / torch.empty_like.  In the rest of the
suite such a block is fresh device memory (zeros) or the block the previous call of the same shape just freed (nearly the
right answer), so a kernel that skips writing a ragged last row, one split-K slice or a bag-boundary row can still pass:
the true value there is often 0, or the stale one matches.  Here every CUDA tensor the step allocates through those calls is
filled first, in two modes:

  nan   float NaN, uint8 workspaces 0xFF, integers -1;
  huge  float 1e30, uint8 workspaces 0x7E (~8.4e37 per fp32 / bf16 element), integers -1 -- fmaxf and max-reductions
        swallow a NaN but not a huge finite value.

torch.zeros is never patched, and the tick words (ops.sync_words) must read zero before and after every call.  Every case
runs on two inputs of the same shape: the second call gets the first call's blocks, poisoned over, so a read that runs
ahead of its store sees poison rather than a plausible stale value (a timing-dependent second line of defence; the
deterministic guard for device-scope handoffs is tools/isa_check.py, rule 4).  Last, the gradient-buffer contract of each
step under poison: grad_out full of NaN is overwritten, a random grad_out is added to within one fp32 rounding, and with
some .grad set and some None the set ones are added to and the missing ones receive exactly the step's gradients."""
import numpy as np
import pytest
import torch

from oracle import bf16_port, cases
from test_gpu_bf16 import compare_bf16
from test_gpu_group_step import _bag_meta, check_group, group_oracle
from test_gpu_maxnet_step import _check as check_omic
from test_gpu_path import DEV, _grads, _load, _t, compare, relu_kink_units

pytestmark = pytest.mark.gpu

MODES = ("nan", "huge")
FILL = {"nan": (float("nan"), 0xFF, -1), "huge": (1e30, 0x7E, -1)}      # (floating point, uint8, other integers)


class Poison:
    """What the `poison` fixture hands a test: run(mode, fn, ...) calls fn with every CUDA allocation made through
    torch.empty / torch.empty_like filled per `mode`, and checks the tick words around the call."""

    def __init__(self):
        self.mode = None
        self.filled = 0

    def fill(self, t):
        if self.mode is not None and torch.is_tensor(t) and t.is_cuda and t.numel() and t.dtype != torch.bool:
            f, u8, i = FILL[self.mode]
            t.fill_(u8 if t.dtype == torch.uint8 else f if t.is_floating_point() else i)
            self.filled += 1
        return t

    @staticmethod
    def words_zero(tag):
        from multimodalfusion_amd import ops
        ops.sync_words(DEV)
        for key, w in list(ops._sync.items()):          # this stream's words and any side stream's
            assert int(w.abs().sum()) == 0, f"{tag}: tick words of {key} not zero"

    def run(self, mode, fn, *a, **kw):
        torch.cuda.synchronize()
        self.words_zero(f"before ({mode})")
        n0, self.mode = self.filled, mode
        try:
            out = fn(*a, **kw)
            torch.cuda.synchronize()
        finally:
            self.mode = None
        self.words_zero(f"after ({mode})")
        assert self.filled > n0, "the step allocated nothing through the poisoned calls"
        return out


@pytest.fixture
def poison(monkeypatch):
    """torch.empty and torch.empty_like (the only forms ops.py, models/ and utils/ allocate device memory with) wrapped so
    that CUDA tensors are filled while a Poison.run call is active; CPU tensors (the oracle's) are left alone."""
    p = Poison()
    empty, empty_like = torch.empty, torch.empty_like
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: p.fill(empty(*a, **kw)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **kw: p.fill(empty_like(*a, **kw)))
    return p


def _pin_seed(monkeypatch, seed):
    from multimodalfusion_amd import ops
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: seed)


def _no_grads(model):
    for p in model.parameters():
        p.grad = None


def _one_rounding(got, want, tag):
    """got (fp32) == want (fp64: base + gradient) to within one fp32 rounding per element."""
    got = np.asarray(got, np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bad = np.abs(got - want) > ulp
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements beyond one fp32 rounding of base + grad " \
                          f"(max {float(np.abs(got - want).max()):.3e})"


def check_grad_contract(poison, model, step, check_write, tag):
    """The gradient-buffer conventions of one step under poison.  step(**kw) runs it (kw: grad_out / accumulate);
    check_write(grads: {name: ndarray}) judges the write-mode gradients against the oracle."""
    names = [k for k, _ in model.named_parameters()]
    params = list(model.parameters())
    gen = torch.Generator().manual_seed(1234)
    for mode in MODES:
        _no_grads(model)
        # grad_out full of NaN, accumulate=False: every element overwritten
        out = [torch.full_like(p, float("nan")) for p in params]
        poison.run(mode, step, grad_out=out, accumulate=False)
        assert all(p.grad is None for p in params), tag
        g = {k: o.cpu().numpy().copy() for k, o in zip(names, out)}
        for k, v in g.items():
            assert np.isfinite(v).all(), f"{tag} ({mode}): {k} not fully written"
        check_write(g)
        # a random base, accumulate=True: base + grads
        base = {k: torch.randn(p.shape, generator=gen) for k, p in zip(names, params)}
        out = [base[k].to(DEV) for k in names]
        poison.run(mode, step, grad_out=out, accumulate=True)
        for k, o in zip(names, out):
            _one_rounding(o.cpu().numpy(), base[k].double().numpy() + g[k], f"{tag} ({mode}) grad_out {k}")
        # .grad: every other parameter set (added to), the rest None (receive exactly the step's gradients)
        for i, p in enumerate(params):
            p.grad = base[names[i]].to(DEV) if i % 2 == 0 else None
        poison.run(mode, step)
        for i, (k, p) in enumerate(zip(names, params)):
            if i % 2 == 0:
                _one_rounding(p.grad.cpu().numpy(), base[k].double().numpy() + g[k], f"{tag} ({mode}) .grad {k}")
            elif p.grad is None:
                assert not g[k].any(), f"{tag} ({mode}): {k} has a gradient but its .grad stayed None"
            else:
                assert np.array_equal(p.grad.cpu().numpy(), g[k]), f"{tag} ({mode}): fresh .grad {k} is not the step's gradient"
    _no_grads(model)


# ---------------- pathology head: nll_step ----------------------------------------------------------------------------

PATH_N = [1, 17, 65, 999, 4097, 16421, 20011]


def _path_meta(N, gated, rep, train=False, dropout=False):
    return dict(N=N, gated=gated, size="small", K=4, dropout=dropout, y=(N + rep) % 4, c=(N + rep) % 2, alpha=0.2,
                bias_std=0.05, train=train, seed=9000 + int(gated), x_seed=9100 + N + 31 * rep, mask_seed=9200 + rep)


def _path_model(m, sd):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    model = _load(MIL_Attention_fc_surv_path(gate_path=m["gated"], model_size_wsi=m["size"], dropout=m["dropout"],
                                             n_classes=m["K"]), sd)
    return model.train() if m["train"] else model.eval()


def _path_step(model, xt, m, **kw):
    hz, S, Yh, A_raw, loss, risk = model.nll_step(xt, torch.tensor([m["y"]]), torch.tensor([float(m["c"])]),
                                                  alpha=m["alpha"], loss_scale=1.0, **kw)
    torch.cuda.synchronize()
    assert abs(float(risk) + float(S.sum())) < 1e-6
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(), A_raw=A_raw.cpu().numpy(),
                loss=float(loss), M=None)


@pytest.mark.parametrize("gated", [True, False])
def test_path_step_write_mode_on_poison(gated, poison):
    """Every .grad None (write mode): the flat gradient buffer, the workspace and every output are poisoned; the sizes
    cover a single row, ragged 16 / 64-row tiles, the K-split and wide tile plans; then the same with bf16x3 GEMMs."""
    from multimodalfusion_amd import ops
    for N in PATH_N:
        for rep in range(2):
            m = _path_meta(N, gated, rep)
            sd, x, _ = cases.path_inputs(m)
            ref, kinks = cases.run_path(m), relu_kink_units(sd, x)
            model, xt = _path_model(m, sd), _t(x)
            for gemm in (0, 1):
                prev = ops.set_gemm(gemm)
                try:
                    for mode in MODES:
                        _no_grads(model)
                        res = poison.run(mode, _path_step, model, xt, m)
                        res["grads"] = _grads(model)
                        compare(res, ref, f"N={N} gated={gated} rep={rep} gemm={gemm} {mode}", kink_units=kinks)
                finally:
                    ops.set_gemm(prev)
            del model, xt


def test_path_step_train_both_dropout_sites_on_poison(poison, monkeypatch):
    for rep in range(2):
        m = _path_meta(4097, True, rep, train=True, dropout=True)
        sd, x, _ = cases.path_inputs(m)
        ref, kinks = cases.run_path(m), relu_kink_units(sd, x)
        model, xt = _path_model(m, sd), _t(x)
        _pin_seed(monkeypatch, m["mask_seed"])
        for mode in MODES:
            _no_grads(model)
            res = poison.run(mode, _path_step, model, xt, m)
            res["grads"] = _grads(model)
            compare(res, ref, f"train dropout rep={rep} {mode}", kink_units=kinks)


def test_path_step_bf16_bag_on_poison(poison, monkeypatch):
    for rep in range(2):
        m = dict(_path_meta(4097, True, rep, train=True, dropout=True), bias_std=0.02)
        sd, x, masks = cases.path_inputs(m)
        xq = bf16_port.rb(bf16_port._t(x)).numpy()
        ref = bf16_port.path_step_bf16(sd, xq, m["y"], m["c"], m["alpha"], gated=True, dropout=True, masks=masks)
        model, xt = _path_model(m, sd), _t(xq).to(torch.bfloat16)
        _pin_seed(monkeypatch, m["mask_seed"])
        for mode in MODES:
            _no_grads(model)
            res = poison.run(mode, _path_step, model, xt, m)
            res["grads"] = _grads(model)
            compare_bf16(res, ref, f"bf16 rep={rep} {mode}", a_tol=5e-3, h_tol=2e-3, l_tol=1e-3, g_rel=1e-2)


def test_path_step_grad_contract_on_poison(poison):
    m = _path_meta(4097, True, 0)
    sd, x, _ = cases.path_inputs(m)
    ref, kinks = cases.run_path(m), relu_kink_units(sd, x)
    model, xt = _path_model(m, sd), _t(x)

    def check_write(g):
        compare(dict(hazards=ref["hazards"], S=ref["S"], A_raw=ref["A_raw"], loss=float(ref["loss"]), grads=g), ref,
                "path grad_out", kink_units=kinks)
    check_grad_contract(poison, model, lambda **kw: _path_step(model, xt, m, **kw), check_write, "path nll_step")


# ---------------- pathology head: nll_step_group ----------------------------------------------------------------------

CYCLE = [1, 15, 16, 17, 63, 64, 65, 255, 257]
GROUPS = {
    "64 cycled sizes": ([CYCLE[g % len(CYCLE)] for g in range(64)], True, False),
    "64 one-row bags": ([1] * 64, False, False),
    "four bags, train": ([1, 999, 4097, 10000], True, True),
}


def _group_metas(sizes, gated, train, rep):
    base = dict(gated=gated, size="small", K=4, dropout=train, alpha=0.3, bias_std=0.05, train=train, seed=4343,
                x_seed=700 + 10007 * rep, mask_seed=1700 + 10007 * rep)
    return [_bag_meta(base, g, n) for g, n in enumerate(sizes)]


def _group_step(model, bags, metas, **kw):
    hz, S, Yh, A, loss, risk = model.nll_step_group(bags, torch.tensor([mm["y"] for mm in metas]),
                                                    torch.tensor([float(mm["c"]) for mm in metas]), alpha=metas[0]["alpha"],
                                                    loss_scale=1.0 / len(metas),
                                                    seeds=[mm["mask_seed"] for mm in metas] if metas[0]["train"] else None,
                                                    **kw)
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(), A=[a.cpu().numpy() for a in A],
                loss=loss.cpu().numpy(), risk=risk.cpu().numpy())


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_step_on_poison(name, poison):
    """The grouped step's SEG kernels, bag-aligned pooling partials and per-bag merge on poisoned memory, up to the full
    64-bag window: per bag against that bag's oracle, the summed gradients against the oracle's sum."""
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_path
    sizes, gated, train = GROUPS[name]
    for rep in range(2):
        metas = _group_metas(sizes, gated, train, rep)
        refs, kinks = group_oracle(metas)
        sd, _, _ = cases.path_inputs(dict(metas[0], N=1))
        model = _path_model(metas[0], sd)
        assert isinstance(model, MIL_Attention_fc_surv_path)
        bags = [_t(cases.path_inputs(mm)[1]) for mm in metas]
        for mode in MODES:
            _no_grads(model)
            res = poison.run(mode, _group_step, model, bags, metas)
            res["grads"] = _grads(model)
            check_group(res, 1.0 / len(metas), refs, kinks, tag=f"{name} rep={rep} {mode}: ")


def test_group_step_grad_contract_on_poison(poison):
    metas = _group_metas(GROUPS["four bags, train"][0], True, True, 0)
    refs, kinks = group_oracle(metas)
    sd, _, _ = cases.path_inputs(dict(metas[0], N=1))
    model = _path_model(metas[0], sd)
    bags = [_t(cases.path_inputs(mm)[1]) for mm in metas]
    scale = 1.0 / len(metas)
    gsum = {k: sum(scale * r["grads"][k] for r in refs) for k in refs[0]["grads"]}

    def check_write(g):
        compare(dict(hazards=0, S=0, A_raw=0, loss=0.0, grads=g), dict(hazards=0, S=0, A_raw=0, loss=0.0, grads=gsum),
                "group grad_out", kink_units=kinks)
    check_grad_contract(poison, model, lambda **kw: _group_step(model, bags, metas, **kw), check_write, "nll_step_group")


# ---------------- radiology head ----------------------------------------------------------------------------------------

def _radio_cases(golden):
    g = golden("radio")
    return [(name, dict(m, x_seed=m["x_seed"] + 977 * rep), rep) for name, m in g.meta.items() for rep in range(2)]


def _radio_model(m, sd):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    model = _load(MIL_Attention_fc_surv_radio(radio_fusion="concat", gate_radio=m["gated"], dropout=m["dropout"],
                                              n_classes=m["K"], modalities=cases.MODS[:m["n_mod"]]), sd)
    return model.train() if m["train"] else model.eval()


def _radio_step(model, kw, m, **extra):
    hz, S, Yh, A_raw, loss, risk = model.nll_step(torch.tensor([m["y"]], device=DEV), torch.tensor([float(m["c"])], device=DEV),
                                                  alpha=m["alpha"], **extra, **kw)
    torch.cuda.synchronize()
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(), A_raw=A_raw.cpu().numpy(),
                loss=float(loss), M=None)


def test_radio_step_on_poison(golden, poison, monkeypatch):
    """The radiology step at the shapes of its fixtures: reduce_dim's output and d loss / d that output (dx) come from
    torch.empty as well."""
    for name, m, rep in _radio_cases(golden):
        sd, xs, _ = cases.radio_inputs(m)
        ref = cases.run_radio(m)
        model = _radio_model(m, sd)
        kw = {k: _t(x) for k, x in zip(cases.MODS, xs)}
        if m["train"]:
            _pin_seed(monkeypatch, m["mask_seed"])
        for mode in MODES:
            _no_grads(model)
            res = poison.run(mode, _radio_step, model, kw, m)
            res["grads"] = _grads(model)
            compare(res, ref, f"radio {name} rep={rep} {mode}")


def test_radio_step_grad_contract_on_poison(golden, poison):
    m = golden("radio").meta["m4_n512"]
    sd, xs, _ = cases.radio_inputs(m)
    ref = cases.run_radio(m)
    model = _radio_model(m, sd)
    kw = {k: _t(x) for k, x in zip(cases.MODS, xs)}

    def check_write(g):
        compare(dict(hazards=ref["hazards"], S=ref["S"], A_raw=ref["A_raw"], loss=float(ref["loss"]), grads=g), ref,
                "radio grad_out")
    check_grad_contract(poison, model, lambda **ex: _radio_step(model, kw, m, **ex), check_write, "radio nll_step")


# ---------------- multimodal head (concat and tensor fusion) ------------------------------------------------------------

def _mm_setup(m):
    from test_gpu_mm_step import _inputs, _model
    sd, kw = _inputs(m)
    return _model(m, sd).eval(), kw


def _mm_step(model, kw, m, **extra):
    hz, S, Yh, A_raw, loss, risk = model.nll_step(torch.tensor([m["y"]], device=DEV), torch.tensor([float(m["c"])], device=DEV),
                                                  alpha=m["alpha"], **extra, **kw)
    torch.cuda.synchronize()
    assert abs(float(risk) + float(S.sum())) <= 1e-6
    return dict(hazards=hz.cpu().numpy(), S=S.cpu().numpy(), Y_hat=Yh.cpu().numpy(),
                A_raw={k: v.cpu().numpy() for k, v in A_raw.items()}, loss=float(loss), M=None)


def test_mm_step_on_poison(golden, poison):
    """The multimodal step at the shapes of its fixtures, concat and tensor fusion: the concatenated feature vector, the
    head's gradient buffers and every branch's workspaces are poisoned."""
    fusions = set()
    for name, m0 in golden("mm").meta.items():
        fusions.add(m0["fusion"])
        for rep in range(2):
            m = dict(m0, x_seed=m0["x_seed"] + 977 * rep)
            ref = cases.run_mm(m)
            model, kw = _mm_setup(m)
            for mode in MODES:
                _no_grads(model)
                res = poison.run(mode, _mm_step, model, kw, m)
                res["grads"] = _grads(model)
                compare(res, ref, f"mm {name} rep={rep} {mode}")
    assert fusions == {"concat", "tensor"}


@pytest.mark.parametrize("fusion", ["concat", "tensor"])
def test_mm_step_grad_contract_on_poison(fusion, golden, poison):
    name, m = next((k, v) for k, v in golden("mm").meta.items() if v["fusion"] == fusion and v["mode"] == "radio_path_omic")
    ref = cases.run_mm(m)
    model, kw = _mm_setup(m)

    def check_write(g):
        compare(dict(hazards=ref["hazards"], S=ref["S"], A_raw=ref["A_raw"], loss=float(ref["loss"]), grads=g), ref,
                f"mm {name} grad_out")
    check_grad_contract(poison, model, lambda **ex: _mm_step(model, kw, m, **ex), check_write, f"mm {name} nll_step")


# ---------------- omic head: cox_step -----------------------------------------------------------------------------------

COX_B = [2, 7, 128, 129, 256]


def _omic_setup(B, train, rep):
    from test_gpu_maxnet_step import _model
    m = dict(B=B, G=36 if B % 2 == 0 else 80, nll=False, K=4, train=train, seed=800 + B, x_seed=900 + B + 53 * rep,
             mask_seed=41 + rep, bias_std=0.05, alpha=0.0, y=0)
    sd, x, t, c, _ = cases.omic_inputs(m)
    model = _model(m, sd)
    assert model.cox_step_ok(_t(x))
    return m, model, (_t(x), torch.as_tensor(t).to(DEV), _t(c))


def _cox_step(model, inputs, **kw):
    risk, loss = model.cox_step(*inputs, **kw)
    torch.cuda.synchronize()
    return risk.cpu().numpy(), float(loss)


@pytest.mark.parametrize("train", [True, False])
def test_cox_step_on_poison(train, poison, monkeypatch):
    """The one-launch omic step with 32 and 64 workgroups, ragged last workgroups: risks, loss, workspace and write-mode
    gradients poisoned.  The risks cross grid barrier 1: a workgroup that read one before it landed would see poison."""
    for B in COX_B:
        for rep in range(2):
            m, model, inputs = _omic_setup(B, train, rep)
            ref = cases.run_omic(m)
            _pin_seed(monkeypatch, m["mask_seed"])
            for mode in MODES:
                _no_grads(model)
                risk, loss = poison.run(mode, _cox_step, model, inputs)
                grads = {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}
                check_omic((risk, loss, grads), ref, f"B={B} train={train} rep={rep} {mode}")


def test_cox_step_grad_contract_on_poison(poison, monkeypatch):
    m, model, inputs = _omic_setup(129, True, 0)
    ref = cases.run_omic(m)
    _pin_seed(monkeypatch, m["mask_seed"])
    risk_loss = {}

    def step(**kw):
        risk_loss["v"] = _cox_step(model, inputs, **kw)

    def check_write(g):
        check_omic((*risk_loss["v"], g), ref, "cox grad_out")
    check_grad_contract(poison, model, step, check_write, "cox_step")
