"""The C-ABI calls behind ops.py's autograd nodes and the heads' one-call steps, and their arguments, without a GPU:
ops.lib, ops.ptr and ops.stream_ptr are replaced by a recorder and the nodes are driven with CPU tensors (the recorder's
library launches nothing: it returns 0, or a size for a *_workspace_bytes query).

Checked: the sequence of entry points, the descriptor fields, that every call gets the workspace just queried and
every backward the workspace of its forward, and that the scheduling hint a stack node's forward saw reaches its
backward."""
import ctypes as C

import pytest
import torch

from multimodalfusion_amd import _lib, ops

STREAM = 0x5EA


def _snap(a):
    """A call argument as plain values, taken when the call is made (structs are filled in place)."""
    if isinstance(a, type(C.byref(C.c_int()))):
        a = a._obj
    if isinstance(a, _lib.BagGroup):     # host arrays behind pointers: read while the caller keeps them alive
        return {"G": a.G, "offsets": a.offsets[:a.G + 1], "seeds": a.seeds[:a.G] if a.seeds else None}
    if isinstance(a, C.Structure):
        return {name: _snap(getattr(a, name)) for name, _ in a._fields_}
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value
    if isinstance(a, C.Array):
        return [_snap(v) for v in a]
    return a


class Recorder:
    """Stands in for ops.lib (calling it returns the fake library), ops.ptr and ops.stream_ptr."""

    def __init__(self):
        self.calls = []          # (entry point, snapshot of the arguments, return value)
        self.tensors = {}        # data_ptr -> tensor, kept alive so that no address is reused within a case

    def __call__(self):
        return self

    def ptr(self, t):
        if t is None:
            return None
        assert t.is_contiguous()
        self.tensors[t.data_ptr()] = t
        return t.data_ptr()

    def __getattr__(self, name):
        if not name.startswith("mmf_"):
            raise AttributeError(name)

        def entry(*args):
            ret = 4096 + 64 * len(self.calls) if name.endswith("_workspace_bytes") else 0
            self.calls.append((name, [_snap(a) for a in args], ret))
            return ret
        return entry

    @property
    def names(self):
        return [c[0] for c in self.calls]

    def log(self):
        """The calls with every device pointer replaced by "s<k>[+offset]": storage k in order of first appearance.
        Returns (log, {label: bytes of the storage})."""
        labels, sizes = {}, {}

        def lab(v):
            if isinstance(v, dict):
                return {k: lab(x) for k, x in v.items()}
            if isinstance(v, list):
                return [lab(x) for x in v]
            if isinstance(v, int) and not isinstance(v, bool) and v in self.tensors:
                st = self.tensors[v].untyped_storage()
                key = st.data_ptr()
                if key not in labels:
                    labels[key] = f"s{len(labels)}"
                    sizes[labels[key]] = st.nbytes()
                off = v - key
                return labels[key] + (f"+{off}" if off else "")
            return v
        return [(n, lab(a), r) for n, a, r in self.calls], sizes


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "lib", r)
    monkeypatch.setattr(ops, "ptr", r.ptr)
    monkeypatch.setattr(ops, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(ops, "_drop_calls", 0)
    monkeypatch.setattr(ops, "_concurrent", 0)
    monkeypatch.setattr(ops, "_gemm", 0)
    torch.manual_seed(0)
    return r


# argument positions of (workspace pointer, workspace bytes) per entry point
WS_ARGS = {"mmf_amil_forward": (2, 3), "mmf_amil_bf16_forward": (2, 3), "mmf_amil_infer": (2, 3),
           "mmf_amil_bf16_infer": (2, 3), "mmf_amil_head_forward": (3, 4), "mmf_amil_nll_step": (3, 4),
           "mmf_amil_backward": (2, 3), "mmf_amil_bf16_backward": (2, 3), "mmf_attn_net_forward": (2, 3),
           "mmf_attn_net_backward": (2, 3), "mmf_linear_backward": (10, 11)}
BACKWARD_OF = {"mmf_amil_backward": ("mmf_amil_forward", "mmf_amil_head_forward"),
               "mmf_amil_bf16_backward": ("mmf_amil_bf16_forward", "mmf_amil_head_forward"),
               "mmf_attn_net_backward": ("mmf_attn_net_forward",)}
FORWARDS = {f for fs in BACKWARD_OF.values() for f in fs}


def check_workspaces(rec):
    """Every call takes a fresh workspace of the size it just queried; a stack's backward takes its forward's (the
    stacks of one case run their backwards in reverse order)."""
    log, sizes = rec.log()
    fwd_ws, last_query = [], None
    for name, args, ret in log:
        if name.endswith("_workspace_bytes"):
            last_query = ret
            continue
        if name not in WS_ARGS:
            continue
        p, n = WS_ARGS[name]
        if name in BACKWARD_OF:
            fname, fws = fwd_ws.pop()
            assert fname in BACKWARD_OF[name]
            assert (args[p], args[n]) == fws
        else:
            assert args[n] == last_query and sizes[args[p]] == last_query, name
            last_query = None
            if name in FORWARDS:
                fwd_ws.append((name, (args[p], args[n])))
    assert not fwd_ws
    return log


def descs(log, *names):
    return [args[0] for n, args, _ in log if n in names]


def _stack(gated, L=16, H=8, D=4, grad=True):
    mk = lambda *s: torch.randn(*s).requires_grad_(grad)
    return (mk(H, L), mk(H), mk(D, H), mk(D), mk(D, H) if gated else None, mk(D) if gated else None, mk(1, D), mk(1))


def _desc_fields(d):
    return {k: d[k] for k in ("N", "L", "H", "D", "gated", "p_h", "p_att", "seed", "concurrent", "gemm", "sync",
                              "sync_words")}


def _expect(N, L, H, D, gated, p_h, p_att, seed, concurrent=0):
    return dict(N=N, L=L, H=H, D=D, gated=int(gated), p_h=p_h, p_att=p_att, seed=seed, concurrent=concurrent, gemm=0,
                sync=None, sync_words=0)


# ---- the attention stack: AmilPoolFn, AmilHeadFn, amil_infer ------------------------------------------------------------
def run_pool(rec, bf16, gated, dx, concurrent=False):
    x = torch.randn(6, 16, dtype=torch.bfloat16 if bf16 else torch.float32).requires_grad_(dx)
    ps = _stack(gated)
    prev = ops.set_concurrent(concurrent)
    M, A = ops.amil_pool(x, *ps, gated, 0.25, 0.125, 1234)
    ops.set_concurrent(prev)
    (M.sum() + (A.sum() if dx else 0)).backward()
    return x, ps


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dx", [False, True])
def test_amil_pool(rec, bf16, gated, dx):
    if bf16 and dx:
        with pytest.raises(_lib.MmfError, match="leaf"):
            run_pool(rec, bf16, gated, dx)
        assert rec.names == ["mmf_amil_bf16_workspace_bytes", "mmf_amil_bf16_forward"]
        return
    x, ps = run_pool(rec, bf16, gated, dx)
    b = "_bf16" if bf16 else ""
    assert rec.names == [f"mmf_amil{b}_workspace_bytes", f"mmf_amil{b}_forward", f"mmf_amil{b}_backward"]
    log = check_workspaces(rec)
    for d in descs(log, f"mmf_amil{b}_forward", f"mmf_amil{b}_backward"):
        assert _desc_fields(d) == _expect(6, 16, 8, 4, gated, 0.25, 0.125, 1234)
        assert (d["Wb"] is None) == (not gated)
    fwd, bwd = log[1][1], log[2][1]
    assert bwd[:2] == fwd[:2] and bwd[4:6] == fwd[4:6]              # desc, x ... M, A_raw
    assert (bwd[7] is None) == (not dx)                             # gA: set_materialize_grads(False)
    g = bwd[8]
    assert (g["dx"] is None) == (not dx) and (g["dWb"] is None) == (not gated) and g["dW1"] is not None
    assert x.grad is not None if dx else x.grad is None
    assert all(p.grad is not None for p in ps if p is not None)


def run_head(rec, bf16, gated, dx, K, concurrent=False):
    x = torch.randn(6, 16, dtype=torch.bfloat16 if bf16 else torch.float32).requires_grad_(dx)
    ps = _stack(gated)
    Wk, bk = torch.randn(K, 8).requires_grad_(), torch.randn(K).requires_grad_()
    prev = ops.set_concurrent(concurrent)
    hz, S, Y_hat, A = ops.amil_head(x, *ps, Wk, bk, gated, 0.25, 0.125, 99)
    ops.set_concurrent(prev)
    (hz.sum() + S.sum() + (A.sum() if dx else 0)).backward()
    return x, ps, Wk, bk


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dx", [False, True])
@pytest.mark.parametrize("K", [4, 40])
def test_amil_head(rec, bf16, gated, dx, K):
    b = "_bf16" if bf16 else ""
    fwd = ["mmf_amil_head_forward"] if K <= 32 else [f"mmf_amil{b}_forward", "mmf_surv_head_forward"]
    if bf16 and dx:
        with pytest.raises(_lib.MmfError, match="leaf"):
            run_head(rec, bf16, gated, dx, K)
        assert rec.names == [f"mmf_amil{b}_workspace_bytes"] + fwd        # nothing of the backward was issued
        return
    x, ps, Wk, bk = run_head(rec, bf16, gated, dx, K)
    assert rec.names == [f"mmf_amil{b}_workspace_bytes"] + fwd + ["mmf_surv_head_backward", f"mmf_amil{b}_backward"]
    log = check_workspaces(rec)
    for d in descs(log, "mmf_amil_head_forward", f"mmf_amil{b}_forward", f"mmf_amil{b}_backward"):
        assert _desc_fields(d) == _expect(6, 16, 8, 4, gated, 0.25, 0.125, 99)
    if K <= 32:
        assert log[1][1][2] == int(bf16)
        hd = log[1][1][5]
        assert hd["K"] == K and hd["risk"] is None
    else:
        assert log[2][1][3:6] == [1, 8, K]                          # B, F, K of the head on M
    sb = log[-2][1]
    assert sb[5:8] == [1, 8, K]
    assert log[-1][1][6] == sb[8]                                   # dM of the head is the stack's gM
    assert (log[-1][1][8]["dx"] is None) == (not dx)
    assert all(p.grad is not None for p in (*ps, Wk, bk) if p is not None)


@pytest.mark.parametrize("node", ["pool", "head"])
def test_concurrent_hint_of_the_forward_reaches_the_backward(rec, node):
    """The hint is raised around the forward only (pipeline.BagsInFlight holds it through its autograd.grad, the
    multimodal fork through the forward): the backward keeps the value its forward saw."""
    (run_pool(rec, False, True, False, True) if node == "pool" else run_head(rec, False, True, False, 4, True))
    assert ops._concurrent == 0
    log = rec.log()[0]
    ds = descs(log, "mmf_amil_forward", "mmf_amil_head_forward", "mmf_amil_backward")
    assert len(ds) == 2 and [d["concurrent"] for d in ds] == [1, 1]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("gated", [True, False])
def test_amil_infer(rec, bf16, gated):
    x = torch.randn(6, 16, dtype=torch.bfloat16 if bf16 else torch.float32)
    ps = _stack(gated)
    Wk, bk = torch.randn(4, 8), torch.randn(4)
    with torch.no_grad():
        M, A = ops.amil_pool(x, *ps, gated)
        hz, S, Y_hat, A2 = ops.amil_head(x, *ps, Wk, bk, gated)
    b = "_bf16" if bf16 else ""
    assert rec.names == [f"mmf_amil{b}_infer_workspace_bytes", f"mmf_amil{b}_infer"] * 2 + ["mmf_surv_head_forward"]
    log = check_workspaces(rec)
    for d in descs(log, f"mmf_amil{b}_infer"):
        assert _desc_fields(d) == _expect(6, 16, 8, 4, gated, 0.0, 0.0, 0)
        assert d["seed_dev"] is None
    assert M.shape == (1, 8) and A.shape == (1, 6) and hz.shape == (1, 4) and Y_hat.dtype == torch.int64


# ---- the scorer alone and the small nodes --------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dx", [False, True])
def test_attn_net(rec, gated, dx):
    x = torch.randn(6, 8).requires_grad_(dx)
    _, _, *sc = _stack(gated)
    A = ops.attn_net(x, *sc, gated, 0.25, 77)
    A.sum().backward()
    assert rec.names == ["mmf_attn_net_workspace_bytes", "mmf_attn_net_forward", "mmf_attn_net_backward"]
    assert rec.calls[0][1] == [6, 8, 4, int(gated)]
    log = check_workspaces(rec)
    for d in descs(log, "mmf_attn_net_forward", "mmf_attn_net_backward"):
        assert _desc_fields(d) == _expect(6, 8, 8, 4, gated, 0.0, 0.25, 77)
        assert d["W1"] is None and d["b1"] is None
    g = log[2][1][5]
    assert g["dW1"] is None and g["db1"] is None and (g["dWb"] is None) == (not gated) and (g["dx"] is None) == (not dx)


@pytest.mark.parametrize("nseg", [1, 4])
def test_linear_cat(rec, nseg):
    xs = [torch.randn(5, 6).requires_grad_(nseg == 1) for _ in range(nseg)]
    W, b = torch.randn(7, 6 * nseg).requires_grad_(), torch.randn(7).requires_grad_()
    ops.linear_cat(xs, W, b).sum().backward()
    assert rec.names == ["mmf_linear_forward_workspace_bytes", "mmf_linear_forward",
                         "mmf_linear_backward_workspace_bytes", "mmf_linear_backward"]
    assert rec.calls[0][1] == [5, 7, nseg, 6]
    fa = rec.calls[1][1]
    assert fa[1:4] == [nseg, 6, 5] and fa[13:17] == [None, 0, None, 0]     # CPU: no tick words, so no workspace
    check_workspaces(rec)
    assert (rec.calls[3][1][9] is None) == (nseg != 1)
    assert W.grad is not None and b.grad is not None


@pytest.mark.parametrize("dx", [False, True])
def test_dense_and_mlp(rec, dx):
    x = torch.randn(3, 5).requires_grad_(dx)
    W, b = torch.randn(4, 5).requires_grad_(), torch.randn(4).requires_grad_()
    ops.dense(x, W, b, act="relu", drop_kind="dropout", drop_p=0.25, seed=5 + (1 << 33), site=2).sum().backward()
    W2, b2 = torch.randn(2, 4).requires_grad_(), torch.randn(2).requires_grad_()
    layers = [(W, b, "selu", "alpha", 0.25, 0), (W2, b2, "selu", "alpha", 0.25, 1)]
    ops.mlp(x, layers, seed=6).sum().backward()
    assert rec.names == ["mmf_dense_forward", "mmf_dense_backward", "mmf_dense_forward", "mmf_dense_forward",
                         "mmf_dense_backward", "mmf_dense_backward"]
    f, bw = rec.calls[0][1], rec.calls[1][1]
    assert f[3:11] == [3, 5, 4, ops.ACT["relu"], 1, 0.25, 5, 2] and bw[4:12] == [3, 5, 4, ops.ACT["relu"], 1, 0.25, 5, 2]
    assert bw[1] == f[12] and bw[2] == f[0]                          # y, x of the forward
    assert (bw[14] is None) == (not dx) and bw[15] is not None
    assert [c[1][10] for c in rec.calls[2:4]] == [0, 1] and [c[1][11] for c in rec.calls[4:]] == [1, 0]   # sites
    assert (rec.calls[5][1][14] is None) == (not dx) and rec.calls[4][1][14] is not None


def test_kron_ones(rec):
    os_ = [torch.randn(2, 3).requires_grad_() for _ in range(3)]
    out = ops.kron_ones(os_, drop_p=0.25, seed=8, site=8)
    assert out.shape == (2, 64)
    out.sum().backward()
    assert rec.names == ["mmf_kron_forward", "mmf_kron_backward"]
    f, b = rec.calls[0][1], rec.calls[1][1]
    assert f[1:7] == [3, 3, 2, 0.25, 8, 8] and b[2:8] == [3, 3, 2, 0.25, 8, 8] and b[1] == f[0]
    assert all(o.grad is not None for o in os_)


def _xfusion_module():
    from multimodalfusion_amd.models.model_modules import XlinearFusion
    return XlinearFusion(dim=32, scale_dim=16, mmhid1=8, mmhid2=8, num_modalities=3).train()


def test_xfusion(rec):
    mod = _xfusion_module()
    vs = [torch.randn(1, 32).requires_grad_() for _ in range(3)]
    mod(vs, seed=21).sum().backward()
    assert rec.names == ["mmf_xreduce_forward", "mmf_kron_forward", "mmf_dense_forward", "mmf_dense_forward",
                         "mmf_dense_backward", "mmf_dense_backward", "mmf_kron_backward", "mmf_xreduce_backward"]
    assert [c[1][1:3] for c in (rec.calls[0], rec.calls[7])] == [[0.25, 21]] * 2
    assert rec.calls[1][1][1:7] == [3, 2, 1, 0.25, 21, 8] and rec.calls[6][1][2:8] == [3, 2, 1, 0.25, 21, 8]
    assert [rec.calls[i][1][10] for i in (2, 3)] == [9, 10] and [rec.calls[i][1][11] for i in (4, 5)] == [10, 9]
    assert all(v.grad is not None for v in vs) and all(p.grad is not None for p in mod.parameters())


def test_surv_head(rec):
    feat = torch.randn(2, 8).requires_grad_()
    Wk, bk = torch.randn(4, 8).requires_grad_(), torch.randn(4).requires_grad_()
    hz, S, Y_hat = ops.surv_head(feat, Wk, bk)
    (hz.sum() + S.sum()).backward()
    assert rec.names == ["mmf_surv_head_forward", "mmf_surv_head_backward"]
    f, b = rec.calls[0][1], rec.calls[1][1]
    assert f[3:6] == [2, 8, 4] and b[5:8] == [2, 8, 4] and b[2] == f[7] and b[3] == f[0]
    assert feat.grad is not None and Wk.grad is not None and bk.grad is not None


# ---- the heads' one-call steps ---------------------------------------------------------------------------------------
MODS = ["T1", "T2", "T1Gd", "FLAIR"]


def run_radio_step(rec, nmod):
    from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio
    model = MIL_Attention_fc_surv_radio(modalities=MODS[:nmod]).train()
    bags = {m: torch.randn(5, 1024) for m in MODS[:nmod]}
    out = model.nll_step(torch.tensor([1]), torch.tensor([0.0]), alpha=0.4, **bags)
    return model, out


@pytest.mark.parametrize("nmod", [1, 4])
def test_radio_nll_step(rec, nmod):
    model, _ = run_radio_step(rec, nmod)
    linear = nmod > 1
    assert rec.names == (["mmf_linear_forward_workspace_bytes", "mmf_linear_forward"] if linear else []) + \
        ["mmf_amil_workspace_bytes", "mmf_amil_nll_step"] + \
        (["mmf_linear_backward_workspace_bytes", "mmf_linear_backward"] if linear else [])
    log = check_workspaces(rec)
    (d,) = descs(log, "mmf_amil_nll_step")
    assert _desc_fields(d) == _expect(5, 1024, 256, 256, True, 0.25, 0.25, d["seed"])
    step = log[3 if linear else 1][1]
    if linear:
        lf, lb = log[1][1], log[5][1]
        assert step[1] == lf[12] and step[8]["dx"] == lb[0]       # reduce_dim's output is the bag, dx its gradient
        assert lb[9] is None
    else:
        assert step[8]["dx"] is None
    assert all(p.grad is not None for p in model.parameters())


def run_mm_step(rec, fusion, bf16=False):
    from multimodalfusion_amd.models import MM_MIL_Attention_fc_surv
    model = MM_MIL_Attention_fc_surv(fusion=fusion, dropout=True).train()
    kw = {m: torch.randn(4, 1024) for m in MODS}
    kw["path_features"] = torch.randn(7, 1024, dtype=torch.bfloat16 if bf16 else torch.float32)
    kw["genomic_features"] = torch.randn(80)
    out = model.nll_step(torch.tensor([2]), torch.tensor([0.0]), alpha=0.4, **kw)
    return model, out


@pytest.mark.parametrize("fusion", ["concat", "tensor"])
@pytest.mark.parametrize("bf16", [False, True])
def test_mm_nll_step(rec, fusion, bf16):
    model, out = run_mm_step(rec, fusion, bf16)
    b = "_bf16" if bf16 else ""
    head = (["mmf_surv_head_nll_step"] if fusion == "concat" else
            ["mmf_xreduce_forward", "mmf_kron_forward", "mmf_dense_forward", "mmf_dense_forward", "mmf_dense_forward",
             "mmf_surv_head_nll_step", "mmf_dense_backward", "mmf_dense_backward", "mmf_dense_backward",
             "mmf_kron_backward", "mmf_xreduce_backward"])
    assert rec.names == ["mmf_linear_forward_workspace_bytes", "mmf_linear_forward", "mmf_amil_workspace_bytes",
                         "mmf_amil_forward", f"mmf_amil{b}_workspace_bytes", f"mmf_amil{b}_forward",
                         "mmf_dense_forward", "mmf_dense_forward"] + head + \
        [f"mmf_amil{b}_backward", "mmf_dense_backward", "mmf_dense_backward", "mmf_amil_backward",
         "mmf_linear_backward_workspace_bytes", "mmf_linear_backward"]
    log = check_workspaces(rec)
    radio, path = descs(log, "mmf_amil_forward", f"mmf_amil{b}_forward")[:2]
    assert _desc_fields(radio) == _expect(4, 1024, 256, 256, True, 0.25, 0.25, radio["seed"])
    assert _desc_fields(path) == _expect(7, 1024, 256, 256, True, 0.25, 0.25, path["seed"])
    assert radio["seed"] != path["seed"]
    bw = [args for n, args, _ in log if n.startswith("mmf_amil") and n.endswith("_backward")]
    assert bw[0][8]["dx"] is None and bw[1][8]["dx"] == log[-1][1][0]   # path: no dx; radio: dx into reduce_dim
    assert [_desc_fields(a[0]) for a in bw] == [_desc_fields(path), _desc_fields(radio)]
    feat = log[3][1][4]                                                # radio M: slot 0 of the feature vector
    assert log[5][1][4] == feat + "+1024" and log[7][1][12] == feat + "+2048"
    hazards, S, Y_hat, A_raw, loss, risk = out
    assert set(A_raw) == {"radiology", "pathology"} and A_raw["pathology"].shape == (1, 7)
    assert all(p.grad is not None for p in model.parameters())


# ---- the grouped passes: one accumulation or evaluation window per call ----------------------------------------------
SIZES = [3, 1, 4]


def _group_case(rec, monkeypatch, gated, K, radio=0, grads=True):
    """Stack, classifier, (reduce_dim) and their gradient buffers of a grouped call; the seed word is a live tensor."""
    word = torch.zeros(1, dtype=torch.int32)
    monkeypatch.setattr(ops, "_seed_word", word)
    stack = _stack(gated, grad=False)
    Wk, bk = torch.randn(K, 8), torch.randn(K)
    red = (torch.randn(16, 16 * radio), torch.randn(16)) if radio else ()
    ps = (*red, *stack, Wk, bk)
    gs = tuple(None if p is None else torch.zeros_like(p) for p in ps) if grads else None
    return word, stack, Wk, bk, red, gs


def _check_window(rec, query, entry, qargs, ws_at):
    """[query, entry] with the query's arguments; the entry gets a fresh workspace of the size just queried.
    Returns the entry's labelled arguments."""
    assert rec.names == [query, entry]
    log, sizes = rec.log()
    assert list(rec.calls[0][1][0]) == [0, 3, 4, 8] and rec.calls[0][1][1:] == qargs
    args = log[1][1]
    assert args[ws_at + 1] == log[0][2] and sizes[args[ws_at]] == log[0][2]
    assert args[-1] == STREAM
    return args


def _check_desc(d, word, L, gated, p_h, p_att, train):
    assert _desc_fields(d) == _expect(sum(SIZES), L, 8, 4, gated, p_h, p_att, 0)
    assert (d["seed_dev"] is not None) == train              # the seed word: training only
    assert (d["Wb"] is None) == (not gated) and d["W1"] is not None and d["trace"] is None


def _check_group(grp, seeds):
    assert grp == {"G": 3, "offsets": [0, 3, 4, 8], "seeds": seeds}


@pytest.mark.parametrize("gated", [True, False])
def test_amil_nll_step_group(rec, monkeypatch, gated):
    word, stack, Wk, bk, _, gs = _group_case(rec, monkeypatch, gated, 4)
    x = torch.randn(8, 16)
    Y, c = torch.tensor([1, 0, 3]), torch.tensor([0.0, 1.0, 0.0])
    hz, S, Y_hat, A, loss, risk = ops.amil_nll_step_group(x, SIZES, stack, Wk, bk, gated, Y, c, 0.4, gs, loss_scale=0.5,
                                                          accumulate=True, p_h=0.25, p_att=0.125, seeds=[7, 8, 1 << 32 | 9])
    a = _check_window(rec, "mmf_amil_group_workspace_bytes", "mmf_amil_nll_step_group", [3, 16, 8, 4, int(gated)], 3)
    d, grp, xp, _, _, hd, tg, A_raw, g, _ = a
    _check_desc(d, word, 16, gated, 0.25, 0.125, train=True)
    _check_group(grp, [7, 8, 9])
    assert hd["K"] == 4 and all(hd[n] is not None for n in ("Wk", "bk", "logits", "hazards", "S", "Y_hat", "risk"))
    assert tg["alpha"] == pytest.approx(0.4) and tg["loss_scale"] == 0.5 and tg["accumulate"] == 1
    assert all(tg[n] is not None for n in ("Y", "c", "loss", "dWk", "dbk"))
    assert len({tg["dWk"], tg["dbk"], tg["loss"]}) == 3
    assert g["dx"] is None and (g["dWb"] is None) == (not gated) and (g["dbb"] is None) == (not gated)
    assert all(g[n] is not None for n in ("dW1", "db1", "dWa", "dba", "dWc", "dbc"))
    assert hz.shape == (3, 4) and S.shape == (3, 4) and Y_hat.shape == (3, 1) and Y_hat.dtype == torch.int64
    assert loss.shape == (3,) and risk.shape == (3,)
    assert [tuple(v.shape) for v in A] == [(1, 3), (1, 1), (1, 4)]
    assert A[1].data_ptr() == A[0].data_ptr() + 12 and rec.tensors[A[0].data_ptr()].numel() == 8   # views of one A_raw
    with pytest.raises(IndexError, match="label out of range"):
        ops.amil_nll_step_group(x, SIZES, stack, Wk, bk, gated, torch.tensor([1, 4, 3]), c, 0.4, gs)
    assert len(rec.calls) == 2


def test_radio_nll_step_group(rec, monkeypatch):
    word, stack, Wk, bk, (Wr, br), gs = _group_case(rec, monkeypatch, True, 4, radio=3)
    xs = [torch.randn(8, 16) for _ in range(3)]
    Y, c = torch.tensor([1, 0, 3]), torch.tensor([0.0, 1.0, 0.0])
    hz, S, Y_hat, A, loss, risk = ops.radio_nll_step_group(xs, SIZES, Wr, br, stack, Wk, bk, True, Y, c, 0.4, gs,
                                                           p_h=0.25, p_att=0.25, seeds=[7, 8, 9])
    a = _check_window(rec, "mmf_radio_group_workspace_bytes", "mmf_radio_nll_step_group", [3, 3, 16, 8, 4, 1], 3)
    d, grp, rd, _, _, hd, tg, A_raw, g, _ = a
    _check_desc(d, word, 16, True, 0.25, 0.25, train=True)
    _check_group(grp, [7, 8, 9])
    assert rd["nseg"] == 3 and rd["kseg"] == 16 and all(rd[n] is not None for n in ("x", "W", "bias", "dW", "db"))
    assert rd["dW"] != rd["W"] and rd["db"] != rd["bias"]
    assert hd["K"] == 4 and tg["loss_scale"] == 1.0 and tg["accumulate"] == 0
    assert tg["dWk"] is not None and tg["dbk"] is not None
    assert g["dx"] is None and g["dW1"] is not None and g["dWb"] is not None
    assert hz.shape == (3, 4) and S.shape == (3, 4) and Y_hat.shape == (3, 1) and loss.shape == (3,) and risk.shape == (3,)
    assert [tuple(v.shape) for v in A] == [(1, 3), (1, 1), (1, 4)]


def test_amil_infer_group_fp32_with_head_and_labels(rec, monkeypatch):
    word, stack, Wk, bk, _, _ = _group_case(rec, monkeypatch, True, 4, grads=False)
    x = torch.randn(8, 16)
    Y, c = torch.tensor([1, 9, 3]), torch.tensor([0.0, 1.0, 0.0])       # a label out of range goes through: NaN loss
    hz, S, Y_hat, risk, A, M, loss = ops.amil_infer_group(x, SIZES, stack, True, Wk, bk, Y, c, alpha=0.4)
    a = _check_window(rec, "mmf_amil_group_infer_workspace_bytes", "mmf_amil_infer_group", [3, 16, 8, 4, 1, 0], 4)
    d, grp, xp, x_bf16, _, _, hd, tg, Mp, A_raw, _ = a
    _check_desc(d, word, 16, True, 0.0, 0.0, train=False)
    _check_group(grp, None)
    assert x_bf16 == 0 and Mp is None and A_raw is not None
    assert hd["K"] == 4 and all(hd[n] is not None for n in ("Wk", "bk", "logits", "hazards", "S", "Y_hat", "risk"))
    assert tg["alpha"] == pytest.approx(0.4) and tg["eps"] == pytest.approx(1e-7) and tg["loss_scale"] == 1.0
    assert tg["dWk"] is None and tg["dbk"] is None and tg["accumulate"] == 0
    assert all(tg[n] is not None for n in ("Y", "c", "loss"))
    assert M is None and hz.shape == (3, 4) and S.shape == (3, 4) and Y_hat.shape == (3, 1) and risk.shape == (3,)
    assert loss.shape == (3,) and [tuple(v.shape) for v in A] == [(1, 3), (1, 1), (1, 4)]


def test_amil_infer_group_bf16_for_M_alone(rec, monkeypatch):
    word, stack, _, _, _, _ = _group_case(rec, monkeypatch, False, 4, grads=False)
    x = torch.randn(8, 16).to(torch.bfloat16)
    hz, S, Y_hat, risk, A, M, loss = ops.amil_infer_group(x, SIZES, stack, False, want_M=True)
    a = _check_window(rec, "mmf_amil_group_infer_workspace_bytes", "mmf_amil_infer_group", [3, 16, 8, 4, 0, 1], 4)
    d, grp, xp, x_bf16, _, _, hd, tg, Mp, A_raw, _ = a
    _check_desc(d, word, 16, False, 0.0, 0.0, train=False)
    _check_group(grp, None)
    assert x_bf16 == 1 and hd is None and tg is None and Mp is not None
    assert (hz, S, Y_hat, risk, loss) == (None,) * 5
    assert M.shape == (3, 8) and M.dtype == torch.float32 and [tuple(v.shape) for v in A] == [(1, 3), (1, 1), (1, 4)]
    with pytest.raises(_lib.MmfError, match="nothing to compute"):
        ops.amil_infer_group(x, SIZES, stack, False)
    with pytest.raises(_lib.MmfError, match="a loss needs the classifier head"):
        ops.amil_infer_group(x, SIZES, stack, False, Y=torch.tensor([0, 0, 0]), c=torch.zeros(3), want_M=True)
    assert len(rec.calls) == 2


def test_radio_infer_group(rec, monkeypatch):
    word, stack, Wk, bk, (Wr, br), _ = _group_case(rec, monkeypatch, True, 4, radio=2, grads=False)
    xs = [torch.randn(8, 16) for _ in range(2)]
    hz, S, Y_hat, risk, A, M, loss = ops.radio_infer_group(xs, SIZES, Wr, br, stack, True, Wk, bk, want_M=True)
    a = _check_window(rec, "mmf_radio_group_infer_workspace_bytes", "mmf_radio_infer_group", [3, 2, 16, 8, 4, 1], 3)
    d, grp, rd, _, _, hd, tg, Mp, A_raw, _ = a
    _check_desc(d, word, 16, True, 0.0, 0.0, train=False)
    _check_group(grp, None)
    assert rd["nseg"] == 2 and rd["kseg"] == 16 and all(rd[n] is not None for n in ("x", "W", "bias"))
    assert rd["dW"] is None and rd["db"] is None
    assert hd["K"] == 4 and hd["risk"] is not None and tg is None and Mp is not None
    assert loss is None and M.shape == (3, 8) and hz.shape == (3, 4) and S.shape == (3, 4) and Y_hat.shape == (3, 1)
    assert risk.shape == (3,) and [tuple(v.shape) for v in A] == [(1, 3), (1, 1), (1, 4)]
