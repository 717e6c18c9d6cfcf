"""CPU checks of the argument contract of the attention-stack entry points (include/mmf_amil.h): null pointers give
MMF_ERR_ARG (-1), unsupported shapes MMF_ERR_SHAPE (-2), misaligned pointers MMF_ERR_ALIGN (-3), and a workspace one byte
below its *_workspace_bytes query MMF_ERR_WORKSPACE (-4) -- which ties each entry point's workspace carving to its query.
Where several checks fail, the code that wins is pinned too.

Every pointer is a fake 16-byte-aligned host address that is never dereferenced: each case fails a check before the first
launch.  Needs the built library, not a GPU."""
import ctypes as C

import pytest

ARG, SHAPE, ALIGN, WS = -1, -2, -3, -4
BF16X3 = 1
_next = [0x10000000]


def fake():
    _next[0] += 0x1000
    return _next[0]


def lib():
    from multimodalfusion_amd import _lib
    return _lib.lib()


def desc(N=1000, L=1024, H=512, D=256, gated=1, **kw):
    from multimodalfusion_amd import _lib
    d = _lib.AmilDesc(N=N, L=L, H=H, D=D, gated=gated)
    for n in ("W1", "b1", "Wa", "ba", "Wb", "bb", "Wc", "bc"):
        setattr(d, n, fake())
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def grads(**kw):
    from multimodalfusion_amd import _lib
    g = _lib.AmilGrads(**{n: fake() for n in ("dW1", "db1", "dWa", "dba", "dWb", "dbb", "dWc", "dbc")})
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def head(K=4):
    from multimodalfusion_amd import _lib
    return _lib.SurvHead(Wk=fake(), bk=fake(), K=K, logits=fake(), hazards=fake(), S=fake(), Y_hat=fake())


def target(**kw):
    from multimodalfusion_amd import _lib
    t = _lib.NllTarget(Y=fake(), c=fake(), loss_scale=1.0, loss=fake(), dWk=fake(), dbk=fake())
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def ref(s):
    return None if s is None else C.byref(s)


def _ws_query(name, d):
    d = d or desc()
    return getattr(lib(), name)(d.N, d.L, d.H, d.D, d.gated)


# ---- fp32 / bf16 forward, inference and backward -------------------------------------------------------------------
FWD = [("mmf_amil_forward", "mmf_amil_workspace_bytes"), ("mmf_amil_infer", "mmf_amil_infer_workspace_bytes"),
       ("mmf_amil_bf16_forward", "mmf_amil_bf16_workspace_bytes"),
       ("mmf_amil_bf16_infer", "mmf_amil_bf16_infer_workspace_bytes")]


@pytest.mark.parametrize("fn,query", FWD)
@pytest.mark.parametrize("gated", [0, 1])
def test_forward_contract(fn, query, gated):
    f = getattr(lib(), fn)

    def call(d, x=True, ws=True, wsb=None, A=True):
        wsb = _ws_query(query, d) if wsb is None else wsb
        return f(ref(d), fake() if x is True else x, fake() if ws is True else ws, wsb, fake(), fake() if A else None, None)

    d = desc(gated=gated)
    full = _ws_query(query, d)
    assert full > 0
    assert f(None, fake(), fake(), full, fake(), fake(), None) == ARG
    assert call(d, x=None) == ARG
    assert call(d, ws=None) == ARG
    assert call(d, A=False) == ARG
    assert call(desc(gated=gated, W1=None)) == ARG
    assert call(desc(gated=gated, p_h=1.0)) == ARG
    assert call(desc(gated=gated, gemm=7)) == ARG
    assert call(desc(gated=gated, H=384), wsb=1 << 40) == SHAPE
    assert call(desc(gated=gated, D=192), wsb=1 << 40) == SHAPE
    assert call(desc(gated=gated, N=0), wsb=1 << 40) == SHAPE
    assert call(desc(gated=gated, H=384, W1=None), wsb=1 << 40) == ARG       # the pointers are checked before the shape
    assert call(d, x=fake() + 4) == ALIGN
    assert call(d, ws=fake() + 8) == ALIGN
    assert call(d, x=fake() + 4, ws=None) == ARG                              # null before alignment
    assert call(d, wsb=full - 1) == WS
    assert call(d, x=fake() + 4, wsb=full - 1) == ALIGN                       # alignment before the workspace
    if gated:
        assert call(desc(gated=1, Wb=None)) == ARG
    if fn.startswith("mmf_amil_bf16"):
        assert call(desc(gated=gated, L=1056), wsb=1 << 40) == SHAPE         # bf16: L % 64
    else:
        assert call(desc(gated=gated, W1=fake() + 4)) == ALIGN
        assert call(desc(gated=gated, Wa=fake() + 4)) == ALIGN
        assert call(desc(gated=gated, L=1056), wsb=0) == WS                  # fp32 takes L % 32


BWD = [("mmf_amil_backward", "mmf_amil_workspace_bytes"), ("mmf_amil_bf16_backward", "mmf_amil_bf16_workspace_bytes")]


@pytest.mark.parametrize("fn,query", BWD)
@pytest.mark.parametrize("gated", [0, 1])
def test_backward_contract(fn, query, gated):
    f = getattr(lib(), fn)
    bf16 = "bf16" in fn

    def call(d, g, x=True, ws=True, wsb=None, M=True, dM=True, A=True):
        wsb = _ws_query(query, d) if wsb is None else wsb
        return f(ref(d), fake() if x is True else x, fake() if ws is True else ws, wsb, fake() if M else None,
                 fake() if A else None, fake() if dM else None, None, ref(g), None)

    d = desc(gated=gated)
    full = _ws_query(query, d)
    assert call(d, grads(), M=False) == ARG
    assert call(d, grads(), dM=False) == ARG
    assert call(d, grads(), M=False, wsb=1) == ARG
    assert call(None, grads()) == ARG
    assert call(d, None) == ARG
    assert call(d, grads(), x=None) == ARG
    assert call(d, grads(), ws=None) == ARG
    assert call(d, grads(), A=False) == ARG
    for n in ("dW1", "db1", "dWa", "dba", "dWc", "dbc"):
        assert call(d, grads(**{n: None})) == ARG, n
    assert call(d, grads(dWb=None, dbb=None), wsb=full - 1) == (ARG if gated else WS)
    if gated:
        assert call(d, grads(dWb=None)) == ARG
        assert call(d, grads(dbb=None)) == ARG
        assert call(d, grads(dWb=fake() + 4)) == ALIGN
    assert call(desc(gated=gated, H=384), grads(), wsb=1 << 40) == SHAPE
    assert call(desc(gated=gated, H=384), grads(dW1=None), wsb=1 << 40) == SHAPE   # the descriptor before the gradients
    assert call(d, grads(dW1=fake() + 4)) == ALIGN
    assert call(d, grads(dWa=fake() + 4)) == ALIGN
    assert call(d, grads(dW1=fake() + 4, dWc=None)) == ARG                          # null before alignment
    assert call(d, grads(), wsb=full - 1) == WS
    assert call(d, grads(dWa=fake() + 4), wsb=full - 1) == ALIGN
    if bf16:
        assert call(d, grads(dx=fake())) == ARG                                       # the bf16 bag is a leaf
        assert call(d, grads(dx=fake(), dWa=fake() + 4)) == ARG
        assert call(desc(gated=gated, L=1056), grads(), wsb=1 << 40) == SHAPE
    else:
        assert call(d, grads(dx=fake() + 4)) == ALIGN
        assert call(d, grads(dx=fake()), wsb=full - 1) == WS


# ---- one-call head forward and training step ------------------------------------------------------------------------
def _query(x_bf16, d):
    name = "mmf_amil_bf16_workspace_bytes" if x_bf16 else "mmf_amil_workspace_bytes"
    return _ws_query(name, d)


@pytest.mark.parametrize("x_bf16", [0, 1])
def test_head_forward_contract(x_bf16):
    f = lib().mmf_amil_head_forward

    def call(d, h, x=True, wsb=None, M=True):
        wsb = _query(x_bf16, d) if wsb is None else wsb
        return f(ref(d), fake() if x is True else x, x_bf16, fake(), wsb, ref(h), fake() if M else None, fake(), None)

    d = desc()
    full = _query(x_bf16, d)
    assert call(None, head()) == ARG
    assert call(d, head(), M=False) == ARG
    assert call(d, None) == ARG
    assert call(d, head(K=0)) == SHAPE
    assert call(d, head(K=33)) == SHAPE
    h = head()
    h.hazards = None
    assert call(d, h) == ARG
    assert call(desc(H=384), head(), wsb=1 << 40) == SHAPE
    assert call(desc(H=384), head(K=0), wsb=1 << 40) == SHAPE
    assert call(d, head(), x=None) == ARG
    assert call(d, head(), x=fake() + 4) == ALIGN
    assert call(d, head(), wsb=full - 1) == WS


@pytest.mark.parametrize("x_bf16", [0, 1])
@pytest.mark.parametrize("gated", [0, 1])
def test_nll_step_contract(x_bf16, gated):
    f = lib().mmf_amil_nll_step

    def call(d, g, t, h=None, x=True, wsb=None, A=True):
        wsb = _query(x_bf16, d) if wsb is None else wsb
        return f(ref(d), fake() if x is True else x, x_bf16, fake(), wsb, ref(h or head()), ref(t),
                 fake() if A else None, ref(g), None)

    d = desc(gated=gated)
    full = _query(x_bf16, d)
    assert call(None, grads(), target()) == ARG
    assert call(d, None, target()) == ARG
    assert call(d, grads(), None) == ARG
    for n in ("Y", "c", "loss", "dWk", "dbk"):
        assert call(d, grads(), target(**{n: None})) == ARG, n
    assert call(d, grads(), target(), h=head(K=0)) == SHAPE
    assert call(d, grads(), target(), A=False) == ARG
    assert call(d, grads(), target(), x=None) == ARG
    # (the gradient pointers are checked by the backward half, after the forward's launches)
    assert call(desc(gated=gated, H=384), grads(), target(), wsb=1 << 40) == SHAPE
    assert call(desc(gated=gated, H=384), grads(), target(), h=head(K=0), wsb=1 << 40) == SHAPE
    assert call(d, grads(), target(), x=fake() + 4) == ALIGN
    assert call(d, grads(), target(), wsb=full - 1) == WS
    if gated:
        assert call(desc(gated=1, bb=None), grads(), target()) == ARG


# ---- grouped steps --------------------------------------------------------------------------------------------------
def group(offsets, seeds=True):
    from multimodalfusion_amd import _lib
    G = len(offsets) - 1
    off = (C.c_int64 * len(offsets))(*offsets)
    sd = (C.c_uint32 * G)(*range(1, G + 1)) if seeds else None
    grp = _lib.BagGroup(G=G, offsets=off, seeds=sd)
    grp._keep = (off, sd)
    return grp


OFFS = [0, 1000, 1017, 3000]


def test_group_step_contract():
    f = lib().mmf_amil_nll_step_group

    def query(d, offs=OFFS):
        d = d or desc(N=3000)
        return lib().mmf_amil_group_workspace_bytes((C.c_int64 * len(offs))(*offs), len(offs) - 1, d.L, d.H, d.D, d.gated)

    def call(d, g, grp=None, t=None, h=None, x=True, ws=True, wsb=None, A=True):
        wsb = query(d) if wsb is None else wsb
        return f(ref(d), ref(grp or group(OFFS)), fake() if x is True else x, fake() if ws is True else ws, wsb,
                 ref(h or head()), ref(t or target()), fake() if A else None, ref(g), None)

    d = desc(N=3000)
    full = query(d)
    assert full > 0
    assert call(None, grads()) == ARG
    assert call(d, None) == ARG
    assert f(ref(d), None, fake(), fake(), full, ref(head()), ref(target()), fake(), ref(grads()), None) == ARG
    assert f(ref(d), ref(group(OFFS)), fake(), fake(), full, ref(head()), None, fake(), ref(grads()), None) == ARG
    # refused before the descriptor is checked: bf16x3, an input gradient, no seeds
    assert call(desc(N=3000, H=384, gemm=BF16X3), grads(), wsb=1 << 40) == ARG
    assert call(desc(N=3000, H=384), grads(dx=fake()), wsb=1 << 40) == ARG
    assert call(desc(N=3000, H=384), grads(), grp=group(OFFS, seeds=False), wsb=1 << 40) == ARG
    # the offset table, then the descriptor, then the head
    assert call(d, grads(), grp=group([0, 1000, 1000, 3000])) == SHAPE
    assert call(d, grads(), grp=group([5, 1000, 3000])) == SHAPE
    assert call(desc(N=2999), grads()) == SHAPE
    assert call(desc(N=3000, H=384), grads(), wsb=1 << 40) == SHAPE
    assert call(desc(N=3000, W1=None), grads()) == ARG
    assert call(desc(N=3000, p_att=1.0), grads()) == ARG
    assert call(d, grads(), h=head(K=0)) == SHAPE
    assert call(desc(N=3000, H=384), grads(), h=head(K=0), wsb=1 << 40) == SHAPE
    assert call(d, grads(), t=target(dWk=None)) == ARG
    assert call(d, grads(), x=None) == ARG
    assert call(d, grads(), ws=None) == ARG
    assert call(d, grads(), A=False) == ARG
    for n in ("dW1", "db1", "dWa", "dba", "dWb", "dbb", "dWc", "dbc"):
        assert call(d, grads(**{n: None})) == ARG, n
    assert call(d, grads(), x=fake() + 4) == ALIGN
    assert call(d, grads(), ws=fake() + 4) == ALIGN
    assert call(desc(N=3000, Wb=fake() + 4), grads()) == ALIGN
    assert call(d, grads(dWb=fake() + 4)) == ALIGN
    assert call(d, grads(dW1=fake() + 4, dbc=None)) == ARG
    assert call(d, grads(), wsb=full - 1) == WS
    assert call(d, grads(), x=fake() + 4, wsb=full - 1) == ALIGN


def test_radio_group_step_contract():
    from multimodalfusion_amd import _lib
    f = lib().mmf_radio_nll_step_group
    L = 1024

    def radio(nseg=4, kseg=L, xs=None, **kw):
        xs = xs if xs is not None else [fake() for _ in range(nseg)]
        arr = (C.c_void_p * len(xs))(*xs)
        r = _lib.RadioReduce(x=C.cast(arr, C.POINTER(C.c_void_p)), nseg=nseg, kseg=kseg, W=fake(), bias=fake(),
                             dW=fake(), db=fake())
        for k, v in kw.items():
            setattr(r, k, v)
        r._keep = arr
        return r

    def query(d, nseg=4, offs=OFFS):
        d = d or desc(N=3000, L=L)
        return lib().mmf_radio_group_workspace_bytes((C.c_int64 * len(offs))(*offs), len(offs) - 1, nseg, L, d.H, d.D,
                                                     d.gated)

    def call(d, g, rd, grp=None, h=None, ws=True, wsb=None):
        wsb = query(d, rd.nseg if rd is not None and 2 <= rd.nseg <= 4 else 4) if wsb is None else wsb
        return f(ref(d), ref(grp or group(OFFS)), ref(rd), fake() if ws is True else ws, wsb, ref(h or head()),
                 ref(target()), fake(), ref(g), None)

    d = desc(N=3000, L=L)
    for nseg in (2, 3, 4):
        full = query(d, nseg)
        assert full > 0
        assert call(d, grads(), radio(nseg), wsb=full - 1) == WS
    assert call(d, grads(), None) == ARG
    r = radio()
    r.x = None
    assert call(d, grads(), r) == ARG
    assert call(d, grads(), radio(nseg=1, xs=[fake()] * 4), wsb=1 << 40) == SHAPE
    assert call(d, grads(), radio(nseg=5, xs=[fake()] * 5), wsb=1 << 40) == SHAPE
    assert call(desc(N=3000, L=L, H=384), grads(), radio(nseg=5, xs=[fake()] * 5), wsb=1 << 40) == SHAPE
    assert call(d, grads(dx=fake()), radio()) == ARG
    assert call(desc(N=3000, L=L, gemm=BF16X3), grads(), radio()) == ARG
    assert call(d, grads(), radio(), grp=group(OFFS, seeds=False)) == ARG
    assert call(desc(N=3000, L=L, H=384), grads(), radio(), wsb=1 << 40) == SHAPE
    assert call(d, grads(), radio(xs=[None, fake(), fake(), fake()])) == ARG     # the stack's input is x[0]
    assert call(d, grads(), radio(xs=[fake() + 4, fake(), fake(), fake()])) == ALIGN
    assert call(d, grads(), radio(kseg=512)) == SHAPE
    big = desc(N=140000, L=L)
    big_offs = [0, 70000, 140000]
    assert call(big, grads(), radio(), grp=group(big_offs), wsb=1 << 40) == SHAPE         # [sum N x 4 L] >= 2 GiB
    for n in ("W", "bias", "dW", "db"):
        assert call(d, grads(), radio(**{n: None})) == ARG, n
    assert call(d, grads(), radio(xs=[fake(), fake(), None, fake()])) == ARG
    assert call(d, grads(), radio(xs=[fake(), fake(), fake() + 4, fake()])) == ALIGN
    assert call(d, grads(), radio(xs=[fake(), fake(), fake() + 4, None])) == ARG     # every null before any alignment
    assert call(d, grads(), radio(W=fake() + 4)) == ALIGN
    assert call(d, grads(), radio(dW=fake() + 4)) == ALIGN
    assert call(d, grads(dW1=fake() + 4), radio()) == ALIGN
    assert call(d, grads(dbc=None), radio()) == ARG


# ---- standalone attention scorer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [0, 1])
def test_attn_net_contract(gated):
    fw, bw = lib().mmf_attn_net_forward, lib().mmf_attn_net_backward

    def query(d):
        d = d or desc(N=5000, H=1024)
        return lib().mmf_attn_net_workspace_bytes(d.N, d.H, d.D, d.gated)

    def fwd(d, x=True, ws=True, wsb=None, A=True):
        wsb = query(d) if wsb is None else wsb
        return fw(ref(d), fake() if x is True else x, fake() if ws is True else ws, wsb, fake() if A else None, None)

    def bwd(d, g, x=True, ws=True, wsb=None, gA=True):
        wsb = query(d) if wsb is None else wsb
        return bw(ref(d), fake() if x is True else x, fake() if ws is True else ws, wsb, fake() if gA else None,
                  ref(g), None)

    d = desc(N=5000, H=1024, D=256, gated=gated, W1=None, b1=None)    # the scorer reads no projection
    full = query(d)
    assert full > 0
    assert fwd(None) == ARG
    assert fwd(d, x=None) == ARG and fwd(d, ws=None) == ARG and fwd(d, A=False) == ARG
    assert fwd(desc(N=5000, H=1024, gated=gated, Wa=None)) == ARG
    assert fwd(desc(N=5000, H=1024, gated=gated, p_att=1.0)) == ARG
    assert fwd(desc(N=5000, H=1000, gated=gated), wsb=1 << 40) == SHAPE
    assert fwd(desc(N=5000, H=1024, D=48, gated=gated), wsb=1 << 40) == SHAPE
    assert fwd(d, x=fake() + 4) == ALIGN
    assert fwd(d, ws=fake() + 4) == ALIGN
    assert fwd(desc(N=5000, H=1024, gated=gated, Wa=fake() + 4)) == ALIGN
    assert fwd(d, wsb=full - 1) == WS
    assert bwd(None, grads()) == ARG
    assert bwd(d, None) == ARG
    assert bwd(d, grads(), gA=False) == ARG and bwd(d, grads(), x=None) == ARG and bwd(d, grads(), ws=None) == ARG
    for n in ("dWa", "dba", "dWc", "dbc"):
        assert bwd(d, grads(**{n: None})) == ARG, n
    assert bwd(d, grads(dW1=None, db1=None), wsb=full - 1) == WS     # no projection gradients
    if gated:
        assert bwd(d, grads(dWb=None)) == ARG
        assert bwd(d, grads(dWb=fake() + 4)) == ALIGN
    assert bwd(desc(N=5000, H=1000, gated=gated), grads(), wsb=1 << 40) == SHAPE
    assert bwd(d, grads(dWa=fake() + 4)) == ALIGN
    assert bwd(d, grads(dx=fake() + 4)) == ALIGN
    assert bwd(d, grads(dx=fake()), wsb=full - 1) == WS
    assert bwd(d, grads(), wsb=full - 1) == WS


# ---- linear backward ------------------------------------------------------------------------------------------------
def test_linear_backward_contract():
    f = lib().mmf_linear_backward
    M, N, kseg = 50000, 512, 1024

    def call(nseg=1, xs=None, dy=True, dW=True, dx=None, W=True, n=N, k=kseg, wsb=None, ws=True):
        xs = xs if xs is not None else [fake() for _ in range(nseg)]
        arr = (C.c_void_p * len(xs))(*xs)
        wsb = lib().mmf_linear_backward_workspace_bytes(M, n, nseg * k) if wsb is None else wsb
        return f(fake() if dy else None, arr, nseg, k, M, fake() if W else None, n, fake() if dW else None, fake(), dx,
                 fake() if ws else None, wsb, None)

    for nseg in (1, 2, 4):
        full = lib().mmf_linear_backward_workspace_bytes(M, N, nseg * kseg)
        assert full > 256                                  # split-K: the slabs live in the workspace
        assert call(nseg, wsb=full - 1) == WS
        assert call(nseg, ws=False) == WS
    assert call(dy=False) == ARG
    assert call(dW=False) == ARG
    assert f(fake(), None, 1, kseg, M, fake(), N, fake(), fake(), None, fake(), 1 << 40, None) == ARG
    assert call(nseg=0, xs=[fake()]) == ARG and call(nseg=5, xs=[fake()] * 5) == ARG
    assert call(nseg=2, dx=fake()) == ARG
    assert call(dx=fake(), W=False) == ARG
    assert call(n=510, wsb=1 << 40) == SHAPE
    assert call(k=1022, wsb=1 << 40) == SHAPE
    assert call(nseg=2, xs=[fake(), None]) == ARG
    assert call(nseg=2, xs=[fake(), None], wsb=0) == WS               # the workspace before the segments


# ---- grouped forward-only passes ------------------------------------------------------------------------------------
def infer_target():
    return target(dWk=None, dbk=None)              # forward-only: no classifier gradients


@pytest.mark.parametrize("x_bf16", [0, 1])
@pytest.mark.parametrize("gated", [0, 1])
def test_infer_group_contract(x_bf16, gated):
    f = lib().mmf_amil_infer_group

    def query(d, offs=OFFS, bf16=x_bf16):
        d = d or desc(N=3000, L=2048)
        return lib().mmf_amil_group_infer_workspace_bytes((C.c_int64 * len(offs))(*offs), len(offs) - 1, d.L, d.H, d.D,
                                                          d.gated, bf16)

    def call(d, grp=True, h=True, t=True, x=True, ws=True, wsb=None, M=True, A=True):
        wsb = query(d) if wsb is None else wsb
        grp = group(OFFS, seeds=False) if grp is True else grp
        h = head() if h is True else h
        t = infer_target() if t is True else t
        return f(ref(d), ref(grp), fake() if x is True else x, x_bf16, fake() if ws is True else ws, wsb, ref(h), ref(t),
                 fake() if M else None, fake() if A else None, None)

    mk = lambda **kw: desc(**{**dict(N=3000, L=2048, gated=gated), **kw})
    d = mk()
    full = query(d)
    assert full > 0
    # A bf16 window's query is the larger of its own carve and the fp32 one (one buffer serves either storage).  Where the
    # bf16 carve is the larger (this gated shape), one byte less is refused; where it is not, query - 1 bytes would pass
    # every check and launch, so the cases below that must get as far as the workspace check pass no bytes at all.
    short = full - 1 if not x_bf16 or full > query(d, bf16=0) else 0
    assert short or not gated
    assert call(None) == ARG
    assert call(d, grp=None) == ARG
    assert call(d, x=None) == ARG
    assert call(d, ws=None) == ARG
    assert call(d, A=False) == ARG
    # the head, the target and M are optional, but a loss needs the head and a call without a head exists for M
    assert call(d, t=None, wsb=short) == WS
    assert call(d, M=False, wsb=short) == WS
    assert call(d, h=None, t=None, wsb=short) == WS
    assert call(d, h=None, t=None, M=False) == ARG
    assert call(d, h=None) == ARG
    assert call(d, h=None, M=False) == ARG
    assert call(d, grp=group(OFFS), wsb=short) == WS                 # seeds are not read
    # refused before the offset table and the descriptor are checked: dropout, bf16x3
    assert call(mk(p_h=0.25)) == ARG
    assert call(mk(p_att=0.25)) == ARG
    assert call(mk(gemm=BF16X3)) == ARG
    assert call(mk(H=384, p_h=0.25), wsb=1 << 40) == ARG
    assert call(mk(H=384, gemm=BF16X3), grp=group([5, 1000, 3000], seeds=False), wsb=1 << 40) == ARG
    # the offset table, then the descriptor, then the head
    assert call(d, grp=group([0, 1000, 1000, 3000], seeds=False)) == SHAPE
    assert call(d, grp=group([5, 1000, 3000], seeds=False)) == SHAPE
    assert call(mk(N=2999)) == SHAPE
    assert call(mk(N=2999, W1=None)) == SHAPE
    assert call(mk(H=384), wsb=1 << 40) == SHAPE
    assert call(mk(W1=None)) == ARG
    assert call(mk(H=384, W1=None), wsb=1 << 40) == ARG
    assert call(d, h=head(K=33)) == SHAPE
    assert call(d, h=head(K=0)) == SHAPE
    assert call(mk(H=384), h=head(K=33), wsb=1 << 40) == SHAPE
    assert call(mk(W1=None), h=head(K=33)) == ARG
    hd = head()
    hd.hazards = None
    assert call(d, h=hd) == ARG
    assert call(d, h=hd, x=fake() + 4) == ARG
    assert call(d, h=head(K=33), x=None) == SHAPE                          # the head before the call's pointers
    for n in ("Y", "c", "loss"):
        assert call(d, t=target(dWk=None, dbk=None, **{n: None})) == ARG, n
    assert call(d, t=target(), wsb=short) == WS                        # classifier gradient pointers are not read
    # a gated H = D = 256 stack takes the fused bf16 forward one bag at a time: its bf16 windows are refused
    small = mk(H=256, D=256)
    assert call(small, wsb=0) == (SHAPE if x_bf16 and gated else WS)
    assert call(small, h=head(K=33)) == SHAPE
    assert call(small, h=None, M=False) == (SHAPE if x_bf16 and gated else ARG)   # the stack before the head
    assert call(mk(L=1056), wsb=0) == (SHAPE if x_bf16 else WS)          # bf16: L % 64; fp32 takes L % 32
    assert call(d, x=fake() + 4) == ALIGN
    assert call(d, ws=fake() + 8) == ALIGN
    assert call(d, x=fake() + 4, ws=None) == ARG                           # null before alignment
    assert call(mk(W1=fake() + 4), wsb=short) == (WS if x_bf16 else ALIGN)   # bf16 converts the weights: any alignment
    assert call(mk(Wa=fake() + 4), wsb=short) == (WS if x_bf16 else ALIGN)
    if gated:
        assert call(mk(Wb=fake() + 4), wsb=short) == (WS if x_bf16 else ALIGN)
        assert call(mk(Wb=None)) == ARG
    assert call(d, wsb=short) == WS
    assert call(d, x=fake() + 4, wsb=short) == ALIGN                    # alignment before the workspace
    assert call(d, A=False, wsb=short) == ARG


def test_radio_infer_group_contract():
    from multimodalfusion_amd import _lib
    f = lib().mmf_radio_infer_group
    L = 1024

    def radio(nseg=4, kseg=L, xs=None, **kw):
        xs = xs if xs is not None else [fake() for _ in range(nseg)]
        arr = (C.c_void_p * len(xs))(*xs)
        r = _lib.RadioReduce(x=C.cast(arr, C.POINTER(C.c_void_p)), nseg=nseg, kseg=kseg, W=fake(), bias=fake(),
                             dW=None, db=None)
        for k, v in kw.items():
            setattr(r, k, v)
        r._keep = arr
        return r

    def query(d, nseg=4, offs=OFFS):
        d = d or desc(N=3000, L=L)
        return lib().mmf_radio_group_infer_workspace_bytes((C.c_int64 * len(offs))(*offs), len(offs) - 1, nseg, L, d.H,
                                                           d.D, d.gated)

    def call(d, rd, grp=True, h=True, t=True, ws=True, wsb=None, M=True, A=True):
        wsb = query(d, rd.nseg if rd is not None and 2 <= rd.nseg <= 4 else 4) if wsb is None else wsb
        grp = group(OFFS, seeds=False) if grp is True else grp
        h = head() if h is True else h
        t = infer_target() if t is True else t
        return f(ref(d), ref(grp), ref(rd), fake() if ws is True else ws, wsb, ref(h), ref(t), fake() if M else None,
                 fake() if A else None, None)

    d = desc(N=3000, L=L)
    for nseg in (2, 3, 4):
        full = query(d, nseg)
        assert full > 0
        assert call(d, radio(nseg), wsb=full - 1) == WS
        assert call(d, radio(nseg), h=None, t=None, wsb=full - 1) == WS
        assert call(d, radio(nseg, xs=[fake() + 4] + [fake()] * (nseg - 1)), wsb=full - 1) == ALIGN
        assert call(d, radio(nseg, xs=[fake()] * (nseg - 1) + [fake() + 4]), wsb=full - 1) == ALIGN
    assert call(d, None) == ARG
    r = radio()
    r.x = None
    assert call(d, r) == ARG
    assert call(None, radio()) == ARG
    assert call(d, radio(), grp=None) == ARG
    assert call(d, radio(nseg=1, xs=[fake()] * 4), wsb=1 << 40) == SHAPE
    assert call(d, radio(nseg=5, xs=[fake()] * 5), wsb=1 << 40) == SHAPE
    assert call(None, radio(nseg=5, xs=[fake()] * 5), wsb=1 << 40) == SHAPE      # the modality count before the descriptor
    assert call(desc(N=3000, L=L, p_h=0.25), radio(nseg=5, xs=[fake()] * 5), wsb=1 << 40) == SHAPE
    assert call(desc(N=3000, L=L, p_h=0.25), radio()) == ARG
    assert call(desc(N=3000, L=L, p_att=0.25), radio()) == ARG
    assert call(desc(N=3000, L=L, gemm=BF16X3), radio()) == ARG
    assert call(desc(N=3000, L=L, H=384), radio(), wsb=1 << 40) == SHAPE
    assert call(desc(N=2999, L=L), radio()) == SHAPE
    assert call(d, radio(), h=None, M=False) == ARG
    assert call(d, radio(), h=None) == ARG                                        # a target without a head
    assert call(d, radio(), h=head(K=33)) == SHAPE
    assert call(d, radio(), ws=None) == ARG
    assert call(d, radio(), A=False) == ARG
    assert call(d, radio(), ws=fake() + 8) == ALIGN
    assert call(desc(N=3000, L=L, W1=fake() + 4), radio()) == ALIGN
    assert call(d, radio(xs=[None, fake(), fake(), fake()])) == ARG               # the stack's input is x[0]
    assert call(d, radio(xs=[fake() + 4, fake(), fake(), fake()])) == ALIGN
    assert call(d, radio(xs=[fake() + 4, fake(), fake(), fake()], kseg=512)) == ALIGN   # ... checked before kseg
    assert call(d, radio(kseg=512)) == SHAPE
    assert call(d, radio(kseg=512, W=None)) == SHAPE
    big = desc(N=140000, L=L)
    big_offs = [0, 70000, 140000]
    assert call(big, radio(), grp=group(big_offs, seeds=False), wsb=1 << 40) == SHAPE    # [sum N x 4 L] >= 2 GiB
    for n in ("W", "bias"):
        assert call(d, radio(**{n: None})) == ARG, n
    assert call(d, radio(dW=fake(), db=fake()), wsb=query(d) - 1) == WS          # reduce_dim's gradient pointers are not read
    assert call(d, radio(xs=[fake(), fake(), None, fake()])) == ARG
    assert call(d, radio(xs=[fake(), fake(), fake() + 4, fake()])) == ALIGN
    assert call(d, radio(xs=[fake(), fake(), fake() + 4, None])) == ARG           # every null before any alignment
    assert call(d, radio(W=fake() + 4)) == ALIGN
    assert call(d, radio(W=fake() + 4, xs=[fake(), None, fake(), fake()])) == ARG
    assert call(d, radio(W=fake() + 4), wsb=query(d) - 1) == ALIGN               # alignment before the workspace
