"""CPU checks of the one-call stage-2 training step in the C ABI (include/mmf_amil.h: mmf_stage2_step_workspace_bytes,
mmf_stage2_step): the ctypes mirrors against the header compiled as C, both symbols bound with the header's arity, the ABI
version unchanged, every refusal in the header's order before any HIP call -- the fake pointers are never read -- and the
workspace query's zeros, formula and monotonicity.  Needs the built library, not a GPU."""
import ctypes as C
import re

from test_abi_layout_cpu import HEADER, _c_layout

FAKE = 0x7F0000001000
OK, ARG, SHAPE, ALIGN, WORKSPACE = 0, -1, -2, -3, -4
NLL, COX = 0, 1
EF, LF, EH, LH, KR = range(5)
L_NLL, L_COX, L_RANK, L_RANK_NLL = range(4)
NEW = ["mmf_stage2_step_workspace_bytes", "mmf_stage2_step"]
LAYERS = ("gate", "nl", "lin")


def test_mirrors_match_the_header_compiled_as_c(tmp_path):
    from multimodalfusion_amd import _lib
    mirrors = {"mmf_stage2_bn_train": _lib.Stage2BnTrain, "mmf_stage2_step_block": _lib.Stage2StepBlock,
               "mmf_stage2_step_desc": _lib.Stage2StepDesc, "mmf_stage2_target": _lib.Stage2Target,
               "mmf_stage2_block_grads": _lib.Stage2BlockGrads, "mmf_stage2_step_grads": _lib.Stage2StepGrads}
    got = _c_layout(tmp_path, {c: [n for n, _ in m._fields_] for c, m in mirrors.items()})
    for cname, m in mirrors.items():
        assert got[(cname, "sizeof")] == C.sizeof(m), cname
        for n, _ in m._fields_:
            assert got[(cname, n)] == getattr(m, n).offset, (cname, n)


def test_new_symbols_are_bound_with_the_headers_arity():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(l, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    for macro in ("MMF_STAGE2_LOSS_NLL 0", "MMF_STAGE2_LOSS_COX 1", "MMF_STAGE2_LOSS_RANK 2", "MMF_STAGE2_LOSS_RANK_NLL 3"):
        assert "#define " + macro in text
    assert l.mmf_abi_version() == _lib.ABI_VERSION == 12          # additive: the version stays


def _bn(**kw):
    from multimodalfusion_amd import _lib
    return _lib.Stage2BnTrain(**{n: kw.get(n, FAKE) for n in ("weight", "bias", "running_mean", "running_var")}, eps=1e-5,
                              momentum=0.1)


def _arr(keep, vals):
    a = (C.c_void_p * len(vals))(*vals)
    keep.append(a)
    return a


def _desc(keep, family=NLL, tt=EF, present=(1, 1, 1), n_layers=1, B=5, K=4, training=1, blk=None, **kw):
    """A descriptor of fake pointers; kw overrides a member (None: a null pointer); blk: {index: {member: value}}."""
    from multimodalfusion_amd import _lib
    d = _lib.Stage2StepDesc(family=family, train_type=tt, radio=present[0], path=present[1], omic=present[2],
                            n_layers=n_layers, B=B, K=K, training=training, Wk=FAKE, bk=FAKE, p_drop=0.7, seed=1)
    n = max(1, min(n_layers, 8))
    for i in range(3):
        d.h[i] = FAKE
        b = d.blk[i]
        b.W0, b.b0, b.W4, b.b4, b.bn, b.bn1, b.bn2 = FAKE, FAKE, FAKE, FAKE, _bn(), _bn(), _bn()
        for name in LAYERS:
            setattr(b, "W" + name, _arr(keep, [FAKE] * n))
            setattr(b, "b" + name, _arr(keep, [FAKE] * n))
        for name, v in (blk or {}).get(i, {}).items():
            if isinstance(v, list):
                v = _arr(keep, v)
            setattr(b, name, v if v is not None else (C.POINTER(C.c_void_p)() if name[1:] in LAYERS else None))
    for name, v in kw.items():
        if name.startswith("h") and name[1:].isdigit():
            d.h[int(name[1:])] = v
        else:
            setattr(d, name, v)
    return d


def _target(loss=L_NLL, **kw):
    from multimodalfusion_amd import _lib
    t = _lib.Stage2Target(loss=loss, Y=FAKE, c=FAKE, times=FAKE, alpha=0.15, nll_ratio=0.5, phi=0, reduction=0, loss_scale=1.0)
    for n, v in kw.items():
        setattr(t, n, v)
    return t


def _grads(keep, n_layers=1, blk=None, **kw):
    from multimodalfusion_amd import _lib
    g = _lib.Stage2StepGrads(dWk=FAKE, dbk=FAKE)
    n = max(1, min(n_layers, 8))
    for i in range(3):
        b = g.blk[i]
        for name in ("dW0", "db0", "dbn_weight", "dbn_bias", "dW4", "db4", "dbn1_weight", "dbn1_bias", "dbn2_weight", "dbn2_bias"):
            setattr(b, name, FAKE)
        for name in LAYERS:
            setattr(b, "dW" + name, _arr(keep, [FAKE] * n))
            setattr(b, "db" + name, _arr(keep, [FAKE] * n))
        for name, v in (blk or {}).get(i, {}).items():
            if isinstance(v, list):
                v = _arr(keep, v)
            setattr(b, name, v if v is not None else (C.POINTER(C.c_void_p)() if name[2:] in LAYERS else None))
    for name, v in kw.items():
        setattr(g, name, v)
    return g


def _call(ws=FAKE, nbytes=1 << 40, target=None, grads=True, gblk=None, gkw=None, outs=None, accumulate=0, no_desc=False,
          no_target=False, **kw):
    from multimodalfusion_amd import _lib
    keep = []
    d = _desc(keep, **kw)
    family = kw.get("family", NLL)
    t = _target(**(target if target is not None else dict(loss=L_COX if family == COX else L_NLL)))
    g = _grads(keep, kw.get("n_layers", 1), gblk, **(gkw or {})) if grads else None
    o = dict(risk=FAKE, hazards=FAKE, S=FAKE, loss=FAKE)
    o.update(outs or {})
    return _lib.lib().mmf_stage2_step(None if no_desc else C.byref(d), None if no_target else C.byref(t), ws, nbytes, o["risk"],
                                      o["hazards"], o["S"], o["loss"], None if g is None else C.byref(g), accumulate, None)


def test_refusals_in_the_headers_order_before_any_launch():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    types = [(f, t) for f in (NLL, COX) for t in (EF, LF, EH, LH)]
    for f, t in types:                                   # everything else in order: only the workspace is wrong
        K = 1 if f == COX else 4
        for grads in (True, False):
            assert _call(family=f, tt=t, K=K, nbytes=16, grads=grads) == WORKSPACE, (f, t)
        for present in ((1, 1, 0), (1, 0, 1), (0, 1, 1)):
            assert _call(family=f, tt=t, K=K, present=present, nbytes=16) == WORKSPACE, (f, t, present)
    # MMF_ERR_ARG
    assert _call(no_desc=True) == ARG and _call(no_target=True) == ARG
    for n in ("Wk", "bk"):
        assert _call(**{n: None}) == ARG, n
    for n in ("risk", "loss", "hazards", "S"):
        assert _call(outs={n: None}) == ARG, n
    assert _call(family=COX, K=1, outs=dict(hazards=None, S=None), nbytes=16) == WORKSPACE     # the cox family writes neither
    assert _call(target=dict(c=None)) == ARG
    for bad in (dict(family=-1), dict(family=2), dict(tt=-1), dict(tt=5)):
        assert _call(**bad) == ARG, bad
    for bad in (dict(loss=-1), dict(loss=4), dict(phi=2), dict(phi=-1), dict(reduction=2), dict(reduction=-1)):
        assert _call(target=bad) == ARG, bad
    assert _call(tt=KR) == ARG and _call(family=COX, K=1, tt=KR) == ARG                          # kronecker is not taken
    for loss in (L_NLL, L_RANK_NLL):                                                         # hazards are an nll-family output
        assert _call(family=COX, K=1, target=dict(loss=loss)) == ARG
    for loss in (L_COX, L_RANK):
        assert _call(family=COX, K=1, target=dict(loss=loss), nbytes=16) == WORKSPACE
    for loss in (L_NLL, L_COX, L_RANK, L_RANK_NLL):
        assert _call(target=dict(loss=loss), nbytes=16) == WORKSPACE
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert _call(p_drop=p) == ARG, p
    assert _call(p_drop=0.0, nbytes=16) == WORKSPACE
    assert _call(h0=None) == ARG and _call(h2=None) == ARG
    assert _call(tt=EF, present=(1, 1, 0), h2=None, nbytes=16) == WORKSPACE                 # an early type reads the present ones
    assert _call(tt=LF, present=(1, 1, 0), h2=None) == ARG                                  # a late type reads all three
    assert _call(tt=LH, present=(0, 1, 1), h0=None) == ARG
    assert _call(tt=EF, blk={0: dict(W0=None)}) == ARG and _call(tt=EF, blk={0: dict(bn=_bn(running_var=None))}) == ARG
    assert _call(tt=EF, blk={1: dict(W0=None)}, nbytes=16) == WORKSPACE                     # the early types read blk[0] alone
    assert _call(tt=LF, blk={2: dict(b0=None)}) == ARG and _call(tt=LF, blk={1: dict(W4=None)}, nbytes=16) == WORKSPACE
    assert _call(tt=LF, present=(1, 1, 0), blk={2: dict(W0=None)}) == ARG                   # the dropped block runs too
    assert _call(family=COX, K=1, tt=LF, blk={1: dict(W4=None)}) == ARG
    assert _call(tt=EH, blk={0: dict(bn2=_bn(running_mean=None))}) == ARG and _call(tt=LH, blk={2: dict(Wnl=None)}) == ARG
    assert _call(tt=LH, blk={1: dict(blin=[None])}) == ARG and _call(tt=EH, blk={0: dict(W0=None)}, nbytes=16) == WORKSPACE
    assert _call(tt=EH, n_layers=2, blk={0: dict(Wlin=[FAKE, None])}) == ARG                # a null entry of a per-layer array
    assert _call(target=dict(loss=L_NLL, Y=None)) == ARG and _call(target=dict(loss=L_RANK_NLL, Y=None)) == ARG
    assert _call(target=dict(loss=L_COX, times=None)) == ARG and _call(target=dict(loss=L_RANK, times=None)) == ARG
    assert _call(target=dict(loss=L_NLL, times=None), nbytes=16) == WORKSPACE
    assert _call(target=dict(loss=L_COX, Y=None), nbytes=16) == WORKSPACE
    # a null gradient of a parameter that takes part
    assert _call(gkw=dict(dWk=None)) == ARG and _call(gkw=dict(dbk=None)) == ARG
    assert _call(tt=EF, gblk={0: dict(dW0=None)}) == ARG and _call(tt=EF, gblk={0: dict(dbn_bias=None)}) == ARG
    assert _call(tt=EF, gblk={1: dict(dW0=None)}, nbytes=16) == WORKSPACE
    assert _call(tt=LF, gblk={2: dict(db0=None)}) == ARG
    assert _call(tt=LF, present=(1, 1, 0), gblk={2: dict(db0=None)}, nbytes=16) == WORKSPACE   # the dropped block gets none
    assert _call(tt=LH, present=(1, 0, 1), gblk={1: dict(dbn1_weight=None, dWgate=None)}, nbytes=16) == WORKSPACE
    assert _call(family=COX, K=1, tt=LF, gblk={0: dict(db4=None)}) == ARG
    assert _call(tt=LF, gblk={0: dict(db4=None)}, nbytes=16) == WORKSPACE
    assert _call(tt=EH, gblk={0: dict(dbn2_weight=None)}) == ARG and _call(tt=LH, gblk={2: dict(dblin=None)}) == ARG
    assert _call(tt=EH, n_layers=2, gblk={0: dict(dWnl=[FAKE, None])}) == ARG
    # MMF_ERR_ARG comes before every MMF_ERR_SHAPE
    assert _call(B=0, Wk=None) == ARG and _call(K=33, family=7) == ARG and _call(B=300, h1=None) == ARG
    # MMF_ERR_SHAPE
    for bad in (dict(present=(1, 0, 0)), dict(present=(0, 0, 0)), dict(B=0), dict(B=-3), dict(B=257), dict(B=1), dict(K=0),
                dict(K=33), dict(family=COX, K=4)):
        assert _call(**bad) == SHAPE, bad
    assert _call(B=1, training=0, nbytes=16) == WORKSPACE and _call(B=2, nbytes=16) == WORKSPACE
    assert _call(B=256, K=32, nbytes=16) == WORKSPACE and _call(K=1, nbytes=16) == WORKSPACE
    for t in (EH, LH):                                                         # a Highway's depth: 1 .. 8
        assert _call(tt=t, n_layers=0) == SHAPE and _call(tt=t, n_layers=9) == SHAPE
        assert _call(tt=t, n_layers=2, nbytes=16) == WORKSPACE and _call(tt=t, n_layers=8, nbytes=16) == WORKSPACE
    assert _call(tt=EF, n_layers=9, nbytes=16) == WORKSPACE                    # the fcnn types have no layers to count
    for loss in (L_RANK, L_RANK_NLL):                                          # a ranking loss needs a pair
        assert _call(B=1, training=0, target=dict(loss=loss)) == SHAPE
    assert _call(B=1, training=0, target=dict(loss=L_COX), nbytes=16) == WORKSPACE
    # a shape refusal comes before an alignment refusal
    assert _call(B=0, h0=FAKE + 4) == SHAPE
    # MMF_ERR_ALIGN
    assert _call(h1=FAKE + 4) == ALIGN and _call(ws=FAKE + 4) == ALIGN and _call(ws=None) == ARG
    assert _call(tt=EF, present=(1, 1, 0), h2=FAKE + 4, nbytes=16) == WORKSPACE
    assert _call(tt=LH, present=(1, 1, 0), h2=FAKE + 4) == ALIGN
    assert _call(tt=EH, blk={0: dict(Wgate=[FAKE + 4])}) == ALIGN and _call(tt=LH, blk={2: dict(Wlin=[FAKE + 8])}) == ALIGN
    assert _call(tt=EH, blk={0: dict(bgate=[FAKE + 4])}, nbytes=16) == WORKSPACE
    assert _call(target=dict(loss=L_COX, times=FAKE + 4)) == ALIGN
    assert _call(Wk=FAKE + 4, blk={0: dict(W0=FAKE + 4)}, nbytes=16) == WORKSPACE   # read one float at a time
    # an alignment refusal comes before the workspace's
    assert _call(h0=FAKE + 4, nbytes=16) == ALIGN
    for f, t in types:
        K = 1 if f == COX else 4
        need = l.mmf_stage2_step_workspace_bytes(f, t, 3, 1, 5, K, 1)
        assert need > 0 and _call(family=f, tt=t, K=K, nbytes=need - 1) == WORKSPACE


def test_workspace_query_zeros_formula_and_monotonicity():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_stage2_step_workspace_bytes
    ok = dict(family=NLL, tt=EF, m=3, n_layers=1, B=5, K=4, training=1)
    ask = lambda **kw: q(*{**ok, **kw}.values())
    assert ask() > 0
    for kw in (dict(family=2), dict(family=-1), dict(tt=4), dict(tt=5), dict(tt=-1), dict(m=1), dict(m=4), dict(B=0), dict(B=257),
               dict(B=1), dict(K=0), dict(K=33), dict(family=COX), dict(tt=EH, n_layers=0), dict(tt=EH, n_layers=9),
               dict(tt=LH, n_layers=100)):
        assert ask(**kw) == 0, kw
    assert ask(B=1, training=0) > 0 and ask(tt=EF, n_layers=0) > 0
    r256 = lambda n: (n + 255) // 256 * 256
    for B in (1, 2, 5, 33, 255, 256):
        ldB = (B + 3) // 4 * 4
        for m in (2, 3):
            for tt, nb, mw in ((EF, 1, 1), (LF, 3, m)):
                want = nb * r256(4 * 128 * ldB) + r256(4 * 128 * mw * ldB) + nb * r256(4 * 256) + r256(4 * 3 * B)
                assert ask(tt=tt, m=m, B=B, training=0) == want, (tt, m, B)
            for tt, nb, D in ((EH, 1, 256 * m), (LH, 3, 256)):
                for L in (1, 2, 8):
                    per = (L + 1) * r256(4 * D * ldB) + L * r256(4 * B * D) + (3 * L + 6) * r256(4 * D * ldB) + 2 * r256(4 * 2 * D)
                    assert ask(tt=tt, m=m, B=B, n_layers=L, training=0) == nb * per + r256(4 * 256 * m * ldB), (tt, m, B, L)
    for f in (NLL, COX):
        for tt, L in ((EF, 1), (LF, 1), (EH, 1), (LH, 1), (EH, 2), (LH, 8)):
            for m in (2, 3):
                K = 1 if f == COX else 32
                prev = 0
                for B in range(2, 257):
                    cur = ask(family=f, tt=tt, m=m, K=K, B=B, n_layers=L)
                    assert cur >= prev and cur > 0, (f, tt, m, B)
                    prev = cur
                assert ask(family=f, tt=tt, m=m, K=K, B=256, n_layers=L) > ask(family=f, tt=tt, m=m, K=K, B=2, n_layers=L)


def test_python_surface_says_no_before_the_library_is_called():
    import torch
    from multimodalfusion_amd.models import coxranking_models_pretrained as cm
    from multimodalfusion_amd.models import nll_models_pretrained as nm
    from multimodalfusion_amd.utils.loss_utils import CoxSurvLoss, NLLSurvLoss
    h = torch.zeros(3, 256)
    for mod in (nm, cm):
        model = mod.multimodal_pretrained(train_type="early-fcnn", mode="radio_path")
        assert model.step_ok(h, h, h, CoxSurvLoss()) is False                    # CPU tensors: there is no CPU path
        assert model.step_ok(h, h, h, object()) is False
    assert cm.multimodal_pretrained(train_type="late-fcnn").step_ok(h, h, h, NLLSurvLoss()) is False
    assert nm.multimodal_pretrained(train_type="kronecker", mode="radio_path").step_ok(h, h, h, NLLSurvLoss()) is False
    assert not hasattr(nm.unimonal_pretrained(train_type="fcnn", mode="path"), "step_ok")
