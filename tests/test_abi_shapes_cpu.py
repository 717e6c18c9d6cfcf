"""CPU: the admitted envelope of the scorer, the dense layer, the stack and the tensor-fusion tail (tests/abi_shapes.py) --
the restated rules against the library where it refuses before any HIP call, the restated planners against the library's,
and the case tables of tests/test_gpu_abi_shapes.py and tests/test_gpu_xfusion_shapes.py against the shape classes the
rules make reachable; for the fusion tail also the two workspace queries over a grid on both sides of every limit, and the
fp64 oracle of every case clear of every ReLU kink under the seed the case records."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import abi_shapes as ab
import launch_plans as lp

# pointer values for calls that must return before any pointer is read: 16-byte aligned, never dereferenced
P = [0x10000 + 0x1000 * i for i in range(16)]


# ---- the tables cover the classes, and no case is idle -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ab.TABLES))
def test_every_class_has_a_case(name):
    missing = ab.uncovered(name)
    assert not missing, f"{name}: no case of tests/abi_shapes.py exercises {sorted(missing, key=str)}"


@pytest.mark.parametrize("name", sorted(ab.TABLES))
def test_every_case_is_the_only_one_for_some_class(name):
    """Dropping any one case leaves a class uncovered (and test_every_class_has_a_case then names it): a case that is not
    the only one for anything either duplicates another or exercises something REQUIRED does not list yet."""
    table, tags, required = ab.TABLES[name]
    for i, c in enumerate(table):
        lost = ab.uncovered(name, table[:i] + table[i + 1:])
        assert lost, f"{name}: {c} covers no required class of its own"
        assert lost <= tags(c)


def test_cases_say_what_they_are_for_and_classes_are_real():
    for name, (table, tags, required) in ab.TABLES.items():
        have = set()
        for c in table:
            assert c.why, (name, c)
            have |= tags(c)
        assert len(set(table)) == len(table), name
        assert required <= have


def test_the_issue_shapes_are_in_the_tables():
    """The values the GPU file is asked to run, read off the tables (not off REQUIRED)."""
    fwd = ab.accepted(ab.LINEAR_FORWARD, ab.linear_forward_rule)
    one = [c for c in fwd if c.nseg == 1 and not c.ws]
    assert {32, 96, 128, 160} <= {c.K for c in one}
    assert {4, 36, 64, 100, 260} <= {c.N for c in fwd} and {1, 63, 64, 65, 130} <= {c.M for c in fwd}
    assert {(c.nseg, c.kseg) for c in fwd if c.nseg > 1} >= {(2, 32), (3, 96), (4, 128)}
    assert {c.act for c in fwd if c.N % 64} == {0, 1, 2, 3, 4}
    assert {c.N for c in fwd if c.drop_p == 0.25} >= {36, 100}
    assert {(c.M, c.N, c.K) for c in fwd if c.ws} == {(65, 100, 512), (130, 36, 768), (64, 100, 1024)}
    assert {c.N for c in ab.refused(ab.LINEAR_FORWARD, ab.linear_forward_rule) if c.N % 4} == {1, 6, 30}
    bwd = ab.accepted(ab.LINEAR_BACKWARD, ab.linear_backward_rule)
    assert {c.N for c in bwd if not c.dx} >= {4, 36, 100, 256} and {c.kseg for c in bwd if not c.dx} >= {4, 36, 100, 1024}
    assert {c.M for c in bwd} >= {1, 3, 5, 64, 65, 1000} and {c.nseg for c in bwd} == {1, 2, 3, 4}
    assert {c.N for c in bwd if c.dx} >= {32, 96, 256} and {c.kseg for c in bwd if c.dx} >= {36, 100}
    att = ab.accepted(ab.ATTN, ab.attn_rule)
    assert {c.H for c in att} >= {32, 96, 128, 160} and {c.D for c in att} >= {32, 96, 160, 256}
    assert {c.N for c in att} >= {1, 63, 65, 777} and {c.gated for c in att} == {True, False}
    assert [c.size + (c.gated,) for c in ab.accepted(ab.STACK_F32, ab.stack_rule)] == [
        (32, 256, 128, False), (96, 256, 128, True), (160, 512, 640, True), (32, 1024, 384, False), (128, 1024, 128, True)]
    assert [c.size + (c.gated,) for c in ab.accepted(ab.STACK_BF16, ab.stack_rule)] == [
        (64, 256, 128, True), (192, 256, 256, True), (128, 256, 256, True), (64, 512, 384, False)]
    assert ab.STACK_BAGS == (1, 65, 300) and ab.BF16_BAGS == (65, 300)
    assert ab.GROUPED == [("mmf_amil_nll_step_group", (1, 65, 300), (96, 256, 128), False),
                          ("mmf_amil_infer_group", (1, 65, 300), (96, 256, 128), False),
                          ("mmf_amil_nll_step_group", (1, 65, 300), (160, 512, 640), True)]
    for _, _, size, gated in ab.GROUPED:        # admitted stack widths, every one
        assert ab.stack_rule(ab.Stack(*size, gated)) == ab.OK


# ---- the restated planners against the library's -----------------------------------------------------------------------
def test_ksplit_and_tn_split_restatements_match_the_library():
    b = lp.bound()
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    for M in (1, 63, 64, 65, 130, 512, 1000, 5000):
        for N in (4, 36, 64, 100, 256, 260, 1024):
            for nseg, kseg in ((1, 32), (1, 96), (1, 128), (1, 256), (1, 512), (1, 768), (1, 1024), (2, 32), (3, 96), (4, 128),
                               (2, 512), (4, 1024)):
                S = ab.linear_ksplit(M, N, nseg * kseg, nseg, kseg)
                assert S == b["linear_ksplit"](M, N, nseg * kseg, nseg, kseg), (M, N, nseg, kseg)
                want = S * ((M + 63) // 64) * ((N + 63) // 64) * 64 * 64 * 4 if S > 1 else 0
                assert l.mmf_linear_forward_workspace_bytes(M, N, nseg, kseg) == want
    for c in ab.accepted(ab.LINEAR_FORWARD, ab.linear_forward_rule):
        if c.ws:       # what the issue states for its K-split shapes
            assert ab.linear_ksplit(c.M, c.N, c.K, 1, c.K) == (4 if c.K == 1024 else 2), c
    for M in (1, 3, 5, 64, 65, 129, 1000, 12288):
        for N, K in ((4, 4), (36, 72), (100, 300), (256, 4096), (36, 100)):
            td = int(b["tn_tile_dim"](M, 0))
            tiles = ((N + td - 1) // td) * ((K + td - 1) // td)
            assert ab.linear_bwd_splits(M, N, K) == b["tn_splits"](M, tiles, td), (M, N, K)
            one = ab.linear_bwd_splits(M, N, K) == 1
            assert (l.mmf_linear_backward_workspace_bytes(M, N, K) == 256) == one
    split = [c for c in ab.accepted(ab.LINEAR_BACKWARD, ab.linear_backward_rule) if ab.linear_bwd_splits(c.M, c.N, c.K) > 1]
    assert split and all(l.mmf_linear_backward_workspace_bytes(c.M, c.N, c.K) > 256 for c in split)


# ---- the rules against the library, where it answers before any HIP call or pointer read ----------------------------------
def _lib():
    from multimodalfusion_amd import _lib as m
    return m, m.lib()


@pytest.mark.parametrize("c", ab.refused(ab.LINEAR_FORWARD, ab.linear_forward_rule), ids=lambda c: c.why)
def test_linear_forward_refusals_in_the_library(c):
    m, l = _lib()
    segs = (C.c_void_p * max(c.nseg, 1))(*P[:max(c.nseg, 1)])
    y = P[8] + (4 if c.misalign == "y" else 0)
    bias = P[9] + (4 if c.misalign == "bias" else 0)
    rc = l.mmf_linear_forward(segs, c.nseg, c.kseg, c.M, P[7], bias, c.N, c.act, C.c_float(c.drop_p), 0, 0, None, y,
                              None, 0, None, 0, None)
    assert rc == ab.linear_forward_rule(c), c
    assert rc in (ab.ERR_ARG, ab.ERR_SHAPE, ab.ERR_ALIGN)


@pytest.mark.parametrize("c", ab.refused(ab.LINEAR_BACKWARD, ab.linear_backward_rule), ids=lambda c: c.why)
def test_linear_backward_refusals_in_the_library(c):
    m, l = _lib()
    segs = (C.c_void_p * c.nseg)(*P[:c.nseg])
    rc = l.mmf_linear_backward(P[5], segs, c.nseg, c.kseg, c.M, P[6], c.N, P[7], P[8] if c.db else None,
                               P[9] if c.dx else None, None, 0, None)
    assert rc == ab.linear_backward_rule(c), c


def _desc(m, c, N=5, H=None):
    return m.AmilDesc(N=N, L=getattr(c, "L", c.H), H=c.H, D=c.D, gated=1 if c.gated else 0, W1=P[0], b1=P[1], Wa=P[2], ba=P[3],
                      Wb=P[4], bb=P[5], Wc=P[6], bc=P[7], p_h=0.0, p_att=0.0, seed=0, seed_dev=None, trace=None, concurrent=0,
                      gemm=0, sync=None, sync_words=0)


@pytest.mark.parametrize("c", ab.refused(ab.ATTN, ab.attn_rule), ids=lambda c: c.why)
def test_attn_net_refusals_in_the_library(c):
    m, l = _lib()
    d = _desc(m, c, N=c.N)
    assert l.mmf_attn_net_forward(C.byref(d), P[8], P[9], 1 << 20, P[10], None) == ab.attn_rule(c)
    g = m.AmilGrads(dW1=None, db1=None, dWa=P[11], dba=P[12], dWb=P[13], dbb=P[14], dWc=P[15], dbc=P[15] + 64, dx=None)
    assert l.mmf_attn_net_backward(C.byref(d), P[8], P[9], 1 << 20, P[10], C.byref(g), None) == ab.attn_rule(c)


@pytest.mark.parametrize("c", ab.refused(ab.STACK_F32, ab.stack_rule) + ab.refused(ab.STACK_BF16, ab.stack_rule),
                         ids=lambda c: c.why)
def test_stack_refusals_in_the_library(c):
    m, l = _lib()
    d = _desc(m, c)
    fwd, infer = (l.mmf_amil_bf16_forward, l.mmf_amil_bf16_infer) if c.bf16 else (l.mmf_amil_forward, l.mmf_amil_infer)
    for f in (fwd, infer):
        assert f(C.byref(d), P[8], P[9], 1 << 30, P[10], P[11], None) == ab.stack_rule(c) == ab.ERR_SHAPE
    if c.bf16:     # the same widths are admitted in fp32 storage: the refusal is the bf16 rule's
        assert ab.stack_rule(dataclasses.replace(c, bf16=False)) == ab.OK


def test_rules_admit_every_accepted_case_and_the_shipped_models():
    for table, rule in ((ab.LINEAR_FORWARD, ab.linear_forward_rule), (ab.LINEAR_BACKWARD, ab.linear_backward_rule),
                        (ab.ATTN, ab.attn_rule), (ab.STACK_F32, ab.stack_rule), (ab.STACK_BF16, ab.stack_rule)):
        assert ab.accepted(table, rule) and ab.refused(table, rule)
    for L, H, D in ((1024, 256, 256), (1024, 512, 384)):
        for bf16 in (False, True):
            assert ab.stack_rule(ab.Stack(L, H, D, True, bf16)) == ab.OK
        assert ab.attn_rule(ab.Attn(1000, H, D, True)) == ab.OK
    assert ab.linear_forward_rule(ab.LinFwd(512, 1024, 4, 1024)) == ab.OK
    assert ab.linear_backward_rule(ab.LinBwd(512, 1024, 4, 1024)) == ab.OK


def test_strerror_and_header_state_the_dense_layer_rule():
    import os
    from conftest import ROOT
    m, l = _lib()
    assert b"N % 4" in l.mmf_strerror(ab.ERR_SHAPE)
    hdr = open(os.path.join(ROOT, "include", "mmf_amil.h")).read()
    dense = hdr[hdr.index("Dense layer on MFMA"):hdr.index("mmf_linear_backward_workspace_bytes")]
    assert "N % 4 == 0" in dense and "MMF_ERR_SHAPE" in dense and "MMF_ERR_ALIGN" in dense and "bias" in dense


# ---- the tensor-fusion tail: the rules against both workspace queries and the entry points ---------------------------------
XF_GRID = dict(m=(1, 2, 3, 4), sdim=(8, 16, 17), dim=(0, 4, 6, 8, 252, 256, 260, 768), mmhid1=(0, 1, 4, 5, 512, 516, 1528, 1532, 1536, 1537),
               mmhid2=(0, 1, 6, 1536, 1537), nhid=(0, 1, 7, 1536, 1537), G=(0, 1, 3, 17, 64, 65))


def _xf_grid():
    import itertools
    for m, sdim, dim, mmhid1, mmhid2, nhid, G in itertools.product(*(XF_GRID[k] for k in ("m", "sdim", "dim", "mmhid1", "mmhid2", "nhid", "G"))):
        yield ab.XFusion(m, dim, mmhid1, mmhid2, nhid, G, sdim=sdim)


def test_xfusion_grid_straddles_every_limit():
    got = {"infer": set(), "train": set()}
    K2 = set()
    for c in _xf_grid():
        got["infer"].add(ab.xfusion_infer_rule(c))
        got["train"].add(ab.xfusion_train_rule(c))
        if ab.xfusion_infer_rule(dataclasses.replace(c, dim=4, mmhid1=4)) == ab.OK:
            K2.add(c.K2)
    assert got == {"infer": {ab.OK, ab.ERR_SHAPE}, "train": {ab.OK, ab.ERR_SHAPE}}
    assert {1536, 1540} <= K2 and any(k > 1536 and k - 1536 < 8 for k in K2)        # the cap from both sides
    trains = [c for c in _xf_grid() if ab.xfusion_train_rule(c) == ab.OK]
    only_infer = [c for c in _xf_grid() if ab.xfusion_infer_rule(c) == ab.OK and ab.xfusion_train_rule(c) != ab.OK]
    assert len(trains) > 500 and {c.mmhid1 % 4 != 0 or c.nhid > 1536 for c in only_infer} == {True}
    assert any(c.mmhid1 % 4 for c in only_infer) and any(c.nhid > 1536 for c in only_infer)


def test_xfusion_workspace_queries_answer_zero_exactly_where_the_rules_refuse():
    """mmf_xfusion_group_workspace_bytes against xfusion_train_rule at every grid point; the forward-only query sees only
    (m, sdim, mmhid1, G): against xfusion_window_ok.  Where they accept: at least the buffers the header names."""
    m_, l = _lib()
    qt, qi = l.mmf_xfusion_group_workspace_bytes, l.mmf_xfusion_group_infer_workspace_bytes
    n_ok = 0
    for c in _xf_grid():
        got = qt(c.m, c.dim, c.sdim, c.mmhid1, c.mmhid2, c.nhid, c.G)
        if ab.xfusion_train_rule(c) != ab.OK:
            assert got == 0, c
            continue
        n_ok += 1
        gate, bits = c.G * c.m * 16, c.G * ((c.E + 63) // 64 * 2)
        # o, h, z, gm, dpo, dz, dph; the keep bits; d of the product; dMM; with accumulate the dense backward's fresh dW and
        # db of classifier[0] and of encoder2, one after the other, go through the workspace: the larger of each
        named = 7 * gate + bits + c.G * c.E + c.G * c.mmhid2 + max(c.mmhid2 * c.K2, c.nhid * c.mmhid2) + max(c.mmhid2, c.nhid)
        assert got >= 4 * named, (c, got, 4 * named)
    assert n_ok > 500
    for m in XF_GRID["m"]:
        for sdim in XF_GRID["sdim"]:
            for mmhid1 in XF_GRID["mmhid1"]:
                for G in XF_GRID["G"]:
                    got = qi(m, sdim, mmhid1, G)
                    if not ab.xfusion_window_ok(m, sdim, mmhid1, G):
                        assert got == 0, (m, sdim, mmhid1, G)
                    else:
                        assert got >= 4 * (G * m * 16 + G * mmhid1), (m, sdim, mmhid1, G)      # o and encoder1's output


def _xf_calls(l, c, nbytes):
    """The three entry points on never-dereferenced pointers: a refused shape returns its code before any pointer is read,
    an admitted one goes on to the workspace check (nbytes = 0: MMF_ERR_WORKSPACE, still before any launch)."""
    from test_mm_infer_group_abi_cpu import _weights
    fake = P[0]
    w = _weights(fake, m=c.m, dim=c.dim, sdim=c.sdim, mmhid1=c.mmhid1, mmhid2=c.mmhid2, nhid=c.nhid)
    v = (C.c_void_p * 3)(fake, fake, fake)
    from multimodalfusion_amd import _lib as m_
    g = m_.XFusionGrads(dWe1=fake, dbe1=fake, dWe2=fake, dbe2=fake, dWc0=fake, dbc0=fake)
    for n in ("dWh", "dbh", "dWz", "dbz", "dWo", "dbo"):
        for i in range(3):
            getattr(g, n)[i] = fake
    infer = l.mmf_xfusion_infer_group(C.byref(w), v, c.G, fake, nbytes, fake, fake, None)
    fwd = l.mmf_xfusion_group_forward(C.byref(w), fake, c.G, C.c_float(0.25), C.c_float(0.25), fake, None, fake, nbytes, fake,
                                      fake, None)
    bwd = l.mmf_xfusion_group_backward(C.byref(w), fake, c.G, C.c_float(0.25), C.c_float(0.25), fake, None, fake, fake, fake,
                                       c.lddhid, fake, nbytes, fake, C.byref(g), 0, None)
    return infer, fwd, bwd


def test_xfusion_entry_points_follow_the_rules_before_any_launch():
    """Every case of the table and a thinned grid: a refusal is MMF_ERR_SHAPE, an admitted shape reaches the workspace
    check.  The forward has no dhid: lddhid is the backward's alone."""
    m_, l = _lib()
    cases = list(ab.XFUSION) + [c for i, c in enumerate(_xf_grid()) if i % 37 == 0]
    cases += [dataclasses.replace(c, lddhid_pad=p) for c in ab.accepted(ab.XFUSION, ab.xfusion_train_rule)[:3] for p in (-1, 0, 5)]
    for c in cases:
        infer, fwd, bwd = _xf_calls(l, c, 0)
        want = lambda code: ab.ERR_WORKSPACE if code == ab.OK else code
        assert infer == want(ab.xfusion_infer_rule(c)), c
        assert fwd == want(ab.xfusion_train_rule(dataclasses.replace(c, lddhid_pad=0))), c
        assert bwd == want(ab.xfusion_train_rule(c)), c


def test_xfusion_table_is_what_the_issue_asks_for():
    acc_t, acc_i = ab.accepted(ab.XFUSION, ab.xfusion_train_rule), ab.accepted(ab.XFUSION, ab.xfusion_infer_rule)
    assert set(acc_t) <= set(acc_i) and 10 <= len(acc_i) <= 14
    assert {c.dim for c in acc_t} >= {4, 256, 260} and any(8 <= c.dim <= 252 for c in acc_t)
    assert {c.mmhid1 for c in acc_t} >= {512, 516, 1528} and any(c.mmhid1 < 32 for c in acc_t)
    assert any(c.mmhid1 % 4 for c in acc_i) and not any(c.mmhid1 % 4 for c in acc_t)
    assert {c.K2 for c in acc_t} >= {12, 1536} and {c.mmhid2 for c in acc_t} >= {1, 1536} and {c.nhid for c in acc_t} >= {1, 1536}
    assert {c.G for c in acc_t} >= {1, 17, 64} and {2, 3} & {c.G for c in acc_t}
    assert all(c.G <= 17 for c in acc_i if not (c.G == 64 and c.K2 <= 64 and c.mmhid2 <= 64 and c.nhid <= 64))
    assert all(c.mmhid1 <= 516 for c in acc_i if c.m == 3)
    for c in acc_t:          # what the header says of x2 and dhid
        assert c.K2 % 4 == 0 and c.lddhid >= c.nhid
    whys = {c.why.split(":")[0] for c in ab.XFUSION if ab.xfusion_infer_rule(c) != ab.OK or ab.xfusion_train_rule(c) != ab.OK}
    assert {"dim % 4", "K2 = 1540", "mmhid2 = 1537", "G = 0", "G = 65", "m = 1", "m = 4", "sdim = 8", "lddhid < nhid",
            "mmhid1 % 4 != 0", "nhid = 1537"} <= whys


def test_xfusion_oracles_keep_clear_of_every_relu_kink():
    """Under the seed each case records, no ReLU pre-activation of the fusion tail, of any patient, in train or eval mode,
    lies within KINK of zero in the fp64 oracle: fp32 and fp64 take the same side of every ReLU, and the GPU file excuses no
    unit; and no case is dead behind a ReLU or a mask.  Also: the shipped shape is admitted by both rules."""
    import xfusion_cases as xc
    for c in ab.accepted(ab.XFUSION, ab.xfusion_infer_rule):
        for train in ((True, False) if ab.xfusion_train_rule(c) == ab.OK else (False,)):
            MM, hid, dv, gw, margin = xc.oracle(c, train)
            assert margin > 2 * xc.KINK, (c, train, margin)
            # and the case checks something: every patient has a live unit in MM and in hid, no gradient is all zero
            assert (np.abs(MM).max(1) > 0).all() and (np.abs(hid).max(1) > 0).all(), (c, train)
            assert all(np.abs(v).max() > 0 for v in dv) and all(np.abs(v).max() > 0 for v in gw.values()), (c, train)
    for m in (2, 3):
        assert ab.xfusion_train_rule(ab.XFusion(m, 256, 512, 512, 256, 64)) == ab.xfusion_infer_rule(ab.XFusion(m, 256, 512, 512, 256, 64)) == ab.OK
