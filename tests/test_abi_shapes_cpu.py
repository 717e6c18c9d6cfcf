"""CPU: the admitted envelope of the scorer, the dense layer, the stack and the tensor-fusion tail (tests/abi_shapes.py) --
the restated rules against the library where it refuses before any HIP call, the restated planners against the library's,
and the case tables of tests/test_gpu_abi_shapes.py and tests/test_gpu_xfusion_shapes.py against the shape classes the
rules make reachable; for the fusion tail also the two workspace queries over a grid on both sides of every limit, and the
fp64 oracle of every case clear of every ReLU kink under the seed the case records; for the small ops (losses, hazard heads,
batch norm, the step tail, the dense backward) also the conditions their generated inputs must meet (tests/small_cases.py) and
the vectorised Cox and ranking restatements against the ports."""
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


# ---- the small ops: the rules against the library, and the conditions the GPU file's inputs must meet ----------------------
def _small(table, rule):
    return pytest.mark.parametrize("c", ab.refused(table, rule), ids=lambda c: c.why)


@_small(ab.HEAD, ab.head_rule)
def test_surv_head_refusals_in_the_library(c):
    m, l = _lib()
    assert l.mmf_surv_head_forward(P[0], P[1], P[2], c.B, c.F, c.K, P[3], P[4], P[5], P[6], None) == ab.head_rule(c)
    assert l.mmf_surv_head_backward(P[0], P[1], P[2], P[3], P[4], c.B, c.F, c.K, P[5], P[6], P[7], None) == ab.head_rule(c)


def test_small_loss_refusals_in_the_library():
    m, l = _lib()
    for c in ab.refused(ab.NLL, ab.nll_rule):
        assert l.mmf_nll_surv(P[0], P[1], P[2], P[3], c.B, c.K, C.c_float(0.4), C.c_float(1e-7), P[4], P[5], P[6], None) == ab.nll_rule(c)
    for c in ab.refused(ab.COX, ab.cox_rule):
        assert l.mmf_cox_surv(P[0], P[1], P[2], c.B, P[3], P[4], None) == ab.cox_rule(c) == ab.ERR_SHAPE
    for c in ab.refused(ab.RANK, ab.rank_rule):
        assert l.mmf_ranking_loss(P[0], P[1], P[2], c.B, c.phi, c.reduction, P[3], P[4], None) == ab.rank_rule(c) == ab.ERR_SHAPE
    for phi, red in ((2, 0), (0, 2), (-1, 0)):
        assert ab.rank_rule(ab.Rank(4, phi, red)) == l.mmf_ranking_loss(P[0], P[1], P[2], 4, phi, red, P[3], P[4], None) == ab.ERR_ARG
    for c in ab.refused(ab.HAZ, ab.haz_rule):
        assert l.mmf_hazards_forward(P[0], c.B, c.K, P[1], P[2], P[3], P[4], None) == ab.haz_rule(c) == ab.ERR_SHAPE
        assert l.mmf_hazards_backward(P[0], P[1], P[2], P[3], c.B, c.K, P[4], None) == ab.ERR_SHAPE
    for c in ab.refused(ab.HIGHWAY, ab.highway_rule):
        assert l.mmf_highway_mix_forward(P[0], P[1], P[2], c.n, P[3], None) == ab.highway_rule(c)
        assert l.mmf_highway_mix_backward(P[0], P[1], P[2], P[3], c.n, P[4], P[5], P[6], None) == ab.highway_rule(c)
    for c in ab.refused(ab.ABS_SUM, ab.abs_sum_rule):
        assert l.mmf_abs_sum(P[0], c.n, P[1], P[2], None) == ab.abs_sum_rule(c)


def test_batchnorm_adam_and_dense_backward_refusals_in_the_library():
    m, l = _lib()
    f = C.c_float
    for c in ab.refused(ab.BN, ab.bn_rule) + [ab.Bn(4, 8, training=False), ab.Bn(4, 8, act=5), ab.Bn(4, 8, drop_p=1.0)]:
        rm, rv = (P[4], P[5]) if c.running else (None, None)
        rc = l.mmf_batchnorm_forward(P[0], None, None, None, rm, rv, c.B, c.F, int(c.training), f(1e-5), f(0.1), c.act, f(c.drop_p),
                                     1, 1, None, P[1], P[2], P[3], None)
        assert rc == ab.bn_rule(c) != ab.OK, c
    for c in ab.refused(ab.ADAM, ab.adam_rule):
        rc = l.mmf_adam_l1_step(P[0] + (4 if c.misalign else 0), P[1], P[2], P[3], c.n, f(1e-3), f(0.9), f(0.999), f(1e-8), f(c.wd),
                                f(c.l1), None, c.step, None)
        assert rc == ab.adam_rule(c), c
    assert l.mmf_adam_l1_step(P[0], P[1], P[2], P[3], 8, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0), f(0), P[4] + 4, 1, None) == ab.ERR_ALIGN
    for c in ab.refused(ab.DENSE_BWD, ab.dense_bwd_rule):
        if c.rows:
            rc = l.mmf_dense_backward_rows(P[0], c.N + c.rows, P[1], c.N + c.rows, P[2], P[3], c.B, c.K, c.N, c.act, c.drop_kind,
                                           f(0.25), 1, None, P[4], P[5], P[6], P[7], P[8], None)
        else:
            rc = l.mmf_dense_backward(P[0], P[1], P[2], P[3], c.B, c.K, c.N, c.act, c.drop_kind, f(0.25), 1, 1, None, P[5], P[6],
                                      P[7], P[8], None)
        assert rc == ab.dense_bwd_rule(c), c


def test_header_states_every_cap_the_small_rules_restate():
    import os
    from conftest import ROOT
    hdr = " ".join(open(os.path.join(ROOT, "include", "mmf_amil.h")).read().split())
    for text in ("B * K <= 256", "B <= 8192", "K <= 32", "B >= 2", "N <= 2048 and B <= 256"):
        assert text in hdr, text
    assert "batch 1..128" not in hdr
    from multimodalfusion_amd import _lib as m
    assert m.ABI_VERSION == 12


def test_small_tables_hold_what_the_issue_lists():
    acc = lambda t, r: ab.accepted(t, r)
    assert {(c.B, c.K) for c in acc(ab.HEAD, ab.head_rule) if c.B * c.K == 256} == {(8, 32), (256, 1)}
    assert {(c.B, c.K) for c in ab.refused(ab.HEAD, ab.head_rule)} == {(9, 29), (257, 1)}
    assert {c.B for c in acc(ab.COX, ab.cox_rule)} >= {2, 256, 257, 1000, 6145, 8192} and [c.B for c in ab.refused(ab.COX, ab.cox_rule)] == [8193]
    assert {c.n for c in acc(ab.ADAM, ab.adam_rule)} == {1, 3, 4, 5, 1023, 1024, 1025, 1027}
    assert {c.n for c in acc(ab.ABS_SUM, ab.abs_sum_rule)} >= {1, 131071, 131072, 131073} and max(c.n for c in ab.ABS_SUM) >= 7 * 131072 + 1
    assert {c.K for c in acc(ab.HAZ, ab.haz_rule)} >= {1, 4, 32} and {c.K for c in ab.refused(ab.HAZ, ab.haz_rule)} == {0, 33}
    assert {(c.B, c.N) for c in acc(ab.DENSE_BWD, ab.dense_bwd_rule)} >= {(256, 2048), (257, 8), (2, 2052)}
    assert [c.bad_row for c in ab.NLL if c.bad_row >= 0] == [280]


def test_small_inputs_meet_the_conditions_the_gpu_file_relies_on():
    import small_cases as sc
    # argmax is unambiguous: the top two logits of every row differ by >= 1e-3
    for c in ab.accepted(ab.HEAD, ab.head_rule):
        assert sc.top_two_gap(sc.head_ref(c)[0]["logits"]) >= 1e-3, c
    for c in ab.accepted(ab.HAZ, ab.haz_rule):
        assert sc.top_two_gap(sc.haz_inputs(c)["logits"]) >= 1e-3, c
        if c.steep:         # (1 - h) underflows: some fp32 hazard is exactly 1
            assert (sc.haz_ref(c)[0]["h32"] == 1).any() and (np.abs(sc.haz_inputs(c)["logits"]) > 25).all()
    assert any((sc.head_ref(c)[0]["h32"] == 1).any() for c in ab.HEAD if c.steep)
    # nll: labels 0 and K - 1, each under both censorship values; the bad label sits in a row >= 256
    for c in ab.accepted(ab.NLL, ab.nll_rule):
        i = sc.nll_inputs(c)
        if c.B >= 2 * c.K:
            assert {(y, v) for y, v in zip(i["Y"].tolist(), i["c"].tolist())} >= {(y, v) for y in (0, c.K - 1) for v in (0.0, 1.0)}, c
        used = np.concatenate([i["hazards"].ravel(), i["S"].ravel()])          # the eps clamp: no input near eps = 1e-7
        assert ((used > 1e-6) | (used < 1e-8)).all(), c
        if c.bad_row >= 0:
            assert c.bad_row >= 256 and i["Y"][c.bad_row] == c.K and int((i["Y"] >= c.K).sum()) == 1
            assert np.isnan(sc.nll_ref(c)[0]["loss"]) and not sc.nll_ref(c)[0]["gH"][c.bad_row].any()
    # Adam: the live elements do not cancel, the pad-like ones are +0 and -0 under a non-zero l1
    for c in ab.accepted(ab.ADAM, ab.adam_rule):
        for rnd in range(4):
            i = sc.adam_inputs(c, rnd)
            live = ~i["zeros"]
            assert live.any() and (np.abs(i["g"][live]) >= 100 * (c.l1 + c.wd * np.abs(i["w"][live]))).all(), c
            assert (np.sign(i["g"][live]) == np.sign(i["m"][live])).all() and (i["v"][live] > 0).all()
            assert not i["w"][i["zeros"]].any() and not i["g"][i["zeros"]].any()
        if c.n >= 4:
            z = sc.adam_inputs(c)["w"][sc.adam_inputs(c)["zeros"]]
            assert {bool(np.signbit(v)) for v in z} == {True, False}
        if c.mask:          # live elements with w != 0 under mask 0 and under mask 1: in the tail, and from n = 1023 in the vectors
            i, t0 = sc.adam_inputs(c), c.n - c.n % 4
            live = ~i["zeros"] & (i["w"] != 0)
            parts = [np.arange(c.n) >= t0] + ([np.arange(c.n) < t0] if c.n >= 1023 else [])
            for part in parts:
                assert {float(v) for v in i["mask"][live & part]} == {0.0, 1.0}, c
    assert any(c.l1 > 0 and c.n >= 3 and c.n % 4 for c in ab.accepted(ab.ADAM, ab.adam_rule))       # a zero in a scalar tail
    assert any(c.mask and c.l1 > 0 and c.n >= 1023 and c.n % 4 == 3 for c in ab.accepted(ab.ADAM, ab.adam_rule))
    # Cox: every float64 risk-set sum inside fp32 range; the all-censored case is all censored
    for c in ab.accepted(ab.COX, ab.cox_rule):
        D = sc.cox_ref(c)[0]["D"]
        assert np.isfinite(D).all() and D.min() > 1e-30 and D.max() < 1e30, c
        assert bool(sc.cox_inputs(c)["c"].all()) == c.all_censored
        assert c.B == 2 or len(set(sc.cox_inputs(c)["times"])) < c.B           # tied times
    # ranking: the comparable-pair counts the cases claim
    for c in ab.accepted(ab.RANK, ab.rank_rule):
        n, i = sc.rank_ref(c)[0]["pairs"], sc.rank_inputs(c)
        assert {"none": n == 0, "one": n == 1, "many": n > 1000, "tied": 1 < n < 15, "equal risks": n == 15}[c.kind], (c, n)
        if c.kind == "tied":
            assert len(set(i["times"])) < c.B
        if c.kind == "equal risks":
            assert c.phi == 1 and int((i["risks"] == 0.25).sum()) >= 3
    # highway: zn exactly 0 somewhere; the dense backward: no recovered y within 1e-5 of SELU's kink under AlphaDropout
    assert all((sc.highway_inputs(c)["zn"] == 0).any() for c in ab.accepted(ab.HIGHWAY, ab.highway_rule) if c.n >= 4)
    for c in ab.accepted(ab.DENSE_BWD, ab.dense_bwd_rule):
        out, _ = sc.dense_ref(c)
        if c.drop_kind == 2:
            kept = sc.dense_inputs(c)["keep"]
            assert c.act == 4 and np.abs(out["y_rec"][kept]).min() > 1e-5, c
        if c.act in (1, 4):
            assert (out["y_act"] != 0).all() or c.act == 1
        assert np.abs(out["dpre"]).max() > 0


def test_small_bars_cover_every_element():
    """No comparison leaves an element out: every bar has a finite, non-negative value for every element of its reference."""
    import small_cases as sc
    refs = [(ab.HEAD, ab.head_rule, sc.head_ref), (ab.NLL, ab.nll_rule, sc.nll_ref), (ab.COX, ab.cox_rule, sc.cox_ref),
            (ab.RANK, ab.rank_rule, sc.rank_ref), (ab.HAZ, ab.haz_rule, sc.haz_ref), (ab.HIGHWAY, ab.highway_rule, sc.highway_ref),
            (ab.BN, ab.bn_rule, sc.bn_ref), (ab.DENSE_BWD, ab.dense_bwd_rule, sc.dense_ref)]
    for table, rule, ref in refs:
        for c in ab.accepted(table, rule):
            out, bar = ref(c)
            for k, b in bar.items():
                b = np.broadcast_to(np.asarray(b, np.float64), np.shape(out[k]))
                assert np.isfinite(b).all() and (b >= 0).all(), (c, k)
                assert (b[np.asarray(out[k]) != 0] > 0).all(), (c, k)


def test_vectorised_restatements_match_the_ports():
    """The sorted-cumulative-sum Cox and the pair-matrix ranking loss (needed at B = 700 and 8192) against oracle.torch_port
    and oracle.stage2_port, loss and gradient, at sizes the ports' loops afford."""
    import torch
    import small_cases as sc
    from oracle import stage2_port as s2
    from oracle import torch_port as tp
    for c in (ab.Cox(2), ab.Cox(5, all_censored=True), ab.Cox(40), ab.Cox(257)):
        i = sc.cox_inputs(c)
        r = sc.T(i["risks"]).requires_grad_(True)
        want = tp.cox_loss(r, i["times"], torch.as_tensor(i["c"]))
        want.backward()
        loss, d = sc.cox_vectorised(i["risks"], i["times"], i["c"])[:2]
        assert abs(loss - float(want.detach())) <= 1e-12 * max(1, abs(loss)) and np.abs(d - r.grad.numpy()).max() <= 1e-13
    small = [c for c in ab.accepted(ab.RANK, ab.rank_rule) if c.B <= 6]
    for c in small + [ab.Rank(40, p, r) for p in (0, 1) for r in (0, 1)]:
        i = sc.rank_inputs(c)
        r = sc.T(i["risks"]).requires_grad_(True)
        want = s2.ranking_loss(r, torch.as_tensor(i["times"]), sc.T(i["c"]), "sigmoid" if c.phi == 0 else "relu",
                               "mean" if c.reduction == 0 else "sum")
        want.sum().backward()
        grad = np.zeros(c.B) if r.grad is None else r.grad.numpy()
        loss, d = sc.rank_vectorised(i["risks"], i["times"], i["c"], c.phi, c.reduction)[:2]
        assert abs(loss - float(want.detach().sum())) <= 1e-12 * max(1, abs(loss)) and np.abs(d - grad).max() <= 1e-13, c
