"""CPU: the admitted envelope of the scorer, the dense layer, the stack and the tensor-fusion tail (tests/abi_shapes.py) --
the restated rules against the library where it refuses before any HIP call, the restated planners against the library's,
and the case tables of tests/test_gpu_abi_shapes.py and tests/test_gpu_xfusion_shapes.py against the shape classes the
rules make reachable; for the fusion tail also the two workspace queries over a grid on both sides of every limit, and the
fp64 oracle of every case clear of every ReLU kink under the seed the case records; for the small ops (losses, hazard heads,
batch norm, the step tail, the dense backward) also the conditions their generated inputs must meet (tests/small_cases.py) and
the vectorised Cox and ranking restatements against the ports; for the dense forward, gate_mul, kron, xreduce and the omic
step (the tables below DENSE_BWD) the same, the kron caps from both sides, the omic step's workspace query, its margin to
SELU's kink and its censoring patterns, and each numpy reference against oracle/torch_port.py through autograd."""
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
                # the exact-fp32 plan with tick words for every tile on offer: what the workspace query sizes
                pl = b["plan_linear"](M, N, nseg * kseg, nseg, kseg, 0, 0, 0, 2**31 - 1)
                assert S == pl.ksplit and (pl.kind == lp.LIN_KSPLIT_64) == (S > 1), (M, N, nseg, kseg)
                want = S * ((M + 63) // 64) * ((N + 63) // 64) * 64 * 64 * 4 if S > 1 else 0
                assert l.mmf_linear_forward_workspace_bytes(M, N, nseg, kseg) == want
    for c in ab.accepted(ab.LINEAR_FORWARD, ab.linear_forward_rule):
        if c.ws:       # what the issue states for its K-split shapes
            assert ab.linear_ksplit(c.M, c.N, c.K, 1, c.K) == (4 if c.K == 1024 else 2), c
    for M in (1, 3, 5, 64, 65, 129, 1000, 12288):
        for N, K in ((4, 4), (36, 72), (100, 300), (256, 4096), (36, 100)):
            assert ab.linear_bwd_splits(M, N, K) == lp.lib_plan_tn(M, 0, [(N, K, 0)]).splits, (M, N, K)
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


# ---- the dense forward, gate_mul, kron, xreduce and the omic step -------------------------------------------------------------
def _xreduce_io(m_, c, bwd):
    io = m_.XReduceIO(m=c.m, B=c.B, dim=c.dim, sdim=c.sdim)
    names = ["v", "Wh", "bh", "Wz", "bz", "Wo", "bo", "h", "z", "gm", "o"] + (["d_o", "dv", "dWh", "dbh", "dWz", "dbz", "dWo", "dbo"] if bwd else [])
    for k, n in enumerate(names):
        for i in range(max(0, min(c.m, 3))):
            getattr(io, n)[i] = 0x100000 * (k + 1) + 0x1000 * i
    if c.misalign:
        io.v[0] = io.v[0] + 4
    if c.null:
        getattr(io, c.null)[c.m - 1] = None
    return io


def _maxstep_call(m_, l, c):
    names = {n: 0x100000 * (k + 1) for k, n in enumerate(ab.MX_PTRS)}
    if c.null:
        names[c.null] = None
    if c.off:
        names[c.off] += 4
    d = m_.MaxnetDesc(B=c.B, G=c.G, H0=c.H0, H1=256, p_drop=c.p_drop, seed=1, seed_dev=None, sync_words=c.sync_words, trace=None,
                      **{k: names[k] for k in ("x", "W0", "b0", "W1", "b1", "Wc", "bc", "sync")})
    g = m_.MaxnetGrads(**{k: names[k] for k in ("dW0", "db0", "dW1", "db1", "dWc", "dbc")})
    ws = l.mmf_maxnet_cox_step_workspace_bytes(c.B) - (1 if c.ws_short else 0)
    return l.mmf_maxnet_cox_step(C.byref(d), names["times"], names["c"], C.c_float(c.loss_scale), names["workspace"], ws,
                                 names["risk"], names["loss"], C.byref(g), c.accumulate, None)


def test_tail_refusals_in_the_library():
    """Every refusal of the five new tables returns before a launch: reproduced with pointers that are never read."""
    m_, l = _lib()
    f = C.c_float
    for c in ab.refused(ab.DENSE_FWD, ab.dense_fwd_rule):
        if c.rows:
            rc = l.mmf_dense_forward_rows(P[0], P[1], P[2], c.B, c.K, c.N, c.act, c.drop_kind, f(c.drop_p), 1, None,
                                          P[3] if c.base else None, P[4], c.N - 1 if c.rows < 0 else c.N, None)
        else:
            rc = l.mmf_dense_forward(P[0], P[1], P[2], c.B, c.K, c.N, c.act, c.drop_kind, f(c.drop_p), 1, 1, None, P[4], None)
        assert rc == ab.dense_fwd_rule(c) != ab.OK, c
    for ptrs in ((None, P[1], P[2]), (P[0], None, P[2]), (P[0], P[1], None)):       # x, W, y
        assert l.mmf_dense_forward(ptrs[0], ptrs[1], P[3], 2, 8, 8, 0, 0, f(0), 1, 1, None, ptrs[2], None) == ab.ERR_ARG
    for c in ab.refused(ab.GATE_MUL, ab.gate_mul_rule):
        assert l.mmf_gate_mul_forward(P[0], P[1], P[2], c.n, None) == ab.gate_mul_rule(c)
        assert l.mmf_gate_mul_backward(P[0], P[1], P[2], P[3], P[4], c.n, None) == ab.gate_mul_rule(c)
    for c in ab.refused(ab.KRON, ab.kron_rule):
        n = max(c.m, 1)
        o = (C.c_void_p * n)(*[None if c.null and t == c.m - 1 else P[t] for t in range(n)])
        d = (C.c_void_p * n)(*P[4:4 + n])
        assert l.mmf_kron_forward(o, c.m, c.dim, c.B, f(c.drop_p), 1, 1, None, P[8], None) == ab.kron_rule(c) != ab.OK, c
        assert l.mmf_kron_backward(P[9], o, c.m, c.dim, c.B, f(c.drop_p), 1, 1, None, d, None) == ab.kron_rule(c), c
    for c in ab.XREDUCE:
        if ab.xreduce_fwd_rule(c) != ab.OK:
            assert l.mmf_xreduce_forward(C.byref(_xreduce_io(m_, c, False)), f(c.drop_p), 1, None, None) == ab.xreduce_fwd_rule(c), c
        if ab.xreduce_bwd_rule(c) != ab.OK:
            assert l.mmf_xreduce_backward(C.byref(_xreduce_io(m_, c, True)), f(c.drop_p), 1, None, None) == ab.xreduce_bwd_rule(c), c
    for name in ("v", "Wh", "bh", "Wz", "bz", "Wo", "bo", "h", "z", "gm", "o"):      # any NULL member, both directions
        c = ab.XReduce(2, 1, 4, 4, null=name)
        assert l.mmf_xreduce_forward(C.byref(_xreduce_io(m_, c, False)), f(0), 1, None, None) == ab.xreduce_fwd_rule(c) == ab.ERR_ARG, name
        assert l.mmf_xreduce_backward(C.byref(_xreduce_io(m_, c, True)), f(0), 1, None, None) == ab.xreduce_bwd_rule(c) == ab.ERR_ARG, name
    for name in ("d_o", "dv", "dWh", "dbh", "dWz", "dbz", "dWo", "dbo"):            # the backward's own members
        c = ab.XReduce(2, 1, 4, 4, null=name)
        assert l.mmf_xreduce_backward(C.byref(_xreduce_io(m_, c, True)), f(0), 1, None, None) == ab.ERR_ARG, name
    for c in (ab.XReduce(1, 65536, 4, 65536), ab.XReduce(3, 46341, 4, 46341), ab.XReduce(3, 2**31 - 1, 4, 2**31 - 1)):
        # m * B * sdim wraps an int (to 0, to a negative value) or an int64: still above the cap of 384, in both directions
        assert ab.xreduce_fwd_rule(c) == ab.xreduce_bwd_rule(c) == ab.ERR_SHAPE
        assert l.mmf_xreduce_forward(C.byref(_xreduce_io(m_, c, False)), f(0), 1, None, None) == ab.ERR_SHAPE, c
        assert l.mmf_xreduce_backward(C.byref(_xreduce_io(m_, c, True)), f(0), 1, None, None) == ab.ERR_SHAPE, c
    # the plain dense forward's 32-bit mask index: B * N >= 2^32 is refused where a mask is drawn (never launched: no such
    # shape is called without dropout here); the _rows form indexes row_base[b] + n and has no such limit in its rule
    for B, N in ((65536, 65536), (2**31 - 1, 3)):
        c = ab.DenseFwd(B, 8, N, drop_kind=1)
        assert ab.dense_fwd_rule(c) == ab.ERR_SHAPE == l.mmf_dense_forward(P[0], P[1], P[2], B, 8, N, 0, 1, f(0.25), 1, 1, None, P[4], None)
        assert ab.dense_fwd_rule(dataclasses.replace(c, drop_kind=0)) == ab.dense_fwd_rule(dataclasses.replace(c, rows=1)) == ab.OK
    assert ab.dense_fwd_rule(ab.DenseFwd(65536, 8, 65535, drop_kind=2)) == ab.OK
    for c in ab.refused(ab.MAXSTEP, ab.maxstep_rule):
        assert _maxstep_call(m_, l, c) == ab.maxstep_rule(c) != ab.OK, c


def test_kron_caps_from_both_sides():
    """F1: B * S^m < 2^31 and B <= 65535 -- the rule on both sides of every limit (the admitted side is never launched)."""
    K = ab.Kron
    for c, want in ((K(3, 1289), ab.OK), (K(3, 1290), ab.ERR_SHAPE), (K(2, 46339), ab.OK), (K(2, 46340), ab.ERR_SHAPE),
                    (K(2, 255, B=32767), ab.OK), (K(2, 255, B=32768), ab.ERR_SHAPE), (K(2, 1, B=65535), ab.OK), (K(2, 1, B=65536), ab.ERR_SHAPE),
                    (K(3, 2**31 - 2), ab.ERR_SHAPE), (K(2, 2**31 - 1), ab.ERR_SHAPE)):
        assert ab.kron_rule(c) == want, c
    assert 1290 ** 3 < 2**31 <= 1291 ** 3 and 46340 ** 2 < 2**31 <= 46341 ** 2
    m_, l = _lib()
    o, d = (C.c_void_p * 3)(*P[:3]), (C.c_void_p * 3)(*P[4:7])
    for m, dim in ((3, 2**31 - 2), (2, 2**31 - 1), (3, 65535), (2, 65536)):          # S^m beyond int64 / int: still refused, not wrapped
        assert l.mmf_kron_forward(o, m, dim, 1, C.c_float(0), 1, 1, None, P[8], None) == ab.ERR_SHAPE
        assert l.mmf_kron_backward(P[9], o, m, dim, 1, C.c_float(0), 1, 1, None, d, None) == ab.ERR_SHAPE
    assert {(c.m, c.dim, c.B) for c in ab.KRON if ab.kron_rule(c) == ab.ERR_SHAPE} == ab.KRON_CAPS


def test_maxstep_workspace_query_matches_the_restated_size():
    m_, l = _lib()
    for B in (-3, 0, 1, 4, 5, 63, 64, 65, 127, 128, 129, 200, 255, 256):
        assert l.mmf_maxnet_cox_step_workspace_bytes(B) == ab.maxstep_workspace_bytes(B), B


def test_tail_header_changes_keep_the_abi_version():
    """The header changes of these entry points are comments, and refusals of shapes and pointers that were never valid: the
    ABI version stays where it was.  (What the header says is checked against the library by the refusal pins above.)"""
    from multimodalfusion_amd import _lib as m
    assert m.ABI_VERSION == 12


def test_tail_tables_hold_what_the_issue_lists():
    acc = ab.accepted
    d = acc(ab.DENSE_FWD, ab.dense_fwd_rule)
    assert {c.K for c in d} >= {1, 63, 64, 65, 255, 256, 257, 513} and {c.B * c.N for c in d} >= {1, 3, 4, 5}
    assert (2049, 1, 2048) in {(c.B, c.K, c.N) for c in d} and 2049 * 2048 > 4 * ab.DENSE_FWD_GRID == 4194240
    assert {c.act for c in d} == {0, 1, 2, 3, 4} and {c.drop_kind for c in d} == {0, 1, 2} and any(not c.bias for c in d)
    assert {c.rows == 1 for c in d if c.rows} == {True, False} and len(ab.refused(ab.DENSE_FWD, ab.dense_fwd_rule)) == 8
    assert [c.n for c in acc(ab.GATE_MUL, ab.gate_mul_rule)] == [1, 255, 256, 257, 1000]
    k = acc(ab.KRON, ab.kron_rule)
    assert {(c.m, c.dim) for c in k} == {(2, 1), (2, 15), (2, 16), (3, 5), (3, 6), (3, 16), (2, 63), (2, 64), (3, 7), (3, 8)}
    assert {c.B for c in k} == {1, 3} and {c.drop_p > 0 for c in k} == {True, False}
    assert {(c.m, c.dim, c.null) for c in ab.refused(ab.KRON, ab.kron_rule) if ab.kron_rule(c) == ab.ERR_ARG} == {(1, 4, False), (4, 4, False), (2, 0, False), (3, 4, True)}
    x = acc(ab.XREDUCE, ab.xreduce_fwd_rule)
    assert {c.dim for c in x} >= {4, 252, 256, 260, 1024, 1028} and {c.sdim for c in x} >= {1, 15, 16, 17, 32, 33, 384}
    assert {(c.m, c.B, c.sdim) for c in x} >= {(1, 1, 1), (2, 1, 16), (3, 1, 16), (3, 8, 16), (1, 1, 32), (1, 1, 33), (1, 1, 384)}
    assert {c.B for c in x} >= {1, 2, 8}
    one_sided = [c for c in ab.XREDUCE if ab.xreduce_fwd_rule(c) != ab.OK and ab.xreduce_bwd_rule(c) == ab.OK]
    assert sorted((ab.xreduce_fwd_rule(c), c.dim % 4 != 0, c.misalign) for c in one_sided) == [(ab.ERR_ALIGN, False, True), (ab.ERR_SHAPE, True, False)]
    assert {(c.m, c.B, c.sdim) for c in ab.XREDUCE if ab.xreduce_bwd_rule(c) == ab.ERR_SHAPE} == {(3, 8, 17), (1, 1, 385)}
    s = acc(ab.MAXSTEP, ab.maxstep_rule)
    assert {c.G for c in s if ab.maxstep_route(c) == "narrow"} == {4, 16, 36, 60, 64}
    assert {c.G for c in s if ab.maxstep_route(c) == "chunked"} >= {1, 63, 65, 128, 129, 193, 256}
    assert [c.G for c in s if c.misalign] == [36]
    assert {c.B for c in s} >= {1, 3, 4, 5, 127, 128, 129, 255, 256, 15, 16, 17, 19, 63, 64, 65} and 10 <= len(s) <= 16
    assert {n.null for n in ab.MAXSTEP if n.null} == set(ab.MX_PTRS)
    assert {(c.B, c.G) for c in ab.refused(ab.MAXSTEP, ab.maxstep_rule) if not c.null} >= {(0, 36), (257, 36), (8, 0), (8, 257)}


def test_tail_inputs_meet_the_conditions_the_gpu_file_relies_on():
    import small_cases as sc
    # the omic step: no unit of either layer within 4 worst-case summation bounds of SELU's kink (the share excused is 0), both
    # SELU branches in both layers, both mask states in both layers of a train-mode case, negative pre-activations above -4
    for c in ab.accepted(ab.MAXSTEP, ab.maxstep_rule):
        out, bar, facts = sc.maxstep_ref(c)
        i = sc.maxstep_inputs(c)
        assert facts["kink0"] >= 4 and facts["kink1"] >= 4, (c, facts["kink0"], facts["kink1"])
        assert facts["branches"] == [True, True] and facts["min_pre"] > -4, c
        assert facts["masks"] == ([True, True] if c.p_drop > 0 else [False, False]), c
        t, cens = i["times"], i["c"]
        if c.censor == "all":
            assert cens.all() and out["loss"] == 0 and all(not out[k].any() for k in sc.MX_GRADS)
        elif c.censor == "none":
            assert not cens.any()
        elif c.censor == "tied":
            assert len(set(t)) < c.B and not cens.all()
        elif c.censor == "last event":
            assert int((cens == 0).sum()) == 1 and t[cens == 0][0] == t.max() and len(set(t)) == c.B
        else:
            assert len(set(t)) == c.B and (c.B < 3 or 0 < cens.sum() < c.B), c
        if c.accumulate:
            assert all(np.abs(i["prior"][k]).min() > 0 for k in sc.MX_GRADS)
        if c.word:           # the masks of seed + word differ from those of the seed alone
            assert (i["keep0"] != sc.maxstep_inputs(dataclasses.replace(c, word=0))["keep0"]).any()
    # xreduce: the masks of the three sites differ pairwise, and each has both states
    for c in ab.accepted(ab.XREDUCE, ab.xreduce_bwd_rule):
        if c.drop_p > 0:
            ks = sc.xreduce_inputs(c)["keep"]
            assert all((ks[a] != ks[b]).any() for a in range(c.m) for b in range(a)) and all(k.any() and not k.all() for k in ks), c
        out, _ = sc.xreduce_ref(c)
        for t in range(c.m):      # the ReLUs the backward branches on: read off fp32 values that are what the kernel is given
            assert (out["h32"][t] > 0).any() and np.abs(out[f"dv{t}"]).max() > 0, c
    for c in ab.accepted(ab.KRON, ab.kron_rule):
        if c.drop_p > 0:
            k = sc.kron_inputs(c)["keep"]
            assert k.any() and not k.all(), c
    for c in ab.accepted(ab.DENSE_FWD, ab.dense_fwd_rule):
        i = sc.dense_fwd_inputs(c)
        if c.drop_kind:
            assert i["keep"].any() and (c.B * c.N < 8 or not i["keep"].all()), c
        if c.rows:                # rows draw different masks: row b is not row 0 of the plain form shifted
            assert len(set(sc.dense_fwd_row_seeds(c))) == c.B
            if c.drop_kind:
                assert (i["keep"] != sc.gen.keep_mask(sc.SEED, sc.SITE, c.B, c.N, i["p"])).any(), c


def test_tail_bars_cover_every_element():
    import small_cases as sc
    refs = [(ab.DENSE_FWD, ab.dense_fwd_rule, sc.dense_fwd_ref), (ab.GATE_MUL, ab.gate_mul_rule, sc.gate_mul_ref),
            (ab.KRON, ab.kron_rule, sc.kron_ref), (ab.XREDUCE, ab.xreduce_bwd_rule, sc.xreduce_ref),
            (ab.MAXSTEP, ab.maxstep_rule, lambda c: sc.maxstep_ref(c)[:2])]
    for table, rule, ref in refs:
        for c in ab.accepted(table, rule):
            out, bar = ref(c)
            for k, b in bar.items():
                b = np.broadcast_to(np.asarray(b, np.float64), np.shape(out[k]))
                assert np.isfinite(b).all() and (b >= 0).all(), (c, k)
                if not (table is ab.MAXSTEP and c.censor in ("all", "last event")):      # exact zeros of censored rows: bar 0
                    assert (b[np.asarray(out[k]) != 0] > 0).all(), (c, k)


def test_tail_restatements_match_the_ports():
    """The numpy references against oracle/torch_port.py through autograd, at the shipped sizes: the omic step (maxnet_forward,
    cox_loss) at G = 36 and 186; xreduce at m = 2 and m = 3 through xfusion with encoder weights that pass the Kronecker product through; the
    Kronecker product and its backward against the bmm chain xfusion uses."""
    import torch
    import small_cases as sc
    from oracle import torch_port as tp
    for c in (ab.MaxStep(4, 36, p_drop=0.25), ab.MaxStep(64, 186, p_drop=0.25), ab.MaxStep(65, 36), ab.MaxStep(16, 63, censor="tied")):
        i = sc.maxstep_inputs(c)
        sd = tp.to_torch(sc.maxstep_state_dict(i))
        keeps = [sc.T(i["keep0"]), sc.T(i["keep1"])] if c.p_drop > 0 else None
        risk = tp.maxnet_forward(sd, sc.T(i["x"]), nll=False, keeps=keeps)[0]
        loss = tp.cox_loss(risk, i["times"], torch.as_tensor(i["c"]))
        grads = tp.grads_of(loss, sd)
        out, _, facts = sc.maxstep_ref(c)
        assert np.abs(out["risk"] - risk.detach().numpy()).max() <= 1e-12 and abs(out["loss"] - float(loss.detach())) <= 1e-12
        for k, name in zip(sc.MX_GRADS, ("fc_omic.0.0.weight", "fc_omic.0.0.bias", "fc_omic.1.0.weight", "fc_omic.1.0.bias",
                                         "classifier.weight", "classifier.bias")):
            want = grads[name].numpy()
            assert np.abs(facts["pure"][k].reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (c, k)
    # xreduce at both shipped sizes (m = 2 and m = 3): encoder1 = I, encoder2 = [I | 0] hand xfusion's Kronecker product through,
    # o_t is read off it where every other operand contributes its appended 1, and the loss weights those entries by d_o
    for c in (ab.XReduce(2, 1, 256, 16, drop_p=0.25), ab.XReduce(3, 1, 256, 16, drop_p=0.25)):
        i = sc.xreduce_inputs(c)
        m, n = c.m, 17 ** c.m
        sd = {}
        for t in range(m):
            for j, (w, b) in enumerate((("Wh", "bh"), ("Wz", "bz"), ("Wo", "bo"))):
                sd[f"mm.reduce.{t}.{j}.0.weight"], sd[f"mm.reduce.{t}.{j}.0.bias"] = i[w][t], i[b][t]
        sd = tp.to_torch(sd)
        eye = torch.eye(n, dtype=torch.float64)
        sd.update({"mm.encoder1.0.weight": eye, "mm.encoder1.0.bias": torch.zeros(n, dtype=torch.float64),
                   "mm.encoder2.0.weight": torch.cat([eye, torch.zeros(n, m * 256, dtype=torch.float64)], 1),
                   "mm.encoder2.0.bias": torch.zeros(n, dtype=torch.float64)})
        vs = [sc.T(v).requires_grad_(True) for v in i["v"]]
        masks = {f"o{t}": sc.T(i["keep"][t]) / (1 - c.drop_p) for t in range(m)}
        full = tp.xfusion(sd, "mm", vs, masks).reshape((17,) * m)
        out, _ = sc.xreduce_ref(c)
        L = 0
        for t in range(m):
            o_t = full[tuple(slice(0, 16) if u == t else 16 for u in range(m))]
            assert np.abs(o_t.detach().numpy() - out[f"o{t}"][0]).max() <= 1e-12, (c, t)
            L = L + (o_t * sc.T(i["d_o"][t][0])).sum()
        g = torch.autograd.grad(L, vs + [sd[f"mm.reduce.{t}.{j}.0.{w}"] for t in range(m) for j in range(3) for w in ("weight", "bias")])
        names = [f"dv{t}" for t in range(m)] + [f"d{w}{t}" for t in range(m) for w in ("Wh", "bh", "Wz", "bz", "Wo", "bo")]
        for k, want in zip(names, g):        # the backward reference starts from the forward rounded to fp32: 2^-24 relative apart
            want = want.numpy()
            assert np.abs(want).max() > 0 and np.abs(out[k].reshape(want.shape) - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (c, k)
    for c in (ab.Kron(2, 16), ab.Kron(3, 16, B=3, drop_p=0.25)):
        i = sc.kron_inputs(c)
        os_ = [sc.T(o).requires_grad_(True) for o in i["o"]]
        ext = [torch.cat((o, torch.ones(c.B, 1, dtype=o.dtype)), 1) for o in os_]
        fus = ext[0]
        for o in ext[1:]:
            fus = torch.bmm(fus.unsqueeze(2), o.unsqueeze(1)).flatten(start_dim=1)
        if c.drop_p > 0:
            fus = fus * sc.T(i["keep"]) / (1 - c.drop_p)
        out, _ = sc.kron_ref(c)
        assert np.abs(out["out"] - fus.detach().numpy()).max() <= 1e-13
        for t, want in enumerate(torch.autograd.grad((fus * sc.T(i["g"])).sum(), os_)):
            assert np.abs(out[f"d{t}"] - want.numpy()).max() <= 1e-12, (c, t)


# ---- the row cap of the attention stack: the rule, the operand census, the library at cap and cap + 1 --------------------
CAP_STACKS = ab.cap_stacks()
_cap_id = lambda k: f"{k[0]} {k[1].size} {'gated' if k[1].gated else 'ungated'}"


def _chain_cap(chain, c):
    return ab.group_row_cap(c) if chain.startswith("group") else ab.stack_row_cap(c)


def test_row_cap_restates_check_desc():
    """stack_rule with N: the cap from both sides, for every admitted stack; the issue's figures."""
    for chain, c in CAP_STACKS:
        cap = ab.stack_row_cap(c)
        assert ab.stack_rule(c, cap) == ab.OK and ab.stack_rule(c, cap + 1) == ab.ERR_SHAPE, (chain, c)
        assert ab.stack_rule(c, 0) == ab.ERR_SHAPE
        assert cap * max(c.H, c.D) < 2**30, "the mask-index rule would bind"
    S = ab.Stack
    assert ab.stack_row_cap(S(32, 256, 128, False)) == 2**21 - 1 and ab.stack_row_cap(S(160, 512, 640, True)) == 419430
    assert ab.stack_row_cap(S(128, 1024, 128, True)) == ab.stack_row_cap(S(32, 1024, 384, False)) == 2**19 - 1
    assert ab.stack_row_cap(S(1024, 256, 256, True)) == 2**19 - 1 == lp.N_MAX["fp32"]
    assert ab.stack_row_cap(S(1024, 256, 256, True, bf16=True)) == ab.stack_row_cap(S(64, 1024, 128, True, bf16=True)) == 2**20 - 1
    assert ab.stack_row_cap(S(1024, 256, 256, True, bf16=True)) == lp.N_MAX["bf16"]
    assert ab.stack_row_cap(S(64, 512, 384, False, bf16=True)) == 1398101
    assert ab.group_row_cap(S(96, 256, 128, False)) == 2**21 - 1 and ab.GROUP_POOL_GROUPS * ab.POOL_MAX_ROWS == 2**21
    assert ab.GROUP_BAG_MAX_PARTIALS * ab.POOL_MAX_ROWS > ab.GROUP_POOL_GROUPS * ab.POOL_MAX_ROWS     # the per-bag limit never binds
    assert ab.group_rule(S(96, 256, 128, False), (337, 2**21 - 1 - 337)) == ab.OK
    assert ab.group_rule(S(96, 256, 128, False), (338, 2**21 - 1 - 337)) == ab.ERR_SHAPE
    assert ab.group_rule(S(96, 256, 128, False), (1,) * 65) == ab.ERR_SHAPE


def _library_cap(chain, c):
    """The largest N the library itself admits for the chain's forward call (bisection over fake-pointer calls that stop at
    the zero-byte workspace): the census below is taken at the library's cap, not at the restated one."""
    m, l = _lib()
    first = {"f32": "forward", "f32 infer": "infer", "bf16 fused": "forward", "bf16 unfused": "forward", "bf16 infer": "infer",
             "group": "mmf_amil_nll_step_group", "group infer": "mmf_amil_infer_group"}[chain]
    pins = "group" if chain.startswith("group") else chain.replace(" infer", "") if chain != "bf16 infer" else "bf16 unfused"
    lo, hi = 338, 2**33                      # admitted, refused
    assert _stack_calls(m, l, pins, c, lo)[first] == ab.ERR_WORKSPACE and _stack_calls(m, l, pins, c, hi)[first] == ab.ERR_SHAPE
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _stack_calls(m, l, pins, c, mid)[first] == ab.ERR_WORKSPACE else (lo, mid)
    return lo


@pytest.mark.parametrize("chain,c", CAP_STACKS, ids=map(_cap_id, CAP_STACKS))
def test_every_operand_is_below_2_gib_at_the_row_cap(chain, c):
    """The census, at the cap the library itself enforces: at the cap no operand of the chain reaches 2^31 bytes -- the condition under which the kernels' 32-bit
    offsets, record counts and the reads-as-zero offset are right.  With max(L, 2 D) as check_desc's `widest` this fails for
    h and du of Stack(128, 1024, 128) (8 GiB at 2,097,151 rows) and Stack(32, 1024, 384) (2.7 GiB at 699,050)."""
    cap = _library_cap(chain, c)
    over = {k: v for k, v in ab.census_bytes(chain, c, cap).items() if v >= 2**31}
    assert not over, (chain, c.size, cap, over)
    assert cap == _chain_cap(chain, c)


@pytest.mark.parametrize("chain,c", CAP_STACKS, ids=map(_cap_id, CAP_STACKS))
def test_the_row_cap_is_tight(chain, c):
    """At cap + 1 an operand reaches 2^31 bytes.  Where 2 D is the widest of a chain that stores no 2 D-wide row (fp32: a and
    b apart; an ungated bf16 stack: dP is [N x D]) the rule's 2 D term is conservative by census_slack: there the largest
    operand, scaled by that factor, reaches 2^31 -- the rule refuses exactly what its formula says, no earlier."""
    if chain.startswith("group") and ab.group_row_cap(c) < ab.stack_row_cap(c):
        pytest.fail("a window whose pooling-group limit binds below the byte cap: restate its tightness here")
    n = _chain_cap(chain, c) + 1
    slack = ab.census_slack(chain, c)
    assert slack >= 1
    rows = [name for name, rows, *_ in ab.census(chain, c) if rows is ab._rows]
    top = max(v for k, v in ab.census_bytes(chain, c, n).items() if k in rows)
    assert top * slack >= 2**31, (chain, c.size, n, top, slack)
    if max(c.L, c.H) >= 2 * c.D or (chain.startswith("bf16") and chain != "bf16 infer" and c.gated):
        assert slack == 1


def _head(m):
    return m.SurvHead(Wk=P[8], bk=P[9], K=4, logits=P[10], hazards=P[11], S=P[12], Y_hat=P[13], risk=None)


def _target(m):
    return m.NllTarget(Y=P[8], c=P[9], alpha=0.0, eps=1e-7, loss_scale=1.0, loss=P[10], dWk=P[11], dbk=P[12], accumulate=0)


def _grads_p(m):
    return m.AmilGrads(dW1=P[8], db1=P[9], dWa=P[10], dba=P[11], dWb=P[12], dbb=P[13], dWc=P[14], dbc=P[15], dx=None)


def _stack_calls(m, l, chain, c, N):
    """Every entry point of the chain at N rows on fake pointers with a zero-byte workspace: an admitted shape gets as far as
    the workspace check (MMF_ERR_WORKSPACE), which comes before the first launch and the first pointer read."""
    d = _desc(m, c, N=N)
    by, x, ws, A = C.byref, P[8], P[9], P[10]
    head, tgt, g = _head(m), _target(m), _grads_p(m)
    if chain == "scorer":
        return {"mmf_attn_net_forward": l.mmf_attn_net_forward(by(d), x, ws, 0, A, None),
                "mmf_attn_net_backward": l.mmf_attn_net_backward(by(d), x, ws, 0, A, by(g), None)}
    if chain.startswith("group"):
        offs = (C.c_int64 * 3)(0, 337, N)
        seeds = (C.c_uint32 * 2)(1, 2)
        grp = m.BagGroup(G=2, offsets=offs, seeds=seeds)
        return {"mmf_amil_nll_step_group": l.mmf_amil_nll_step_group(by(d), by(grp), x, ws, 0, by(head), by(tgt), A, by(g), None),
                "mmf_amil_infer_group": l.mmf_amil_infer_group(by(d), by(grp), x, 0, ws, 0, by(head), None, P[11], A, None),
                "mmf_amil_group_forward": l.mmf_amil_group_forward(by(d), by(grp), x, ws, 0, P[11], c.H, A, None),
                "mmf_amil_group_backward": l.mmf_amil_group_backward(by(d), by(grp), x, ws, 0, P[11], c.H, A, by(g), 0, None)}
    b = 1 if c.bf16 else 0
    fwd, bwd, infer = ((l.mmf_amil_bf16_forward, l.mmf_amil_bf16_backward, l.mmf_amil_bf16_infer) if b else
                       (l.mmf_amil_forward, l.mmf_amil_backward, l.mmf_amil_infer))
    return {"forward": fwd(by(d), x, ws, 0, P[11], A, None),
            "backward": bwd(by(d), x, ws, 0, P[11], A, P[12], None, by(g), None),
            "infer": infer(by(d), x, ws, 0, P[11], A, None),
            "mmf_amil_head_forward": l.mmf_amil_head_forward(by(d), x, b, ws, 0, by(head), P[11], A, None),
            "mmf_amil_nll_step": l.mmf_amil_nll_step(by(d), x, b, ws, 0, by(head), by(tgt), A, by(g), None)}


CAP_PINS = [k for k in CAP_STACKS if k[0] in ("f32", "bf16 fused", "bf16 unfused", "group")]
SCORERS = [ab.Attn(1, 256, 128, True), ab.Attn(1, 1024, 128, True), ab.Attn(1, 160, 256, False), ab.Attn(1, 128, 160, True)]
CAP_PINS += [("scorer", a) for a in SCORERS]


@pytest.mark.parametrize("chain,c", CAP_PINS, ids=[f"{k[0]} {getattr(k[1], 'size', (k[1].H, k[1].D))}" for k in CAP_PINS])
def test_the_library_refuses_cap_plus_one_and_admits_the_cap(chain, c):
    """Forward, backward, head_forward, nll_step, their bf16 forms, both infer calls, the grouped calls on sum N, the scorer."""
    m, l = _lib()
    cap = (2**31 - 1) // (max(c.H, 2 * c.D) * 4) if chain == "scorer" else _chain_cap(chain, c)
    if chain == "scorer":
        assert ab.attn_rule(dataclasses.replace(c, N=cap)) == ab.OK and ab.attn_rule(dataclasses.replace(c, N=cap + 1)) == ab.ERR_SHAPE
    for name, rc in _stack_calls(m, l, chain, c, cap).items():
        assert rc == ab.ERR_WORKSPACE, (name, rc, "at the cap: admitted, stopped by the zero-byte workspace")
    for name, rc in _stack_calls(m, l, chain, c, cap + 1).items():
        assert rc == ab.ERR_SHAPE, (name, rc, "at cap + 1")


def _ws_bytes(l, chain, c, N):
    a = (N, c.L, c.H, c.D, 1 if c.gated else 0) if chain != "scorer" else None
    if chain.startswith("group"):
        offs = (C.c_int64 * 3)(0, 337, N)
        if chain == "group":
            return l.mmf_amil_group_workspace_bytes(offs, 2, *a[1:])
        return l.mmf_amil_group_infer_workspace_bytes(offs, 2, *a[1:], 0)
    return {"f32": l.mmf_amil_workspace_bytes, "f32 infer": l.mmf_amil_infer_workspace_bytes,
            "bf16 fused": l.mmf_amil_bf16_workspace_bytes, "bf16 unfused": l.mmf_amil_bf16_workspace_bytes,
            "bf16 infer": l.mmf_amil_bf16_infer_workspace_bytes}[chain](*a)


@pytest.mark.parametrize("chain,c", CAP_STACKS, ids=map(_cap_id, CAP_STACKS))
def test_workspace_queries_do_not_wrap_at_the_cap(chain, c):
    """The query at the cap holds every workspace operand of the census (each in its 256-byte slot) and is no smaller than
    at cap - 1: no 32-bit product inside the carve."""
    m, l = _lib()
    cap = _chain_cap(chain, c)
    at, below = _ws_bytes(l, chain, c, cap), _ws_bytes(l, chain, c, cap - 1)
    assert at >= ab.census_workspace(chain, c, cap), (chain, c.size, at, ab.census_workspace(chain, c, cap))
    assert at >= below > 0
    if chain == "group infer":      # with x_bf16 the query is the larger of the two storages
        offs = (C.c_int64 * 3)(0, 337, cap)
        assert l.mmf_amil_group_infer_workspace_bytes(offs, 2, c.L, c.H, c.D, 1 if c.gated else 0, 1) >= at


def test_scorer_workspace_query_does_not_wrap_at_the_cap():
    m, l = _lib()
    for a in SCORERS:
        cap = (2**31 - 1) // (max(a.H, 2 * a.D) * 4)
        c = dataclasses.replace(a, N=cap)
        assert max(ab.census_bytes("scorer", c, cap).values()) < 2**31
        at = l.mmf_attn_net_workspace_bytes(cap, a.H, a.D, 1 if a.gated else 0)
        assert at >= ab.census_workspace("scorer", c, cap) and at >= l.mmf_attn_net_workspace_bytes(cap - 1, a.H, a.D, 1 if a.gated else 0)


def test_header_states_the_row_cap():
    import os
    from conftest import ROOT
    from multimodalfusion_amd import _lib as m
    hdr = open(os.path.join(ROOT, "include", "mmf_amil.h")).read()
    desc = hdr[hdr.index("typedef struct mmf_amil_desc"):hdr.index("} mmf_amil_desc;")]
    assert "N * max(L, H, 2 * D) * 4 < 2^31" in desc and "MMF_ERR_SHAPE" in desc and "524,287" in desc
    bf = hdr[hdr.index("bf16-storage variant"):hdr.index("mmf_amil_bf16_workspace_bytes")]
    assert "N * max(L, H, 2 * D) * 2 < 2^31" in bf and "mmf_amil_desc::N" in bf
    for section in ("Grouped training step:", "Grouped forward-only pass:"):
        s = hdr[hdr.index(section):]
        assert "mmf_amil_desc::N's row cap" in s[:s.index("-- */")] and "2,097,152" in s[:s.index("-- */")]
    scorer = hdr[hdr.index("The attention scorer on its own"):hdr.index("mmf_attn_net_workspace_bytes")]
    assert "N * max(H, 2 * D) * 4 < 2^31" in scorer
    assert m.ABI_VERSION == 12
