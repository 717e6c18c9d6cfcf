"""CPU checks of the grouped multimodal step in the C ABI (include/mmf_amil.h: mmf_amil_group_forward / _backward,
mmf_radio_group_forward / _backward, mmf_surv_head_nll_step_group and its workspace query, mmf_dense_forward_rows /
_backward_rows, mmf_dropout_row_base): the structs these entry points take are laid out in ctypes as the header compiled
as C lays them out, every new prototype has the arity its binding declares, the head's workspace query answers 0 outside
its limits, refusals that need no device come back as error codes, and the ABI version is unchanged (the entry points
are additive; no new struct).  Needs the built library, not a GPU."""
import ctypes as C
import re

from test_abi_layout_cpu import HEADER, _c_layout

NEW = ["mmf_amil_group_forward", "mmf_amil_group_backward", "mmf_radio_group_forward", "mmf_radio_group_backward",
       "mmf_surv_head_group_workspace_bytes", "mmf_surv_head_nll_step_group", "mmf_dropout_row_base",
       "mmf_dense_forward_rows", "mmf_dense_backward_rows"]


def test_structs_of_the_new_entry_points_match_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    mirrors = {"mmf_bag_group": _lib.BagGroup, "mmf_radio_reduce": _lib.RadioReduce, "mmf_surv_head": _lib.SurvHead,
               "mmf_nll_target": _lib.NllTarget, "mmf_amil_grads": _lib.AmilGrads, "mmf_amil_desc": _lib.AmilDesc}
    got = _c_layout(tmp_path, {c: [n for n, _ in m._fields_] for c, m in mirrors.items()})
    for cname, m in mirrors.items():
        assert got[(cname, "sizeof")] == C.sizeof(m), cname
        for n, _ in m._fields_:
            assert got[(cname, n)] == getattr(m, n).offset, (cname, n)


def test_new_symbols_are_bound_with_the_headers_arity_and_the_abi_version_is_unchanged():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    assert _lib.ABI_VERSION == 12 and l.mmf_abi_version() == 12
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(l, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_head_group_workspace_query():
    from multimodalfusion_amd import _lib
    q = _lib.lib().mmf_surv_head_group_workspace_bytes
    for G in range(1, 65):
        assert q(768, 4, G) >= 4 * (G * 4 * 768 + G * 4), G          # the per-patient slabs of dWk and dbk
    assert q(768, 4, 1) < q(768, 4, 64) and q(768, 4, 64) < q(1024, 32, 64)
    assert q(768, 4, 0) == 0 and q(768, 4, 65) == 0 and q(768, 4, -1) == 0
    assert q(0, 4, 16) == 0 and q(1025, 4, 16) == 0 and q(768, 0, 16) == 0 and q(768, 33, 16) == 0
    assert q(7, 1, 1) > 0 and q(1024, 32, 64) > 0


def test_row_base_is_the_seed_times_the_inverse_of_the_hash_multiplier():
    from multimodalfusion_amd import _lib, ops
    rb = _lib.lib().mmf_dropout_row_base
    assert rb(0) == 0
    for seed in (1, 2, 0x9E3779B1, 0xFFFFFFFF, 123456789):
        assert (rb(seed) * 0x9E3779B1) & 0xFFFFFFFF == seed             # hash(key0, i + base) = mix(i * a + seed + key0)
        assert rb(seed) == (seed * ops._HASH_MUL_INV) & 0xFFFFFFFF
    # ... so the seed-0 key at index row_base + n draws what the key of seed_b draws at index n (the host restatement of
    # the device keep-hash)
    keep = _lib.lib().mmf_dropout_keep_host
    for seed in (1, 0x9E3779B1, 0xFFFFFFFF, 123456789):
        for site in (0, 1):
            a = [keep(0, site, (rb(seed) + n) & 0xFFFFFFFF, 0.25) for n in range(512)]
            b = [keep(seed, site, n, 0.25) for n in range(512)]
            assert a == b and 0 < sum(a) < 512


def test_refusals_that_need_no_device():
    """Null pointers and out-of-range shapes come back as error codes before any HIP call."""
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    ARG, SHAPE = -1, -2
    hd, tg = _lib.SurvHead(), _lib.NllTarget()
    assert l.mmf_surv_head_nll_step_group(None, 8, 8, 1, C.byref(hd), C.byref(tg), None, None, 0, None) == ARG
    fake = 4096                       # a non-null pointer that is never dereferenced: the shape checks come first
    assert l.mmf_surv_head_nll_step_group(fake, 1025, 1025, 1, C.byref(hd), C.byref(tg), fake, fake, 0, None) == SHAPE
    assert l.mmf_surv_head_nll_step_group(fake, 4, 8, 1, C.byref(hd), C.byref(tg), fake, fake, 0, None) == SHAPE   # ldf < F
    assert l.mmf_surv_head_nll_step_group(fake, 8, 8, 65, C.byref(hd), C.byref(tg), fake, fake, 0, None) == SHAPE
    assert l.mmf_surv_head_nll_step_group(fake, 8, 8, 1, C.byref(hd), C.byref(tg), fake, fake, 0, None) == ARG     # empty head
    assert l.mmf_dense_forward_rows(fake, fake, None, 2, 8, 8, 0, 0, 0.0, 0, None, None, fake, 8, None) == ARG     # no row_base
    assert l.mmf_dense_forward_rows(fake, fake, None, 2, 8, 8, 0, 0, 0.0, 0, None, fake, fake, 7, None) == SHAPE   # ldy < N
    assert l.mmf_dense_backward_rows(fake, 7, fake, 8, fake, fake, 2, 8, 8, 0, 0, 0.0, 0, None, fake, fake, None, fake,
                                     None, None) == SHAPE
    assert l.mmf_amil_group_forward(None, None, None, None, 0, None, 0, None, None) == ARG
    assert l.mmf_amil_group_backward(None, None, None, None, 0, None, 0, None, None, 0, None) == ARG
    assert l.mmf_radio_group_forward(None, None, None, None, 0, None, 0, None, None) == ARG
    assert l.mmf_radio_group_backward(None, None, None, None, 0, None, 0, None, None, 0, None) == ARG
    # a window the contract refuses: G = 65, then an empty bag, then ldm < H
    d = _lib.AmilDesc(N=65, L=1024, H=256, D=256, gated=0, W1=fake, b1=fake, Wa=fake, ba=fake, Wc=fake, bc=fake)
    seeds = (C.c_uint32 * 65)()
    offs = (C.c_int64 * 66)(*range(66))
    grp = _lib.BagGroup(G=65, offsets=offs, seeds=seeds)
    assert l.mmf_amil_group_forward(C.byref(d), C.byref(grp), fake, fake, 1 << 30, fake, 256, fake, None) == SHAPE
    d.N = 10
    grp = _lib.BagGroup(G=2, offsets=(C.c_int64 * 3)(0, 10, 10), seeds=seeds)
    assert l.mmf_amil_group_forward(C.byref(d), C.byref(grp), fake, fake, 1 << 30, fake, 256, fake, None) == SHAPE
    grp = _lib.BagGroup(G=2, offsets=(C.c_int64 * 3)(0, 4, 10), seeds=seeds)
    assert l.mmf_amil_group_forward(C.byref(d), C.byref(grp), fake, fake, 1 << 30, fake, 255, fake, None) == SHAPE
    d.gemm = 1
    assert l.mmf_amil_group_forward(C.byref(d), C.byref(grp), fake, fake, 1 << 30, fake, 256, fake, None) == ARG
