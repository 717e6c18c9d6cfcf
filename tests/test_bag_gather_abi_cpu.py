"""CPU checks of mmf_bag_gather in the C ABI (include/mmf_amil.h "Bag feed"): every refusal the header lists comes back
as its error code before any HIP call (the pointers are fake 16-byte-aligned addresses that are never dereferenced, so a
call that got as far as a launch would not return one of these codes on a machine without a GPU), where several checks
fail the code that wins is pinned, the prototype has the arity its binding declares, and the ABI version is unchanged
(the entry point is additive).  Needs the built library, not a GPU."""
import ctypes as C
import re

import pytest

from test_abi_contract_cpu import ALIGN, ARG, SHAPE, fake
from test_abi_layout_cpu import HEADER

GROUP_MAX = 64


def call(sizes=(3, 1, 5), nplane=1, L=1024, src=True, dst=True, offsets=True, sb=0, db=0, G=None, bad_src=None,
         bad_dst=None):
    """mmf_bag_gather on fake pointers.  offsets: True (from sizes), None, or a list; bad_src / bad_dst: (index, value)."""
    from multimodalfusion_amd import _lib
    G = len(sizes) if G is None else G
    if offsets is True:
        offsets = [0]
        for n in sizes:
            offsets.append(offsets[-1] + n)
    offs = (C.c_int64 * len(offsets))(*offsets) if offsets is not None else None
    n_src = max(nplane, 1) * max(len(sizes), 1)
    s = (C.c_void_p * n_src)(*[fake() for _ in range(n_src)]) if src else None
    d = (C.c_void_p * max(nplane, 1))(*[fake() for _ in range(max(nplane, 1))]) if dst else None
    if bad_src is not None:
        s[bad_src[0]] = bad_src[1]
    if bad_dst is not None:
        d[bad_dst[0]] = bad_dst[1]
    return _lib.lib().mmf_bag_gather(offs, G, nplane, s, d, L, sb, db, None)


def test_the_symbol_is_bound_with_the_headers_arity_and_the_abi_version_is_unchanged():
    from multimodalfusion_amd import _lib
    l = _lib.lib()
    assert _lib.ABI_VERSION == 12 and l.mmf_abi_version() == 12
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "mmf_bag_gather" in _lib.SYMBOLS and hasattr(l, "mmf_bag_gather")
    m = re.search(r"\bmmf_bag_gather\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "mmf_bag_gather is not declared in the header"
    assert len(m.group(1).split(",")) == len(_lib.SYMBOLS["mmf_bag_gather"][1]) == 9


def test_null_pointers():
    assert call(offsets=None) == ARG
    assert call(src=None) == ARG
    assert call(dst=None) == ARG
    assert call(bad_src=(1, None)) == ARG
    assert call(nplane=4, bad_src=(11, None)) == ARG              # the last entry of a full [4 x 3] table
    assert call(nplane=2, bad_dst=(1, None)) == ARG
    assert call(bad_src=(0, None), bad_dst=(0, fake() + 4)) == ARG      # null before alignment


@pytest.mark.parametrize("sb,db", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_shapes(sb, db):
    kw = dict(sb=sb, db=db)
    assert call(sizes=(), G=0, offsets=[0], **kw) == SHAPE
    assert call(sizes=(1,) * (GROUP_MAX + 1), **kw) == SHAPE
    assert call(G=-1, **kw) == SHAPE
    for nplane in (0, 5, -1):
        assert call(nplane=nplane, **kw) == SHAPE
    assert call(sizes=(3, 0, 5), **kw) == SHAPE                      # an empty bag
    assert call(offsets=[0, 3, 2, 9], **kw) == SHAPE                 # decreasing
    assert call(offsets=[1, 4, 5, 10], **kw) == SHAPE                # not from 0
    for L in (0, 4, 12, 1028, -8):
        assert call(L=L, **kw) == SHAPE                              # 16 bytes of the narrower type: L % 8 == 0
    assert call(L=1028, bad_src=(0, fake() + 4), **kw) == SHAPE      # shape before alignment


def test_alignment():
    for off in (2, 4, 8):
        assert call(bad_src=(2, fake() + off)) == ALIGN
        assert call(nplane=4, bad_src=(7, fake() + off), sb=1) == ALIGN
        assert call(nplane=3, bad_dst=(2, fake() + off), db=1) == ALIGN
