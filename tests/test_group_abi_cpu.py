"""CPU checks of the grouped step's C ABI (include/mmf_amil.h: mmf_bag_group, mmf_amil_group_workspace_bytes): the ctypes
mirror lays its fields out as the header compiled as C does, and the workspace query accepts valid offset tables and
rejects (returns 0 for) invalid ones.  Needs the built library, not a GPU."""
import ctypes as C

from test_abi_layout_cpu import _c_layout


def test_bag_group_mirror_matches_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    m = _lib.BagGroup
    got = _c_layout(tmp_path, {"mmf_bag_group": [n for n, _ in m._fields_]})
    assert got[("mmf_bag_group", "sizeof")] == C.sizeof(m)
    for n, _ in m._fields_:
        assert got[("mmf_bag_group", n)] == getattr(m, n).offset, n


def _ws(offsets, G=None):
    from multimodalfusion_amd import _lib
    arr = (C.c_int64 * len(offsets))(*offsets)
    return _lib.lib().mmf_amil_group_workspace_bytes(arr, len(offsets) - 1 if G is None else G, 1024, 512, 256, 1)


def test_group_workspace_query_validates_offsets():
    from multimodalfusion_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.lib().mmf_abi_version() == 12
    one = _ws([0, 1000])
    sixteen = _ws([1000 * i for i in range(17)])
    assert 0 < one < sixteen
    assert _ws([0, 1, 1000, 5097, 15097]) > 0
    assert _ws([0] + [1] * 64, G=64) == 0               # empty bags
    assert _ws(list(range(65))) > 0                      # 64 one-row bags
    assert _ws(list(range(66))) == 0                     # G = 65
    assert _ws([0, 10, 5]) == 0                          # decreasing
    assert _ws([3, 10, 20]) == 0                         # offsets[0] != 0
    assert _ws([0, 10], G=0) == 0
    assert _lib.lib().mmf_amil_group_workspace_bytes(None, 1, 1024, 512, 256, 1) == 0
