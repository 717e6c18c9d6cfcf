"""CPU checks of the radiology head's grouped step in the C ABI (include/mmf_amil.h: mmf_radio_reduce,
mmf_radio_group_workspace_bytes): the ctypes mirror lays its fields out as the header compiled as C does, the workspace
query accepts valid offset tables and modality counts and returns 0 for invalid ones, and the ABI version is unchanged
(the entry point is additive).  Needs the built library, not a GPU."""
import ctypes as C

from test_abi_layout_cpu import _c_layout


def test_radio_reduce_mirror_matches_the_c_header(tmp_path):
    from multimodalfusion_amd import _lib
    m = _lib.RadioReduce
    got = _c_layout(tmp_path, {"mmf_radio_reduce": [n for n, _ in m._fields_]})
    assert got[("mmf_radio_reduce", "sizeof")] == C.sizeof(m)
    for n, _ in m._fields_:
        assert got[("mmf_radio_reduce", n)] == getattr(m, n).offset, n


def _ws(offsets, G=None, nseg=4):
    from multimodalfusion_amd import _lib
    arr = (C.c_int64 * len(offsets))(*offsets)
    return _lib.lib().mmf_radio_group_workspace_bytes(arr, len(offsets) - 1 if G is None else G, nseg, 1024, 512, 256, 1)


def test_radio_group_workspace_query_validates_offsets_and_modalities():
    from multimodalfusion_amd import _lib
    one = _ws([0, 512])
    sixteen = _ws([512 * i for i in range(17)])
    assert 0 < one < sixteen
    assert _ws([0, 1, 18, 118, 451]) > 0
    assert _ws([0, 1, 18, 118, 451], nseg=2) > 0
    # more than the stack's workspace: reduce_dim's output and its gradient live there too
    stack = _lib.lib().mmf_amil_group_workspace_bytes((C.c_int64 * 2)(0, 512), 1, 1024, 512, 256, 1)
    assert one > stack + 2 * 512 * 1024 * 4
    assert _ws([0] + [1] * 64, G=64) == 0               # empty bags
    assert _ws(list(range(65))) > 0                      # 64 one-row bags
    assert _ws(list(range(66))) == 0                     # G = 65
    assert _ws([0, 10, 5]) == 0                          # decreasing
    assert _ws([3, 10, 20]) == 0                         # offsets[0] != 0
    assert _ws([0, 10], G=0) == 0
    assert _ws([0, 10], nseg=1) == 0 and _ws([0, 10], nseg=5) == 0
    assert _lib.lib().mmf_radio_group_workspace_bytes(None, 1, 4, 1024, 512, 256, 1) == 0


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    from multimodalfusion_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.lib().mmf_abi_version() == 12
    assert "mmf_radio_nll_step_group" in _lib.SYMBOLS and "mmf_radio_group_workspace_bytes" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "mmf_radio_nll_step_group")
