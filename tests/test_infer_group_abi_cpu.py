"""CPU checks of the grouped forward-only pass in the C ABI (include/mmf_amil.h: mmf_amil_group_infer_workspace_bytes,
mmf_radio_group_infer_workspace_bytes, mmf_amil_infer_group, mmf_radio_infer_group): the workspace queries accept valid
offset tables and return 0 for invalid ones, a bf16 window's workspace is at least an fp32 one's, the symbols are bound
and the ABI version is unchanged (the entry points are additive).  Needs the built library, not a GPU."""
import ctypes as C

import pytest


def _amil_ws(offsets, G=None, bf16=0, L=1024, H=512, D=384, gated=1):
    from multimodalfusion_amd import _lib
    arr = None if offsets is None else (C.c_int64 * len(offsets))(*offsets)
    n = (len(offsets) - 1 if offsets is not None else 1) if G is None else G
    return _lib.lib().mmf_amil_group_infer_workspace_bytes(arr, n, L, H, D, gated, bf16)


def _radio_ws(offsets, G=None, nseg=4):
    from multimodalfusion_amd import _lib
    arr = None if offsets is None else (C.c_int64 * len(offsets))(*offsets)
    n = (len(offsets) - 1 if offsets is not None else 1) if G is None else G
    return _lib.lib().mmf_radio_group_infer_workspace_bytes(arr, n, nseg, 1024, 256, 256, 1)


@pytest.mark.parametrize("query", [lambda o, G=None: _amil_ws(o, G), lambda o, G=None: _amil_ws(o, G, bf16=1),
                                   lambda o, G=None: _radio_ws(o, G)], ids=["fp32", "bf16", "radio"])
def test_workspace_queries_validate_offsets(query):
    one = query([0, 512])
    sixteen = query([512 * i for i in range(17)])
    assert 0 < one < sixteen
    assert query([0, 1, 18, 118, 451]) > 0
    assert query([0] + [1] * 64, G=64) == 0               # empty bags
    assert query(list(range(65))) > 0                      # 64 one-row bags
    assert query(list(range(66))) == 0                     # G = 65
    assert query([0, 10, 5]) == 0                          # decreasing
    assert query([3, 10, 20]) == 0                         # offsets[0] != 0
    assert query([0, 10], G=0) == 0
    assert query(None) == 0


def test_radio_query_refuses_modality_counts_outside_2_to_4():
    assert _radio_ws([0, 10], nseg=2) > 0
    assert _radio_ws([0, 10], nseg=1) == 0 and _radio_ws([0, 10], nseg=5) == 0


@pytest.mark.parametrize("offsets", [[0, 1], [0, 512], [0, 1000, 2000, 2064], [0, 63, 127, 191, 319, 10319],
                                     [10000 * i for i in range(5)], list(range(65))])
@pytest.mark.parametrize("gated,H,D", [(1, 256, 256), (0, 256, 256), (1, 512, 384)])
def test_bf16_workspace_is_at_least_the_fp32_one(offsets, gated, H, D):
    f32 = _amil_ws(offsets, H=H, D=D, gated=gated)
    b16 = _amil_ws(offsets, H=H, D=D, gated=gated, bf16=1)
    assert f32 > 0 and b16 >= f32


def test_forward_only_workspace_is_smaller_than_the_training_one():
    from multimodalfusion_amd import _lib
    offs = [1000 * i for i in range(17)]
    arr = (C.c_int64 * len(offs))(*offs)
    train = _lib.lib().mmf_amil_group_workspace_bytes(arr, 16, 1024, 256, 256, 1)
    assert 0 < _amil_ws(offs, H=256, D=256) < train


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    from multimodalfusion_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.lib().mmf_abi_version() == 12
    for name in ("mmf_amil_group_infer_workspace_bytes", "mmf_amil_infer_group",
                 "mmf_radio_group_infer_workspace_bytes", "mmf_radio_infer_group"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name


def test_row_limits():
    from multimodalfusion_amd import ops
    assert ops.infer_group_row_limit(1024, 256, 256) == ops.group_row_limit(1024, 256, 256)
    # a bf16 window's [sum N x *] operands are two bytes wide: twice the rows of the fp32 operand bound
    assert ops.infer_group_row_limit(1024, 256, 256, bf16=True) == 2 * ops.group_row_limit(1024, 256, 256) + 1
    assert ops.radio_infer_group_row_limit(4, 1024, 256, 256) == ops.radio_group_row_limit(4, 1024, 256, 256)
