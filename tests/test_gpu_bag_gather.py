"""GPU: ops.bag_gather (mmf_bag_gather) -- the bags of a window, each somewhere in HBM, into the contiguous rows of one
matrix per plane in one launch, for the four storage pairs.  Every comparison is on the raw bits: the copies and the
widening are exact, and the one rounding step (fp32 -> bf16) is compared with torch's own conversion on the CPU; a NaN
must stay a NaN, whatever its payload."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
SIZES = [1, 63, 64, 65, 999, 1, 4097]
NAN_BITS = {F32: 0x7FC00BAD, BF16: 0x7FCB}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(got, want):
    """Bit equality, a NaN of `want` matched by any NaN."""
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(bits(got)[~nan], bits(want)[~nan]))


def poisoned(shape, dtype, device="cuda"):
    raw = torch.full(shape, NAN_BITS[dtype], dtype=torch.int32 if dtype == F32 else torch.int16, device=device)
    return raw.view(dtype)


def is_poison(t):
    return bool((bits(t) == NAN_BITS[t.dtype]).all())


def sources(sizes, L, dtype, seed):
    """One bag per size: every other one a view at an odd multiple of 16 bytes into a larger buffer, the rest
    allocated on their own."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        x = torch.randn(n, L, generator=g, device="cuda").to(dtype)
        if i % 2:
            shift = (2 * i + 1) * 16 // x.element_size()          # elements: an odd number of 16-byte units
            big = torch.empty(n * L + shift + 64, dtype=dtype, device="cuda")
            view = big[shift:shift + n * L].view(n, L)
            view.copy_(x)
            assert view.data_ptr() % 32 == 16
            x = view
        out.append(x)
    return out


def guarded(nplane, rows, L, dtype, spare=3, guard=2):
    buf = poisoned((nplane, guard + rows + spare + guard, L), dtype)
    return buf, [buf[m, guard:guard + rows + spare] for m in range(nplane)]


def check_guarded(buf, planes, rows, dtype, spare=3, guard=2):
    for m, p in enumerate(planes):
        want = torch.cat(p).to(dtype)
        assert torch.equal(bits(buf[m, guard:guard + rows]), bits(want)), m
        assert is_poison(buf[m, :guard]) and is_poison(buf[m, guard + rows:]), m     # guards and spare rows untouched


@pytest.mark.parametrize("nplane", [1, 4])
@pytest.mark.parametrize("sdt,ddt", PAIRS)
def test_parity_with_torch_cat(sdt, ddt, nplane):
    from multimodalfusion_amd import ops
    L, rows = 1024, sum(SIZES)
    planes = [sources(SIZES, L, sdt, 100 + m) for m in range(nplane)]
    buf, dst = guarded(nplane, rows, L, ddt)
    assert ops.bag_gather(planes, dst) == SIZES
    check_guarded(buf, planes, rows, ddt)
    again, dst2 = guarded(nplane, rows, L, ddt)
    ops.bag_gather(planes, dst2)
    assert torch.equal(bits(again), bits(buf))                     # deterministic: identical bytes


@pytest.mark.parametrize("sdt,ddt", PAIRS)
@pytest.mark.parametrize("sizes,nplane,L", [([3, 1, 2], 2, 8), ([1] * 64, 4, 1024), ([777], 1, 1024), ([5], 3, 40)])
def test_edges(sizes, nplane, L, sdt, ddt):
    """L = 8 (the smallest admitted), a full table (64 one-row bags x 4 planes), G = 1, and a width of 5 x 8."""
    from multimodalfusion_amd import ops
    planes = [sources(sizes, L, sdt, 200 + m) for m in range(nplane)]
    buf, dst = guarded(nplane, sum(sizes), L, ddt)
    ops.bag_gather(planes, dst)
    check_guarded(buf, planes, sum(sizes), ddt)


def test_a_3d_destination_and_refusals_reach_the_caller():
    from multimodalfusion_amd import _lib, ops
    x = [torch.randn(4, 64, device="cuda"), torch.randn(2, 64, device="cuda")]
    out = poisoned((2, 9, 64), F32)
    ops.bag_gather([x, x], out)
    assert torch.equal(out[0, :6], torch.cat(x)) and torch.equal(out[1, :6], torch.cat(x)) and is_poison(out[:, 6:])
    keep = out.clone()
    for planes, dst in [([x], [out[0, :5]]),                                  # too few rows
                        ([x], [out[0, :, :32]]),                              # another width
                        ([x] * 5, [out[0]] * 5),                              # five planes
                        ([[x[0][:, :12].contiguous()]], [torch.empty(4, 12, device="cuda")]),     # L % 8 != 0
                        ([[torch.randn(24, device="cuda")[1:17].view(2, 8)]],
                         [torch.empty(2, 8, device="cuda")])]:               # a source that is not 16-byte aligned
        with pytest.raises(_lib.MmfError):
            ops.bag_gather(planes, dst)
    assert torch.equal(bits(out), bits(keep))                                 # nothing was written


def _f32(words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).view(F32)


NARROW = {
    "zeros_inf": [0x00000000, 0x80000000, 0x7F800000, 0xFF800000],
    "denormals": [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00017FFF, 0x00018000, 0x007FFFFF, 0x807F8000,
                  0x80000001, 0x00010000, 0x007F7FFF, 0x007F8000],
    # within one bf16 ulp of a tie: the kept half even (0x3F80) and odd (0x3F81), both signs, a huge and a tiny exponent
    "ties": [hi << 16 | lo for hi in (0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x7F00, 0x7F01, 0x0080, 0x0081, 0x4000, 0x40FF)
             for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)],
    "largest": [0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F7F0000],
    "nans": [0x7F800001, 0x7FC00000, 0xFFC00000, 0xFFFFFFFF, 0x7F80FFFF, 0xFF800001, 0x7FFF8000, 0x7FBFFFFF],
}


def test_narrowing_rounds_as_torch_does():
    from multimodalfusion_amd import ops
    bags = []
    for name, words in NARROW.items():
        words = words + [words[-1]] * (-len(words) % 8)
        bags.append(_f32(words).view(-1, 8))
    want = torch.cat(bags).to(BF16)                                 # torch's conversion, on the CPU
    assert torch.isnan(want).sum() >= len(NARROW["nans"])
    out = poisoned((sum(b.shape[0] for b in bags) + 1, 8), BF16)
    ops.bag_gather([[b.cuda() for b in bags]], [out])
    got = out[:-1].cpu()
    for r0, (name, b) in zip(torch.tensor([0] + [b.shape[0] for b in bags]).cumsum(0).tolist(), zip(NARROW, bags)):
        assert same_bits(got[r0:r0 + b.shape[0]], want[r0:r0 + b.shape[0]]), name
    assert is_poison(out[-1:])
    # and the widening gives the same values back, bit for bit, NaNs included
    back = poisoned(tuple(got.shape), F32)
    ops.bag_gather([[out[:-1]]], [back])
    assert torch.equal(bits(back.cpu()), bits(got).to(torch.int32) << 16)


def test_a_source_beyond_4_gib_of_one_allocation():
    from multimodalfusion_amd import ops
    n, L = 65, 1024
    tail = n * L * 4
    free, _ = torch.cuda.mem_get_info()
    assert free > (5 << 30), "needs 5 GiB of free device memory"
    arena = torch.empty((1 << 32) + 4096 + tail, dtype=torch.uint8, device="cuda")
    src = arena[(1 << 32) + 4096:].view(F32).view(n, L)
    assert src.data_ptr() - arena.data_ptr() > 1 << 32
    front = arena[:2 * L * 4].view(F32).view(2, L)
    src.copy_(torch.randn(n, L, device="cuda"))
    front.fill_(-1.0)
    for ddt in (F32, BF16):
        out = poisoned((n + 2 + 1, L), ddt)
        ops.bag_gather([[front, src]], [out])
        assert torch.equal(bits(out[2:n + 2]), bits(src.to(ddt))) and bool((out[:2] == -1).all()) and is_poison(out[n + 2:])
    del arena
