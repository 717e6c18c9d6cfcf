"""GPU: the routes that merge one bag's pooling partials and run the hazard head agree to the bit.  The per-bag merge
(bag_merge in csrc/mmf_amil_fwd.hip) runs in group_tail_kernel (ops.amil_nll_step_group), group_merge_kernel
(ops._group_half_fwd_raw) and group_infer_tail_kernel (ops.amil_infer_group) and shares its order of additions with
pool_merge_kernel (ops.amil_infer); the hazard head (head_tail) runs behind it in the first and the third and alone in
surv_head_group_kernel (ops.surv_head_nll_step_group).  Dropout is off and loss_scale is 1, so every route runs the same
projection, gate and pooling-partial kernels in front: whatever differs, differs in the tails.

The window [1, 64, 65, 700, 2200] gives 64-row partial groups and bags of 1, 1, 2, 11 and 35 partials: a single partial,
a ragged last group, and more than 32 partials (the interleaved-slice loop takes a second step).  H = 1024: every one of
the 1024 threads owns a column."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_path import DEV

pytestmark = pytest.mark.gpu

L, D, K = 64, 128, 4
SIZES = [1, 64, 65, 700, 2200]
ALPHA = 0.15
HEADS = [(256, True), (256, False), (1024, True)]


def _weights(H, gated, seed=7):
    g = torch.Generator().manual_seed(seed + H + int(gated))

    def rn(*shape, scale):
        return (torch.randn(*shape, generator=g) * scale).to(DEV)

    stack = (rn(H, L, scale=L ** -0.5), rn(H, scale=0.02), rn(D, H, scale=H ** -0.5), rn(D, scale=0.02),
             rn(D, H, scale=H ** -0.5), rn(D, scale=0.02), rn(1, D, scale=4 * D ** -0.5), rn(1, scale=0.02))
    return stack, rn(K, H, scale=H ** -0.5), rn(K, scale=0.02)


def _rows(n, seed):
    return torch.randn(n, L, generator=torch.Generator().manual_seed(seed)).to(DEV)


@functools.lru_cache(maxsize=None)
def _window(H, gated):
    """Every route once over the same window; the tests below only compare."""
    from multimodalfusion_amd import ops
    stack, Wk, bk = _weights(H, gated)
    x = _rows(sum(SIZES), 11)
    G = len(SIZES)
    Y = torch.tensor([(g + 1) % K for g in range(G)])
    c = torch.tensor([float(g % 2) for g in range(G)])
    out = {}
    M_half = torch.empty((G, H), dtype=torch.float32, device=DEV)
    A_half, _ = ops._group_half_fwd_raw([x], SIZES, stack, gated, 0.0, 0.0, None, M_half)
    out["half"] = dict(M=M_half, A=A_half)
    _, _, _, _, A, M, _ = ops.amil_infer_group(x, SIZES, stack, gated, want_M=True)
    out["infer_M"] = dict(M=M, A=A)
    hz, S, Yh, risk, A, M, loss = ops.amil_infer_group(x, SIZES, stack, gated, Wk, bk, Y, c, alpha=ALPHA, want_M=True)
    out["infer"] = dict(M=M, A=A, hazards=hz, S=S, Y_hat=Yh, risk=risk, loss=loss)
    grads = tuple(torch.empty_like(t) for t in (*stack, Wk, bk))
    hz, S, Yh, A, loss, risk = ops.amil_nll_step_group(x, SIZES, stack, Wk, bk, gated, Y, c, ALPHA, grads, loss_scale=1.0)
    out["step"] = dict(A=A, hazards=hz, S=S, Y_hat=Yh, risk=risk, loss=loss, dWk=grads[8], dbk=grads[9])
    dWk, dbk = torch.empty_like(Wk), torch.empty_like(bk)
    hz, S, Yh, loss, risk, _ = ops.surv_head_nll_step_group(M_half, Wk, bk, Y, c, ALPHA, dWk, dbk, loss_scale=1.0)
    out["head"] = dict(hazards=hz, S=S, Y_hat=Yh, risk=risk, loss=loss, dWk=dWk, dbk=dbk)
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, what
    print(f"{what}: max |a - b| = {float((a.double() - b.double()).abs().max()):.3e}")
    assert torch.equal(a, b), what


@pytest.mark.parametrize("H,gated", HEADS)
def test_merge_kernel_and_infer_tail_give_the_same_M(H, gated):
    w = _window(H, gated)
    for other in ("infer_M", "infer"):
        _same(w["half"]["M"], w[other]["M"], f"M: group_merge_kernel vs group_infer_tail_kernel ({other})")
        for g, (a, b) in enumerate(zip(w["half"]["A"], w[other]["A"])):
            _same(a, b, f"A_raw of bag {g} ({other})")


@pytest.mark.parametrize("H,gated", HEADS)
def test_the_three_heads_give_the_same_hazards_and_loss(H, gated):
    w = _window(H, gated)
    for name in ("hazards", "S", "Y_hat", "risk", "loss"):
        _same(w["step"][name], w["infer"][name], f"{name}: group_tail_kernel vs group_infer_tail_kernel")
        _same(w["step"][name], w["head"][name], f"{name}: group_tail_kernel vs surv_head_group_kernel")
    for name in ("dWk", "dbk"):
        _same(w["step"][name], w["head"][name], f"{name}: group_tail_kernel vs surv_head_group_kernel")


@pytest.mark.parametrize("N", [640, 2240])
@pytest.mark.parametrize("H,gated", HEADS)
def test_one_bag_window_matches_pool_merge_kernel(H, gated, N):
    """Both routes cut N rows into the same 64-row partial groups (10 / 35): the per-bag merge against
    pool_merge_kernel's order of additions."""
    from multimodalfusion_amd import ops
    stack, _, _ = _weights(H, gated)
    x = _rows(N, 13 + N)
    M1, A1 = ops.amil_infer(x, *stack, gated)
    _, _, _, _, A, M, _ = ops.amil_infer_group(x, [N], stack, gated, want_M=True)
    _same(M1, M, "M: pool_merge_kernel vs group_infer_tail_kernel")
    _same(A1, A[0], "A_raw")


def test_bf16_one_bag_window_matches_the_one_bag_pass():
    """bf16, ungated H = 256: pool_partial_bf16_kernel and group_pool_partial_bf16_kernel run one body."""
    from multimodalfusion_amd import ops
    assert ops.infer_group_takes_bf16(False, 256, D)
    stack, _, _ = _weights(256, False)
    x = _rows(640, 17).to(torch.bfloat16)
    M1, A1 = ops.amil_infer(x, *stack, False)
    _, _, _, _, A, M, _ = ops.amil_infer_group(x, [640], stack, False, want_M=True)
    _same(M1, M, "M: bf16 one-bag pass vs bf16 window of one bag")
    _same(A1, A[0], "A_raw (bf16)")
