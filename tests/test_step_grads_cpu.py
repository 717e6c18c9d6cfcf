"""The gradient-destination helpers every one-call step uses (models/model_modules.py), driven with CPU tensors:
step_grad_buffers for the steps whose kernels write or accumulate in place, hand_over_grads for the composed steps."""
import pytest
import torch

from multimodalfusion_amd import ops
from multimodalfusion_amd.models.model_modules import hand_over_grads, make_amil_stack, stack_args, step_grad_buffers


def _params(*shapes):
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s)) for s in shapes]


@pytest.fixture
def allocs(monkeypatch):
    """Records which of torch.empty / torch.zeros the helper allocates with."""
    seen = []
    for name in ("empty", "zeros"):
        real = getattr(torch, name)
        monkeypatch.setattr(torch, name, lambda *a, _n=name, _f=real, **k: seen.append(_n) or _f(*a, **k))
    return seen


def _kernel(dests, step, accumulate):
    """What the in-place kernels do with the destinations."""
    for d, g in zip(dests, step):
        if d is not None:
            d.add_(g) if accumulate else d.copy_(g)


def test_all_grads_missing_write_into_one_empty_buffer(allocs):
    ps = _params((3, 4), (3,), (2, 3))
    params = [ps[0], None, ps[1], ps[2]]
    dests, acc = step_grad_buffers(params, "cpu", None, None)
    assert acc is False and allocs == ["empty"]
    assert dests[1] is None
    assert [d is p.grad for d, p in zip(dests, params) if p is not None] == [True] * 3
    assert all(p.grad.shape == p.shape and p.grad.dtype == torch.float32 for p in ps)
    base = ps[0].grad.untyped_storage().data_ptr()
    assert all(p.grad.untyped_storage().data_ptr() == base for p in ps)      # slices of one flat buffer
    step = [torch.randn(p.shape) if p is not None else None for p in params]
    _kernel(dests, step, acc)
    for p, g in zip(params, step):
        if p is not None:
            assert torch.equal(p.grad, g)


def test_some_grads_set_are_added_to_and_missing_ones_zero_filled(allocs):
    ps = _params((3, 4), (3,), (2, 3))
    old = torch.randn(3)
    ps[1].grad = old.clone()
    kept = ps[1].grad
    dests, acc = step_grad_buffers(ps, "cpu", None, False)
    assert acc is True and allocs == ["zeros"]
    assert dests[1] is kept
    assert torch.count_nonzero(ps[0].grad) == 0 and torch.count_nonzero(ps[2].grad) == 0
    step = [torch.randn(p.shape) for p in ps]
    _kernel(dests, step, acc)
    assert torch.equal(ps[0].grad, step[0]) and torch.equal(ps[2].grad, step[2])
    assert torch.allclose(ps[1].grad, old + step[1])


@pytest.mark.parametrize("accumulate", [False, True, None])
def test_grad_out_is_used_as_given(allocs, accumulate):
    ps = _params((3, 4), (3,))
    out = [torch.full((3, 4), 2.0), torch.full((3,), 2.0)]
    dests, acc = step_grad_buffers([ps[0], None, ps[1]], "cpu", iter(out), accumulate)
    assert acc is bool(accumulate) and allocs == []
    assert dests[0] is out[0] and dests[1] is None and dests[2] is out[1]
    assert all(p.grad is None for p in ps)


@pytest.mark.parametrize("accumulate", [False, True])
def test_hand_over_to_grad_out(accumulate):
    ps = _params((3, 4), (3,), (5,))
    out = [torch.full(p.shape, 2.0) for p in ps]
    g0, g2 = torch.randn(3, 4), torch.randn(5)
    hand_over_grads(ps, {ps[0]: g0, ps[2]: g2}, out, accumulate)
    assert torch.equal(out[0], 2.0 + g0 if accumulate else g0)
    assert torch.equal(out[2], 2.0 + g2 if accumulate else g2)
    assert torch.equal(out[1], torch.full((3,), 0.0 if not accumulate else 2.0))   # took no part
    assert all(p.grad is None for p in ps)


def test_hand_over_to_grad(monkeypatch):
    ps = _params((3, 4), (3,), (5,), (2,))
    old = torch.randn(3)
    ps[1].grad = old.clone()
    kept = ps[1].grad
    g0, g1, g2 = torch.randn(3, 4), torch.randn(3), torch.randn(5)
    calls = []
    real = torch._foreach_add_
    monkeypatch.setattr(torch, "_foreach_add_", lambda d, s: calls.append(len(d)) or real(d, s))
    hand_over_grads(ps, {ps[0]: g0, ps[1]: g1, ps[2]: g2}, None, None)
    assert ps[0].grad is g0 and ps[2].grad is g2                     # a fresh .grad is the very tensor, no copy
    assert ps[1].grad is kept and torch.allclose(kept, old + g1)      # a set .grad is added to
    assert ps[3].grad is None                                         # took no part
    assert calls == [1]


def test_hand_over_with_every_grad_missing_adds_nothing(monkeypatch):
    ps = _params((3,), (4,))
    monkeypatch.setattr(torch, "_foreach_add_", lambda d, s: pytest.fail("nothing to add to"))
    g = {p: torch.randn(p.shape) for p in ps}
    hand_over_grads(ps, g, None, None)
    assert all(p.grad is g[p] for p in ps)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("att_dropout", [True, False])
def test_stack_args(gated, training, att_dropout):
    seq = make_amil_stack("small", gated=gated, att_dropout=att_dropout)
    before = ops._drop_calls
    g, stack, p_h, p_att = stack_args(seq, training)
    assert ops._drop_calls == before                                  # the caller draws the seed
    assert g is gated
    live = [p for p in stack if p is not None]
    assert len(live) == len(list(seq.parameters())) and all(a is b for a, b in zip(live, seq.parameters()))
    assert (stack[4] is None) == (not gated) and (stack[5] is None) == (not gated)
    assert p_h == (0.25 if training else 0.0)
    assert p_att == (0.25 if training and att_dropout else 0.0)
