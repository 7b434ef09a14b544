"""CPU checks of the weight-gradient operand hand-off in ops/linear.py: a producer kernel may attach
the transposed copy of its output (``_grt_T``, ops.fused.swiglu); the consuming projection takes it
exactly once and only when it is the [C, M] transpose of the 2-D view it needs."""
import pytest
import torch

from gke_ray_train_amd.models.llama import _direct_wgrad
from gke_ray_train_amd.ops import linear as L


def test_provided_transposed_is_taken_once_and_shape_checked():
    t = torch.randn(2, 64, 128).bfloat16()
    t2 = t.reshape(-1, 128)
    t._grt_T = t2.t().contiguous()
    got = L.provided_transposed(t2, t)
    assert got is not None and torch.equal(got, t2.t())
    assert not hasattr(t, "_grt_T") and L.provided_transposed(t2, t) is None  # consumed
    t._grt_T = torch.empty(64, 128, dtype=torch.bfloat16)  # not [C, M]
    assert L.provided_transposed(t2, t) is None and not hasattr(t, "_grt_T")
    u = torch.randn(100, 128).bfloat16()  # M not a multiple of 64: the TN path does not apply
    u._grt_T = u.t().contiguous()
    assert L.provided_transposed(u, u) is None
    v = torch.randn(128, 128)  # fp32
    v._grt_T = v.t().contiguous()
    assert L.provided_transposed(v, v) is None


def test_grad_slot_protocol_on_cpu():
    """The whole GradSlot protocol with a hand-attached slot: the backward GEMM overwrites the
    (NaN-filled) view on the first micro-step and accumulates on the second, announces the
    parameter once per backward, and leaves nothing for autograd; fold / grad_slot / a failing
    writer behave as the engines and ops rely on."""
    g = torch.Generator().manual_seed(3)
    lin = L.Linear(128, 64, bias=False)
    w = lin.weight
    fired = []
    slot = w._grt_slot = L.GradSlot(torch.full((64, 128), float("nan")), fired.append)
    x = torch.randn(3, 40, 128, generator=g)
    dys = [torch.randn(3, 40, 64, generator=g) for _ in range(2)]
    assert slot.fresh and not slot.accumulate
    for n, dy in enumerate(dys, 1):
        lin(x.clone().requires_grad_()).backward(dy)
        assert len(fired) == n and fired[-1] is w
        assert slot.direct and not slot.fresh and slot.accumulate
    ref = sum(dy.reshape(-1, 64).t() @ x.reshape(-1, 128) for dy in dys)
    assert torch.allclose(slot.view, ref, rtol=0, atol=1e-4)
    assert w.grad is None and slot.fresh is False
    assert slot.consume_direct() and not slot.consume_direct()

    # AccumulateGrad side: copy into a fresh slot, add onto a written one, skip the view itself
    grad = torch.randn(64, 128, generator=g)
    sl = L.GradSlot(torch.full((64, 128), float("nan")), fired.append)
    sl.fold(grad)
    assert torch.equal(sl.view, grad) and sl.fresh is False and not sl.direct
    sl.fold(grad)
    assert torch.equal(sl.view, 2 * grad)
    sl.fold(sl.view)
    assert torch.equal(sl.view, 2 * grad)
    assert len(fired) == 2  # fold announces nothing: the engine's hook does

    # lookup: trainable parameters only; match_dtype refuses a view of another dtype
    assert L.grad_slot(w) is slot and L.grad_slot(w, match_dtype=True) is slot
    assert L.grad_slot(L.Linear(8, 8).weight) is None
    wb = torch.nn.Parameter(torch.zeros(4, 4, dtype=torch.bfloat16))
    wb._grt_slot = L.GradSlot(torch.zeros(4, 4), fired.append)  # fp32 gradient buffer
    assert L.grad_slot(wb) is wb._grt_slot and L.grad_slot(wb, match_dtype=True) is None
    w.requires_grad_(False)
    assert L.grad_slot(w) is None and L.grad_slot(w, match_dtype=True) is None

    # a writer that fails leaves the slot as it was: still fresh, nothing announced
    sl = L.GradSlot(torch.zeros(2, 2), fired.append)

    def boom(view, accumulate):
        raise RuntimeError("kernel refused")
    with pytest.raises(RuntimeError):
        sl.write(wb, boom)
    assert sl.fresh is True and sl.direct is False and len(fired) == 2


def test_direct_wgrad_needs_a_trainable_slotted_device_weight():
    lin = L.Linear(128, 64, bias=False)
    assert not _direct_wgrad(lin)  # CPU weight, no gradient slot
    lin.weight._grt_slot = L.GradSlot(torch.empty(64, 128), lambda p: None)
    assert not _direct_wgrad(lin)  # still a CPU weight
    lin.weight.requires_grad_(False)
    assert not _direct_wgrad(lin)
