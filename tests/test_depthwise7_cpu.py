"""ops/depthwise7.py on the CPU: the module is a drop-in nn.Conv2d, the
fallback is F.conv2d, the grad_slot path leaves the unfused gradients, the
feature switch is known -- and the fp64 references of tests/exact_ref_dw7.py
(the GPU tests' yardstick) agree with PyTorch autograd."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import depthwise7 as D7
from distributed_model_parallel_amd.ops.fused import GradSlot, grad_tap
from tests import exact_ref_dw7 as R


def test_module_is_a_drop_in_conv2d():
    conv = D7.DepthwiseConv7x7(16)
    ref = nn.Conv2d(16, 16, 7, padding=3, groups=16, bias=True)
    assert isinstance(conv, nn.Conv2d)
    assert list(conv.state_dict()) == list(ref.state_dict()) == ["weight", "bias"]
    assert {k: v.shape for k, v in conv.state_dict().items()} == {k: v.shape for k, v in ref.state_dict().items()}
    ref.load_state_dict(conv.state_dict())
    x = torch.randn(2, 16, 9, 5)
    t0 = D7._STATS["torch"]
    assert torch.equal(conv(x), ref(x))
    assert D7._STATS["torch"] == t0 + 1
    assert torch.equal(D7.depthwise_conv7x7(x, conv.weight, conv.bias),
                       F.conv2d(x, conv.weight, conv.bias, 1, 3, 1, 16))
    assert torch.equal(D7.depthwise_conv7x7(x, conv.weight), F.conv2d(x, conv.weight, None, 1, 3, 1, 16))


def test_grad_slot_on_cpu_leaves_the_unfused_sum():
    """No native consumer registers on the CPU: the tap passes its gradient on
    and autograd sums both branches as usual."""
    torch.manual_seed(0)
    conv = D7.DepthwiseConv7x7(8)
    x = torch.randn(2, 8, 6, 7, requires_grad=True)
    gy, gr = torch.randn(2, 8, 6, 7), torch.randn(2, 8, 6, 7)
    slot = GradSlot()
    y = conv(x, slot)
    assert not slot.consumer
    res = grad_tap(x, slot)
    ((y * gy).sum() + (res * gr).sum()).backward()
    got = x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()
    x.grad = conv.weight.grad = conv.bias.grad = None
    ((F.conv2d(x, conv.weight, conv.bias, 1, 3, 1, 8) * gy).sum() + (x * gr).sum()).backward()
    for a, b in zip(got, (x.grad, conv.weight.grad, conv.bias.grad)):
        assert torch.equal(a, b)
    assert slot.grad is None


def test_feature_switch_is_known():
    assert "dwconv7" in _native.FEATURES
    assert _native.disabled("dwconv7") in (False, True)
    D7.set_enabled(False)
    assert D7._ENABLED is False
    D7.set_enabled(True)
    assert D7._ENABLED is True


@pytest.mark.parametrize("n,c,h,w", [(2, 3, 1, 1), (1, 2, 3, 9), (2, 4, 7, 7), (1, 3, 10, 8)])
def test_fp64_references_agree_with_autograd(n, c, h, w):
    torch.manual_seed(1)
    x = torch.randn(n, c, h, w, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(c, 1, 7, 7, dtype=torch.float64, requires_grad=True)
    b = torch.randn(c, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(n, c, h, w, dtype=torch.float64)
    add = torch.randn(n, c, h, w, dtype=torch.float64)
    y = F.conv2d(x, wt, b, 1, 3, 1, c)
    y.backward(dy)
    tol = dict(atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(R.forward(x.detach(), wt.detach(), b.detach()), y.detach(), **tol)
    torch.testing.assert_close(R.forward(x.detach(), wt.detach()), F.conv2d(x, wt, None, 1, 3, 1, c).detach(), **tol)
    torch.testing.assert_close(R.dgrad(dy, wt.detach()), x.grad, **tol)
    torch.testing.assert_close(R.dgrad(dy, wt.detach(), add), x.grad + add, **tol)
    dw, db = R.wgrad(dy, x.detach())
    torch.testing.assert_close(dw, wt.grad, **tol)
    torch.testing.assert_close(db, b.grad, **tol)
    # the absolute-value stencils bound the plain ones
    assert bool((R.forward_abs(x.detach(), wt.detach(), b.detach()) >= y.detach().abs() - 1e-12).all())
    assert bool((R.dgrad_abs(dy, wt.detach(), add) >= (x.grad + add).abs() - 1e-12).all())
    tw, tb = R.wgrad_abs(dy, x.detach())
    assert bool((tw >= dw.abs() - 1e-12).all()) and bool((tb >= db.abs() - 1e-12).all())
