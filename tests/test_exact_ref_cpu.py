"""tests/exact_ref.py against PyTorch autograd in fp64 on the CPU, so that the
references the GPU edge tests trust are known to be right without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_ref as R

# stride 2 on odd and even sizes, H = 1, W = 1, every W % 4 remainder
DW_GEOS = [(2, 8, 1, 1), (2, 8, 1, 5), (1, 8, 4, 1), (2, 8, 2, 3), (2, 8, 5, 7), (1, 16, 8, 9), (1, 8, 9, 4),
           (1, 8, 7, 62)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n,c,h,w", DW_GEOS)
def test_depthwise_refs_match_conv2d_autograd(n, c, h, w, stride):
    torch.manual_seed(0)
    x = torch.randn(n, c, h, w, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wt, None, stride, 1, 1, c)
    assert y.shape[2:] == (R.dw_out(h, stride), R.dw_out(w, stride))
    dy = torch.randn_like(y)
    y.backward(dy)
    torch.testing.assert_close(R.dw_forward(x.detach(), wt.detach(), stride), y.detach(), atol=1e-13, rtol=1e-13)
    torch.testing.assert_close(R.dw_dgrad(dy, wt.detach(), stride, h, w), x.grad, atol=1e-13, rtol=1e-13)
    torch.testing.assert_close(R.dw_wgrad(dy, x.detach(), stride), wt.grad, atol=1e-12, rtol=1e-13)
    # the |.|-sums are the same convolutions of the absolute values and bound the plain ones
    ya = R.dw_forward_abs(x.detach(), wt.detach(), stride)
    torch.testing.assert_close(ya, F.conv2d(x.detach().abs(), wt.detach().abs(), None, stride, 1, 1, c),
                               atol=1e-13, rtol=1e-13)
    assert bool((ya >= y.detach().abs() - 1e-13).all())
    assert bool((R.dw_dgrad_abs(dy, wt.detach(), stride, h, w) >= x.grad.abs() - 1e-13).all())
    assert bool((R.dw_wgrad_abs(dy, x.detach(), stride) >= wt.grad.abs() - 1e-12).all())


def test_depthwise_refs_are_exact_on_integers():
    torch.manual_seed(1)
    x = torch.randint(-3, 4, (2, 8, 5, 6)).double()
    wt = torch.randint(-3, 4, (8, 1, 3, 3)).double()
    for stride in (1, 2):
        y = R.dw_forward(x, wt, stride)
        assert torch.equal(y, F.conv2d(x, wt, None, stride, 1, 1, 8)) and bool((y == y.round()).all())
        assert float(y.abs().max()) <= 81


POOL_GEOS = [((2, 4, 7, 9), 3, 2, 1), ((2, 4, 8, 4), 3, 2, 1), ((1, 4, 3, 5), 3, 2, 0), ((1, 4, 8, 8), 3, 2, 0),
             ((1, 4, 1, 2), 3, 2, 1), ((2, 4, 10, 10), 2, 2, 0), ((1, 4, 11, 13), 3, 1, 1),
             ((2, 4, 8, 8), 5, 3, 2), ((1, 4, 16, 16), 15, 1, 7)]


@pytest.mark.parametrize("shape,k,s,p", POOL_GEOS)
def test_pool_refs_match_max_pool2d_autograd(shape, k, s, p):
    torch.manual_seed(0)
    n, c, h, w = shape
    # continuous values (no ties), then five integer values (most windows tie)
    for x in (torch.randn(*shape, dtype=torch.float64), torch.randint(-2, 3, shape).double()):
        xr = x.float().requires_grad_()
        yr = F.max_pool2d(xr, k, s, p)
        dy = torch.randint(-3, 4, yr.shape).float()
        yr.backward(dy)
        y, taps = R.pool_forward(x, k, s, p)
        assert torch.equal(y, yr.detach())
        assert taps.shape == (n, yr.shape[2], yr.shape[3], c)
        assert int(taps.min()) >= 0 and int(taps.max()) < k * k
        dx = R.pool_scatter(dy, taps, h, w, k, s, p)
        assert torch.equal(dx, xr.grad.double())
    if k == 15:  # window (0, 0) starts at (-7, -7): a maximum at pixel (7, 7) is its last tap
        x = torch.zeros(*shape)
        x[:, :, 7, 7] = 1.0
        assert int(R.pool_forward(x, k, s, p)[1][0, 0, 0, 0]) == 224  # a signed byte could not hold it


def test_pool_forward_tap_formula_by_hand():
    x = torch.zeros(1, 1, 4, 4)
    x[0, 0, 2, 3] = 5.0  # window (oh=1, ow=1) of k3/s2/p1 starts at (1, 1): tap (2-1)*3 + (3-1) = 5
    x[0, 0, 0, 0] = 1.0  # window (0, 0) starts at (-1, -1): tap (0+1)*3 + (0+1) = 4
    y, taps = R.pool_forward(x, 3, 2, 1)
    assert y[0, 0].tolist() == [[1.0, 0.0], [0.0, 5.0]]
    # all-zero windows: the first in-bounds tap
    assert taps[0, :, :, 0].tolist() == [[4, 3], [1, 5]]


def test_bn_relu_pool_refs_match_autograd():
    torch.manual_seed(0)
    n, c, h, w = 2, 8, 7, 6
    x = (torch.randint(-32, 33, (n, c, h, w)).float() / 8).bfloat16()
    sc = torch.tensor([-1.0, 0.5, 1.0, 2.0]).repeat(2)
    sh = torch.randint(-8, 9, (c,)).float() / 8
    mean = torch.randint(-4, 5, (c,)).float() / 8
    for p in (0, 1):
        y, taps = R.bn_relu_pool_forward(x, sc, sh, 3, 2, p)
        z = torch.relu(x.double() * sc.double().view(1, c, 1, 1) + sh.double().view(1, c, 1, 1)).requires_grad_()
        assert bool((z.detach().float().bfloat16().double() == z.detach()).all())  # bf16 holds it exactly here
        yr = F.max_pool2d(z, 3, 2, p)
        assert torch.equal(y.double(), yr.detach())
        dy = torch.randint(-3, 4, yr.shape).double()
        yr.backward(dy)
        dz, s0, s1 = R.bn_pool_backward(dy, taps, x, sc, sh, mean, 3, 2, p)
        on = (x.double() * sc.double().view(1, c, 1, 1) + sh.double().view(1, c, 1, 1)) > 0
        dref = torch.where(on, z.grad, torch.zeros_like(z.grad))
        assert torch.equal(dz, dref)
        assert torch.equal(s0, dref.sum(dim=(0, 2, 3)))
        assert torch.equal(s1, (dref * (x.double() - mean.double().view(1, c, 1, 1))).sum(dim=(0, 2, 3)))
