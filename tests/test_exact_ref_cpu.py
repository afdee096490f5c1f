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


def _bn_case(m, c, seed=0):
    """Non-degenerate fp64 data: channel means and spreads differ, nothing sits on a ReLU threshold."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, dtype=torch.float64, generator=g) * (0.5 + torch.rand(c, dtype=torch.float64, generator=g)) \
        + torch.randn(c, dtype=torch.float64, generator=g) * 2
    w = torch.randn(c, dtype=torch.float64, generator=g)
    b = torch.randn(c, dtype=torch.float64, generator=g)
    res = torch.randn(m, c, dtype=torch.float64, generator=g)
    dy = torch.randn(m, c, dtype=torch.float64, generator=g)
    return x, w, b, res, dy


@pytest.mark.parametrize("affine", ["both", "no_weight", "no_bias", "neither"])
@pytest.mark.parametrize("act", [None, "relu", "relu6"])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,c", [(2, 4), (37, 8), (200, 24)])
def test_bn_training_refs_match_batch_norm_autograd(m, c, residual, act, affine):
    x, w, b, res, dy = _bn_case(m, c)
    if act == "relu6":
        x = x * 3  # enough pre-activations above the clip
    w = w if affine in ("both", "no_bias") else None
    b = b if affine in ("both", "no_weight") else None
    eps, momentum = 1e-5, 0.3
    clip = {None: float("inf"), "relu": float("inf"), "relu6": 6.0}[act]
    rm0, rv0 = torch.randn(c, dtype=torch.float64), torch.rand(c, dtype=torch.float64) + 0.5
    leaves = [t.clone().requires_grad_() for t in (x, res) + tuple(t for t in (w, b) if t is not None)]
    xl, rl = leaves[0], leaves[1]
    wl = leaves[2] if w is not None else None
    bl = leaves[-1] if b is not None else None
    rm, rv = rm0.clone(), rv0.clone()
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    t = F.batch_norm(xl, rm, rv, wl, bl, True, momentum, eps32)
    if residual:
        t = t + rl
    y = t if act is None else F.hardtanh(t, 0.0, clip) if act == "relu6" else F.relu(t)
    y.backward(dy)

    sums = R.bn_moments(x)
    assert sums.shape == (2 * c + 1,) and sums[2 * c].item() == m
    mean, var, invstd, scale, shift = R.bn_fwd_coeffs(sums, w, b, eps)
    close = dict(atol=1e-11, rtol=1e-11)
    torch.testing.assert_close(mean, x.mean(0), **close)
    torch.testing.assert_close(var, x.var(0, unbiased=False), **close)
    yr = R.bn_apply(x, scale, shift, res if residual else None, act is not None, clip)
    torch.testing.assert_close(yr, y.detach(), **close)
    nrm, nrv = R.bn_running_update(rm0, rv0, mean, var, m, momentum)
    torch.testing.assert_close(nrm, rm, **close)
    torch.testing.assert_close(nrv, rv, **close)

    mask = None if act is None else R.bn_mask_from_y(yr, clip)
    if act is not None and not residual:  # both ways to the mask agree off the thresholds
        assert torch.equal(mask, R.bn_mask_from_x(x, scale, shift, clip))
        assert 0 < int(mask.sum()) < mask.numel()
    bs = R.bn_bwd_moments(dy, x, mean, mask)
    a, bb, cc, dw, db = R.bn_bwd_coeffs(bs, m, w, mean, invstd, True)
    dx, dz = R.bn_bwd_apply(dy, x, a, bb, cc, mask)
    torch.testing.assert_close(dx, xl.grad, **close)
    if residual:
        torch.testing.assert_close(dz, rl.grad, **close)
    if w is not None:
        torch.testing.assert_close(dw, wl.grad, **close)
    if b is not None:
        torch.testing.assert_close(db, bl.grad, **close)
    # the |.|-companions bound what they accompany
    sa, qa = R.bn_moments_abs(x)
    assert bool((sa >= sums[:c].abs() - 1e-12).all()) and torch.equal(qa, sums[c:2 * c])
    ba, bq = R.bn_bwd_moments_abs(dy, x, mean, mask)
    assert bool((ba >= bs[:c].abs() - 1e-12).all()) and bool((bq >= bs[c:].abs() - 1e-12).all())
    ya = R.bn_apply_abs(x, mean, scale, b, res if residual else None)
    assert bool((ya >= R.bn_preact(x, scale, shift, res if residual else None).abs() - 1e-12).all())
    assert bool((R.bn_bwd_apply_abs(dy, x, a, bb, cc, mask) >= dx.abs() - 1e-12).all())


@pytest.mark.parametrize("act", [None, "relu6"])
def test_bn_eval_refs_match_batch_norm_autograd(act):
    m, c = 37, 8
    x, w, b, res, dy = _bn_case(m, c, seed=1)
    eps = 1e-3
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    clip = 6.0 if act else float("inf")
    rm, rv = torch.randn(c, dtype=torch.float64), torch.rand(c, dtype=torch.float64) + 0.5
    xl, wl, bl = (t.clone().requires_grad_() for t in (x, w, b))
    t = F.batch_norm(xl, rm.clone(), rv.clone(), wl, bl, False, 0.1, eps32)
    y = F.hardtanh(t, 0.0, clip) if act else t
    y.backward(dy)
    mean, invstd, scale, shift = R.bn_eval_coeffs(rm, rv, w, b, eps)
    yr = R.bn_apply(x, scale, shift, None, act is not None, clip)
    torch.testing.assert_close(yr, y.detach(), atol=1e-12, rtol=1e-12)
    mask = R.bn_mask_from_x(x, scale, shift, clip) if act else None
    bs = R.bn_bwd_moments(dy, x, mean, mask)
    a, bb, cc, dw, db = R.bn_bwd_coeffs(bs, m, w, mean, invstd, False)
    assert not bb.any() and not cc.any()
    dx, _ = R.bn_bwd_apply(dy, x, a, bb, cc, mask)
    torch.testing.assert_close(dx, xl.grad, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dw, wl.grad, atol=1e-11, rtol=1e-11)
    torch.testing.assert_close(db, bl.grad, atol=1e-11, rtol=1e-11)


def test_bn_refs_on_the_thresholds_and_on_a_dead_channel():
    # masks are strict at both ends
    y = torch.tensor([[-1.0, 0.0, 0.5, 6.0, 7.0]])
    assert R.bn_mask_from_y(y, 6.0).tolist() == [[False, False, True, False, False]]
    assert R.bn_mask_from_y(y).tolist() == [[False, False, True, True, True]]
    # a constant channel: the variance is clamped at 0 and invstd = 1/sqrt(eps as fp32 holds it)
    x = torch.full((5, 2), 0.3, dtype=torch.float64)
    x[:, 1] = 0.0
    mean, var, invstd, scale, shift = R.bn_fwd_coeffs(R.bn_moments(x), None, None, 1e-5)
    assert not var.any()
    assert invstd[0].item() == 1.0 / float(torch.tensor(1e-5, dtype=torch.float32)) ** 0.5
    # one row: the running variance takes the biased value
    _, nrv = R.bn_running_update(torch.zeros(2), torch.ones(2), mean, var, 1, 0.5)
    assert nrv.tolist() == [0.5, 0.5]


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
