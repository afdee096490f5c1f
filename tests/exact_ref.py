"""Plain fp64 references for the depthwise, pooling and batch-norm kernels, on
whatever device the inputs live on.

Two kinds of comparison use them (tests/test_gpu_depthwise_edges.py,
tests/test_gpu_pool_edges.py, tests/test_gpu_bn_edges.py):
  * integer-valued inputs, where every fp32 partial sum is an integer below
    2^24 and every bf16 output an integer of magnitude at most 256: the kernel
    must then equal the fp64 reference bit for bit;
  * real-valued inputs, where the bound is U * (sum of |products|) from fp32
    fused-multiply-add accumulation -- the ``*_abs`` functions give that sum.
tests/test_exact_ref_cpu.py checks the references themselves against PyTorch
autograd in fp64 on the CPU."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24        # fp32 unit roundoff
BF16_HALF_ULP = 2.0 ** -8  # half a bf16 ulp at the bottom of a binade, relative


# ---------------------------------------------------------------------------
# depthwise 3x3, padding 1, stride 1 or 2; x [N,C,H,W], w [C,1,3,3], all fp64
# ---------------------------------------------------------------------------
def dw_out(size, stride):
    return (size + 2 - 3) // stride + 1


def _tap_view(t, kh, kw, oh, ow, s):
    """The [N,C,oh,ow] view of the padded tensor that tap (kh, kw) reads."""
    return t[:, :, kh:kh + (oh - 1) * s + 1:s, kw:kw + (ow - 1) * s + 1:s]


def dw_forward(x, w, stride):
    x, w = x.double(), w.double()
    n, c, h, wd = x.shape
    oh, ow = dw_out(h, stride), dw_out(wd, stride)
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros(n, c, oh, ow, dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            y += _tap_view(xp, kh, kw, oh, ow, stride) * w[:, 0, kh, kw].view(1, c, 1, 1)
    return y


def dw_dgrad(dy, w, stride, h, wd):
    dy, w = dy.double(), w.double()
    n, c, oh, ow = dy.shape
    assert (oh, ow) == (dw_out(h, stride), dw_out(wd, stride))
    dxp = torch.zeros(n, c, h + 2, wd + 2, dtype=torch.float64, device=dy.device)
    for kh in range(3):
        for kw in range(3):
            _tap_view(dxp, kh, kw, oh, ow, stride).add_(dy * w[:, 0, kh, kw].view(1, c, 1, 1))
    return dxp[:, :, 1:h + 1, 1:wd + 1].contiguous()


def dw_wgrad(dy, x, stride):
    dy, x = dy.double(), x.double()
    n, c, oh, ow = dy.shape
    assert (oh, ow) == (dw_out(x.shape[2], stride), dw_out(x.shape[3], stride))
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(c, 1, 3, 3, dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            dw[:, 0, kh, kw] = (_tap_view(xp, kh, kw, oh, ow, stride) * dy).sum(dim=(0, 2, 3))
    return dw


def dw_forward_abs(x, w, stride):
    return dw_forward(x.double().abs(), w.double().abs(), stride)


def dw_dgrad_abs(dy, w, stride, h, wd):
    return dw_dgrad(dy.double().abs(), w.double().abs(), stride, h, wd)


def dw_wgrad_abs(dy, x, stride):
    return dw_wgrad(dy.double().abs(), x.double().abs(), stride)


# ---------------------------------------------------------------------------
# max pooling; taps as the kernels store them: one byte per [N,Ho,Wo,C] element
# ---------------------------------------------------------------------------
def pool_out(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def pool_forward(x, k, s, p):
    """(y, taps) from CPU PyTorch on an NCHW fp32 copy of x [N,C,H,W] (bf16 and
    fp32 are both exact in it): y [N,C,Ho,Wo] fp32, taps [N,Ho,Wo,C] int64 with
    tap = (ih - (oh*s - p)) * k + (iw - (ow*s - p)), both on x's device.  First
    maximum in window order; an all -inf window gives its first in-bounds tap;
    with one NaN in a window the NaN wins."""
    xc = x.detach().float().cpu().contiguous()
    n, c, h, w = xc.shape
    y, ind = F.max_pool2d(xc, k, s, p, return_indices=True)
    ho, wo = y.shape[2], y.shape[3]
    assert (ho, wo) == (pool_out(h, k, s, p), pool_out(w, k, s, p))
    ih, iw = ind // w, ind % w
    oh = torch.arange(ho).view(1, 1, ho, 1)
    ow = torch.arange(wo).view(1, 1, 1, wo)
    a, b = ih - (oh * s - p), iw - (ow * s - p)
    assert bool(((a >= 0) & (a < k) & (b >= 0) & (b < k)).all())
    taps = (a * k + b).permute(0, 2, 3, 1).contiguous()
    return y.to(x.device), taps.to(x.device)


def pool_scatter(dy, taps, h, w, k, s, p):
    """dx [N,C,H,W] fp64: every dy[n,c,oh,ow] added to the input pixel its tap names."""
    n, c, ho, wo = dy.shape
    dev = dy.device
    taps = taps.to(dev).long().view(n, ho, wo, c)
    oh = torch.arange(ho, device=dev).view(1, ho, 1, 1)
    ow = torch.arange(wo, device=dev).view(1, 1, wo, 1)
    ih = oh * s - p + taps // k
    iw = ow * s - p + taps % k
    assert bool(((ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)).all()), "a tap names a padding pixel"
    nn_ = torch.arange(n, device=dev).view(n, 1, 1, 1).expand_as(taps)
    cc = torch.arange(c, device=dev).view(1, 1, 1, c).expand_as(taps)
    flat = ((nn_ * c + cc) * h + ih) * w + iw
    dx = torch.zeros(n * c * h * w, dtype=torch.float64, device=dev)
    dx.index_add_(0, flat.reshape(-1), dy.double().permute(0, 2, 3, 1).reshape(-1))
    return dx.view(n, c, h, w)


def bn_relu_pool_forward(x, scale, shift, k, s, p):
    """maxpool(bf16(relu(x * scale + shift))) with the affine in fp64: (y, taps)
    as pool_forward gives them.  The caller chooses x, scale and shift so that
    the affine is exact in fp32 too (tests/test_gpu_pool_edges.py)."""
    c = x.shape[1]
    z = torch.relu(x.double() * scale.double().view(1, c, 1, 1) + shift.double().view(1, c, 1, 1))
    z32 = z.float()
    assert bool((z32.double() == z).all()), "the affine is not exact in fp32"
    return pool_forward(z32.bfloat16(), k, s, p)


def bn_pool_backward(dy, taps, x, scale, shift, mean, k, s, p):
    """(dz [N,C,H,W] fp64, sum dz [C], sum dz*(x-mean) [C]) of the fused BN+ReLU+pool
    backward: the pool gradient rounded to bf16, masked by relu'(x*scale+shift)."""
    n, c, h, w = x.shape
    g = pool_scatter(dy, taps, h, w, k, s, p).float().bfloat16().double()
    x64 = x.double()
    on = x64 * scale.double().view(1, c, 1, 1) + shift.double().view(1, c, 1, 1) > 0
    dz = torch.where(on, g, torch.zeros_like(g))
    return dz, dz.sum(dim=(0, 2, 3)), (dz * (x64 - mean.double().view(1, c, 1, 1))).sum(dim=(0, 2, 3))


# ---------------------------------------------------------------------------
# batch normalisation over the rows of an [M, C] matrix, split into the phases
# csrc/bn/batchnorm.hip has: moments -> coefficients -> apply, and the same
# for the backward.  Everything is fp64 and nothing is rounded on the way, so
# a caller that wants exact equality chooses inputs whose results fp32 holds.
# ---------------------------------------------------------------------------
def bn_moments(x):
    """fp64 [2C+1] = (column sums, column sums of squares, rows)."""
    xd = x.double()
    return torch.cat([xd.sum(0), (xd * xd).sum(0), xd.new_tensor([float(x.shape[0])])])


def bn_moments_abs(x):
    """(sum |x|, sum x^2) per channel: what the moments' rounding errors scale with."""
    xd = x.double()
    return xd.abs().sum(0), (xd * xd).sum(0)


def _or_const(t, like, value):
    return t.double() if t is not None else torch.full_like(like, value)


def bn_fwd_coeffs(sums, weight, bias, eps):
    """(mean, var, invstd, scale, shift), each fp64 [C], with the arithmetic of
    csrc/bn/bn_coeffs.h: biased variance clamped at 0, eps as fp32 holds it."""
    c = (sums.numel() - 1) // 2
    sums = sums.double()
    n = sums[2 * c]
    mean = sums[:c] / n
    var = (sums[c:2 * c] / n - mean * mean).clamp_min(0.0)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    invstd = 1.0 / torch.sqrt(var + eps32)
    scale = _or_const(weight, invstd, 1.0) * invstd
    shift = _or_const(bias, invstd, 0.0) - mean * scale
    return mean, var, invstd, scale, shift


def bn_eval_coeffs(running_mean, running_var, weight, bias, eps):
    """(mean, invstd, scale, shift) of an eval-mode BN, from the running statistics."""
    mean = running_mean.double()
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    invstd = 1.0 / torch.sqrt(running_var.double() + eps32)
    scale = _or_const(weight, invstd, 1.0) * invstd
    return mean, invstd, scale, _or_const(bias, invstd, 0.0) - mean * scale


def bn_preact(x, scale, shift, residual=None):
    t = x.double() * scale + shift
    return t if residual is None else t + residual.double()


def bn_apply(x, scale, shift, residual=None, relu=False, clip=float("inf")):
    """act(x * scale + shift [+ residual]); act = ReLU clipped at `clip` when relu."""
    t = bn_preact(x, scale, shift, residual)
    return t.clamp(0.0, clip) if relu else t


def bn_apply_abs(x, mean, scale, bias, residual=None):
    """|x*scale| + |mean*scale| + |bias| + |residual|: the terms the apply rounds."""
    t = (x.double() * scale).abs() + (mean * scale).abs() + _or_const(bias, scale, 0.0).abs()
    return t if residual is None else t + residual.double().abs()


def bn_running_update(running_mean, running_var, mean, var, n, momentum):
    """The running statistics after one training step over n rows (unbiased variance)."""
    n = float(n)
    unbiased = var * n / (n - 1.0) if n > 1.0 else var
    return ((1.0 - momentum) * running_mean.double() + momentum * mean,
            (1.0 - momentum) * running_var.double() + momentum * unbiased)


def bn_mask_from_y(y, clip=float("inf")):
    """Where the clipped ReLU passes a gradient, from its output: 0 < y < clip, both strict."""
    yd = y.double()
    return (yd > 0.0) & (yd < clip)


def bn_mask_from_x(x, scale, shift, clip=float("inf")):
    """The same mask re-derived from the BN input (no residual was added)."""
    return bn_mask_from_y(bn_preact(x, scale, shift), clip)


def _dz(dy, mask):
    dz = dy.double()
    return dz if mask is None else dz * mask


def bn_bwd_moments(dy, x, mean, mask=None):
    """fp64 [2C] = (sum dz, sum dz*(x - mean)), dz = dy where `mask` (None: everywhere)."""
    dz = _dz(dy, mask)
    return torch.cat([dz.sum(0), (dz * (x.double() - mean.double())).sum(0)])


def bn_bwd_moments_abs(dy, x, mean, mask=None):
    dz = _dz(dy, mask).abs()
    return dz.sum(0), (dz * (x.double() - mean.double()).abs()).sum(0)


def bn_bwd_coeffs(sums, count, weight, mean, invstd, training=True):
    """(a, b, c, dweight, dbias), fp64 [C]: dx = a*dz + b*x + c.  `count` is the
    global row count; eval mode has b = c = 0."""
    c_ = sums.numel() // 2
    sums = sums.double()
    sdz, sdzx = sums[:c_], sums[c_:]
    istd = invstd.double()
    a = _or_const(weight, istd, 1.0) * istd
    if training:
        b = -a * istd * istd * sdzx / float(count)
        c = -a * sdz / float(count) - b * mean.double()
    else:
        b, c = torch.zeros_like(a), torch.zeros_like(a)
    return a, b, c, sdzx * istd, sdz


def bn_bwd_apply(dy, x, a, b, c, mask=None):
    """(dx, dz): dz is also the gradient of a fused residual."""
    dz = _dz(dy, mask)
    return a * dz + b * x.double() + c, dz


def bn_bwd_apply_abs(dy, x, a, b, c, mask=None):
    return (a * _dz(dy, mask)).abs() + (b * x.double()).abs() + c.abs()
