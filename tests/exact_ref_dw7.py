"""Plain fp64 references for the depthwise 7x7 kernels
(csrc/conv/depthwise7.hip), built from tap views with no conv call, on
whatever device the inputs live on.  Stride 1, padding 3; x [N,C,H,W],
w [C,1,7,7], bias [C].

As in tests/exact_ref.py two kinds of comparison use them:
  * integer-valued inputs in [-2, 2]: every forward / dgrad output has
    magnitude <= 49*4 + 2 = 198 < 256, so fp32 accumulation and the one bf16
    rounding are exact and the kernel must equal the reference bit for bit;
  * real-valued inputs, where the bound is a multiple of U * T with T the same
    stencil of the absolute values -- the ``*_abs`` functions.
tests/test_depthwise7_cpu.py checks the references against PyTorch autograd in
fp64 on the CPU."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24             # fp32 unit roundoff
BF16_HALF_ULP = 2.0 ** -8  # half a bf16 ulp at the bottom of a binade, relative
K, PAD = 7, 3


def _tap(tp, kh, kw, h, w):
    """The [N,C,h,w] view of the padded tensor that tap (kh, kw) reads."""
    return tp[:, :, kh:kh + h, kw:kw + w]


def forward(x, w, bias=None):
    """y[n,c,h,w] = b[c] + sum_{kh,kw} x[n,c,h+kh-3,w+kw-3] * w[c,0,kh,kw]"""
    x, w = x.double(), w.double()
    n, c, h, wd = x.shape
    xp = F.pad(x, (PAD, PAD, PAD, PAD))
    y = torch.zeros(n, c, h, wd, dtype=torch.float64, device=x.device)
    if bias is not None:
        y += bias.double().view(1, c, 1, 1)
    for kh in range(K):
        for kw in range(K):
            y += _tap(xp, kh, kw, h, wd) * w[:, 0, kh, kw].view(1, c, 1, 1)
    return y


def dgrad(dy, w, add=None):
    """dx = add + scatter of dy through the taps (= the stencil with flipped taps)."""
    dy, w = dy.double(), w.double()
    n, c, h, wd = dy.shape
    dxp = torch.zeros(n, c, h + 2 * PAD, wd + 2 * PAD, dtype=torch.float64, device=dy.device)
    for kh in range(K):
        for kw in range(K):
            _tap(dxp, kh, kw, h, wd).add_(dy * w[:, 0, kh, kw].view(1, c, 1, 1))
    dx = dxp[:, :, PAD:h + PAD, PAD:wd + PAD].contiguous()
    if add is not None:
        dx += add.double()
    return dx


def wgrad(dy, x):
    """(dw [C,1,7,7], db [C])"""
    dy, x = dy.double(), x.double()
    n, c, h, wd = dy.shape
    xp = F.pad(x, (PAD, PAD, PAD, PAD))
    dw = torch.zeros(c, 1, K, K, dtype=torch.float64, device=x.device)
    for kh in range(K):
        for kw in range(K):
            dw[:, 0, kh, kw] = (_tap(xp, kh, kw, h, wd) * dy).sum(dim=(0, 2, 3))
    return dw, dy.sum(dim=(0, 2, 3))


def forward_abs(x, w, bias=None):
    return forward(x.double().abs(), w.double().abs(), None if bias is None else bias.double().abs())


def dgrad_abs(dy, w, add=None):
    return dgrad(dy.double().abs(), w.double().abs(), None if add is None else add.double().abs())


def wgrad_abs(dy, x):
    return wgrad(dy.double().abs(), x.double().abs())
