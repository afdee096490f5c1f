"""The pooling kernels (csrc/pool/maxpool.hip) at their edges: outputs, the
argmax bytes themselves, dx, dz and the BN-backward sums, all compared exactly
(atol = rtol = 0) with references derived from CPU PyTorch (tests/exact_ref.py).

Inputs are integers from a range of five values, so most windows hold ties and
the byte must name the FIRST maximum; dy is a small integer, so every gathered
gradient and every fp32 / fp64 sum is exact.  The fused BN+ReLU+pool gets x,
scale and shift on a 1/8 grid, which makes its affine exact in fp32 as well.
DMP_POOL_FWD1 (the one-row A/B variant of the fused forward) is read once per
process and is not covered here."""
import pytest
import torch

from distributed_model_parallel_amd import _native
from tests import exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
POOL_THREADS = 128  # kPoolThreads


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ints(shape, dtype, lo, hi):
    return _cl(torch.randint(lo, hi + 1, shape, device=DEV).to(dtype))


def _same(out, ref, what, nan=False):
    assert out.shape == ref.shape, what
    torch.testing.assert_close(out.double(), ref.double(), atol=0, rtol=0, equal_nan=nan,
                               msg=lambda m: f"{what}: {m}")


def _fwd_bwd(C, x, dy, k, s, p):
    y, idx = C.maxpool2d_forward(x, k, s, p)
    assert idx.dtype == torch.uint8 and idx.numel() == y.numel()
    dx = C.maxpool2d_backward(dy, idx, x.shape[2], x.shape[3], k, s, p)
    return y, idx, dx


def _both_routes(C, cases):
    """Each (x, dy, k, s, p) through the default route (fixed k3/s2 kernels where
    they apply) and through the generic kernels."""
    default = [_fwd_bwd(C, *c) for c in cases]
    C.set_pool_generic(True)
    try:
        generic = [_fwd_bwd(C, *c) for c in cases]
    finally:
        C.set_pool_generic(False)
    return default, generic


def _check_against_ref(x, dy, k, s, p, got, what, nan=False):
    y, idx, dx = got
    n, c, h, w = x.shape
    yr, taps = R.pool_forward(x, k, s, p)
    assert y.dtype == x.dtype and y.is_contiguous(memory_format=torch.channels_last)
    _same(y, yr, "y " + what, nan)
    _same(idx.view(taps.shape).long(), taps, "argmax bytes " + what)
    _same(dx, R.pool_scatter(dy, taps, h, w, k, s, p), "dx " + what, nan)
    return yr, taps


def _case(n, c, h, w, k, s, p, dtype):
    x = _ints((n, c, h, w), dtype, -2, 2)
    dy = _ints((n, c, R.pool_out(h, k, s, p), R.pool_out(w, k, s, p)), dtype, -3, 3)
    return x, dy, k, s, p


def _check_cases(C, cases, nan=False):
    default, generic = _both_routes(C, cases)
    for case, d, g in zip(cases, default, generic):
        x, dy, k, s, p = case
        what = f"{tuple(x.shape)} k{k} s{s} p{p} {x.dtype}"
        _check_against_ref(x, dy, k, s, p, d, what + " default", nan)
        _check_against_ref(x, dy, k, s, p, g, what + " generic", nan)
        for a, b, name in zip(d, g, ("y", "argmax bytes", "dx")):
            _same(a, b, f"{name} default vs generic {what}", nan)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_k3s2_fixed_and_generic_exact(dtype):
    """k3/s2, p in {0, 1}, H and W over odd, even and smaller-than-window
    sizes: the fixed kernels, the generic kernels and the CPU-derived reference
    agree on y, on every argmax byte and on dx."""
    C = _native.require("maxpool2d")
    torch.manual_seed(0)
    cases = []
    for p, sizes in ((0, (3, 4, 5, 7, 8, 9)), (1, (1, 2, 3, 4, 5, 7, 8, 9))):
        for h in sizes:
            for w in sizes:
                cases.append(_case(2, 16, h, w, 3, 2, p, dtype))
    _check_cases(C, cases)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_other_generic_geometries_exact(dtype):
    C = _native.require("maxpool2d")
    torch.manual_seed(1)
    cases = [_case(2, 8, h, w, k, s, p, dtype)
             for (k, s, p) in ((2, 2, 0), (3, 1, 1), (5, 3, 2)) for (h, w) in ((10, 10), (11, 13), (8, 7), (5, 6))]
    _check_cases(C, cases)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_k15_taps_above_127(dtype):
    """k=15, s=1, p=7: tap ids go up to 224 = 14*15 + 14, which a signed byte
    cannot hold.  A planted maximum at pixel (7, 7) is window (0, 0)'s last tap."""
    C = _native.require("maxpool2d")
    torch.manual_seed(2)
    x, dy, k, s, p = _case(1, 8, 16, 16, 15, 1, 7, dtype)
    x[:, :, 7, 7] = 9
    y, idx, dx = _fwd_bwd(C, x, dy, k, s, p)
    _, taps = _check_against_ref(x, dy, k, s, p, (y, idx, dx), "k15")
    assert int(taps[0, 0, 0, 0]) == 224 and int(idx.max()) == 224
    assert int((taps > 127).sum()) > 100


def test_row_longer_than_one_block():
    """row_len = Wo*C/8 = 136 forward and 264 backward: above the 128-lane
    block and no multiple of it, so blockIdx.y > 0 and a partly idle last block."""
    C = _native.require("maxpool2d")
    torch.manual_seed(3)
    case = _case(1, 64, 5, 33, 3, 2, 1, BF16)
    wo = case[1].shape[3]
    assert wo == 17 and wo * 8 > POOL_THREADS and (wo * 8) % POOL_THREADS != 0
    assert 33 * 8 > POOL_THREADS and (33 * 8) % POOL_THREADS != 0
    _check_cases(C, [case])


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_nan_and_infinities(dtype):
    """+-inf mixed into ordinary values, a block of nothing but -inf (its windows
    must name their first in-bounds tap), and NaNs on a grid of pitch k so that
    no window holds two: y is NaN exactly where the reference is, the bytes
    name the NaN, and the gradient reaches the NaN pixel."""
    C = _native.require("maxpool2d")
    torch.manual_seed(4)
    cases, masks = [], []
    for (k, s, p) in ((3, 2, 1), (3, 2, 0), (3, 1, 1)):
        n, c, h, w = 2, 8, 9, 11
        x = _ints((n, c, h, w), dtype, -2, 2)
        r = torch.rand(n, c, h, w, device=DEV)
        x[r < 0.15] = float("inf")
        x[r > 0.7] = float("-inf")
        x[0, :, :4, :] = float("-inf")  # whole windows of -inf, at the border too: the first in-bounds tap
        grid = torch.zeros(n, c, h, w, dtype=torch.bool, device=DEV)
        grid[1, :, 1::k, 1::k] = True
        nan = grid & (torch.rand(n, c, h, w, device=DEV) < 0.5)
        x[nan] = float("nan")
        dy = _ints((n, c, R.pool_out(h, k, s, p), R.pool_out(w, k, s, p)), dtype, 1, 3)
        cases.append((x, dy, k, s, p))
        masks.append(nan)
    _check_cases(C, cases, nan=True)
    for (x, dy, k, s, p), nan in zip(cases, masks):
        y, idx, dx = _fwd_bwd(C, x, dy, k, s, p)
        yr, _ = R.pool_forward(x, k, s, p)
        assert torch.equal(torch.isnan(y), torch.isnan(yr)) and bool(torch.isnan(yr).any())
        # every pixel of rows/columns 1, 4, 7 lies in a window here, and dy > 0
        assert bool((dx[nan] > 0).all())


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_two_nans_in_one_window_first_wins(dtype):
    """This project's documented rule: NaN beats every number, and a later NaN
    does not replace an earlier one (`v != v && m == m`), so the byte names the
    FIRST NaN in window order.  (CPU PyTorch keeps the last NaN; the reference
    in exact_ref.py is therefore not used for this hand-built window.)"""
    C = _native.require("maxpool2d")
    x = _cl(torch.zeros(1, 8, 3, 3, device=DEV, dtype=dtype))
    x[:, :, 0, 1] = float("nan")  # tap 1
    x[:, :, 2, 0] = float("nan")  # tap 6
    x[:, :, 1, 1] = 5.0
    dy = _cl(torch.full((1, 8, 1, 1), 2.0, device=DEV, dtype=dtype))
    default, generic = _both_routes(C, [(x, dy, 3, 2, 0)])
    want = torch.zeros(1, 8, 3, 3, device=DEV, dtype=torch.float64)
    want[:, :, 0, 1] = 2.0
    for y, idx, dx in (default[0], generic[0]):
        assert bool(torch.isnan(y).all())
        assert idx.tolist() == [1] * 8
        _same(dx, want, "dx two NaNs")


def test_rejected_geometries_raise():
    C = _native.require("maxpool2d")
    x = _cl(torch.zeros(1, 8, 20, 20, device=DEV, dtype=BF16))
    with pytest.raises(RuntimeError, match="unsupported pool geometry"):
        C.maxpool2d_forward(x, 16, 1, 8)  # k*k = 256 does not fit the byte
    with pytest.raises(RuntimeError, match="unsupported pool geometry"):
        C.maxpool2d_forward(x, 3, 2, 2)  # 2p > k: a window of padding only
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.maxpool2d_forward(_cl(torch.zeros(1, 12, 8, 8, device=DEV, dtype=BF16)), 3, 2, 1)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        C.maxpool2d_forward(_cl(torch.zeros(1, 6, 8, 8, device=DEV, dtype=F32)), 3, 2, 1)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.maxpool2d_backward(_cl(torch.zeros(1, 12, 4, 4, device=DEV, dtype=BF16)),
                             torch.zeros(12 * 16, device=DEV, dtype=torch.uint8), 8, 8, 3, 2, 1)


# ---------------------------------------------------------------------------
# fused BN + ReLU + pool
# ---------------------------------------------------------------------------
def _bn_inputs(n, c, h, w):
    """x, shift and mean on a 1/8 grid and scale from {-1, 0.5, 1, 2}: x*scale+shift
    is then exact in fp32 (and its ReLU exact in bf16), so nothing is rounded."""
    x = _cl((torch.randint(-32, 33, (n, c, h, w), device=DEV).float() / 8).bfloat16())
    sc = torch.tensor([-1.0, 0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 4, (c,), device=DEV)].contiguous()
    sc[:4] = torch.tensor([-1.0, 0.5, 1.0, 2.0], device=DEV)  # every value, negatives included
    sh = (torch.randint(-8, 9, (c,), device=DEV).float() / 8).contiguous()
    mean = (torch.randint(-4, 5, (c,), device=DEV).float() / 8).contiguous()
    return x, sc, sh, mean


def _check_bn_forward(C, n, c, h, w, p):
    x, sc, sh, _ = _bn_inputs(n, c, h, w)
    what = f"bn pool forward N={n} C={c} {h}x{w} p{p}"
    y, idx = C.maxpool2d_bn_forward(x, sc, sh, 3, 2, p)
    yr, taps = R.bn_relu_pool_forward(x, sc, sh, 3, 2, p)
    assert y.dtype == BF16 and idx.dtype == torch.uint8
    _same(y, yr, "y " + what)
    _same(idx.view(taps.shape).long(), taps, "argmax bytes " + what)
    return taps.shape[1]


@pytest.mark.parametrize("c", [8, 64, 1024])
def test_bn_pool_forward_exact(c):
    """maxpool2d_bn_forward = maxpool(bf16(relu(x*sc+sh))) against fp64: the
    two-rows-per-thread kernel with Ho odd (the second row breaks) and even,
    Ho = 1, both paddings, one to 128 channel vectors."""
    C = _native.require("bn pool forward")
    torch.manual_seed(5)
    seen = set()
    for p, heights in ((1, (1, 2, 3, 4, 9, 10, 16)), (0, (3, 4, 5, 6, 11, 17, 18))):
        for h in heights:
            for w in (3, 4, 7):
                seen.add(_check_bn_forward(C, 2 if c < 1024 else 1, c, h, w, p))
    assert seen == {1, 2, 5, 8}  # Ho


def test_bn_pool_forward_row_longer_than_one_block():
    C = _native.require("bn pool forward")
    torch.manual_seed(6)
    assert R.pool_out(33, 3, 2, 1) * (64 // 8) == 136 > POOL_THREADS
    for h in (6, 9):
        _check_bn_forward(C, 2, 64, h, 33, 1)


@pytest.mark.parametrize("n,c,h,w,p,rb", [(65, 8, 16, 6, 1, 1024), (2, 64, 7, 18, 1, 28), (2, 16, 7, 9, 0, 14),
                                          (3, 16, 9, 7, 1, 27), (40, 64, 8, 18, 1, 640)])
def test_bn_pool_backward_exact(n, c, h, w, p, rb):
    """dz and both BN-backward sums exact on integer dy.  (65, 8, 16, 6) has 1040
    input rows on a 1024-block grid, so 16 blocks take a second row in the
    grid-stride loop, and 1024 partial rows, so the kernel zeroes the sums and
    the reduce adds four chunks atomically; (2, 64, 7, 18) and (40, 64, 8, 18)
    have gy = 2 (row_len 144), the latter with 640 partial rows; (2, 16, 7, 9)
    is p = 0.  Run twice into fresh outputs: equal, so nothing is left over."""
    C = _native.require("bn pool backward")
    torch.manual_seed(7)
    rows, gy = n * h, -(-(w * (c // 8)) // POOL_THREADS)
    assert min(rows, 1024) * gy == rb
    if n == 65:
        assert rows > 1024 and rb > 256
    x, sc, sh, mean = _bn_inputs(n, c, h, w)
    y, idx = C.maxpool2d_bn_forward(x, sc, sh, 3, 2, p)
    yr, taps = R.bn_relu_pool_forward(x, sc, sh, 3, 2, p)
    _same(idx.view(taps.shape).long(), taps, "argmax bytes")
    dy = _ints(tuple(y.shape), BF16, -3, 3)
    dzr, s0, s1 = R.bn_pool_backward(dy, taps, x, sc, sh, mean, 3, 2, p)
    dz1, sums1 = C.maxpool2d_bn_backward(dy, idx, x, sc, sh, mean, 3, 2, p)
    first = sums1.clone()
    del sums1
    dz2, sums2 = C.maxpool2d_bn_backward(dy, idx, x, sc, sh, mean, 3, 2, p)
    for dz, sums in ((dz1, first), (dz2, sums2)):
        _same(dz, dzr, "dz")
        _same(sums[:c], s0, "sum dz")
        _same(sums[c:2 * c], s1, "sum dz*(x-mean)")
        assert sums[2 * c].item() == n * h * w
    assert torch.equal(first, sums2) and torch.equal(dz1, dz2)


# ---------------------------------------------------------------------------
# global average pool backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (5, 7)])
def test_global_avgpool_backward_bound(dtype, h, w):
    """dx = g / HW against fp64.  The kernel multiplies by fp32(1/HW): two fp32
    roundings, |err| <= 2*U*|ref|, plus 2^-8*|ref| for the bf16 store.  HW = 4
    is exact; N=3, C=40 gives 15*HW vector lanes, no multiple of the 256-lane
    block, and more than one block at HW = 35."""
    C = _native.require("global avgpool backward")
    torch.manual_seed(8)
    n, c = 3, 40
    lanes = n * h * w * (c // (8 if dtype == BF16 else 4))
    assert lanes % 256 != 0 and (h * w != 35 or lanes > 256)
    g = torch.randn(n, c, device=DEV).to(dtype)
    dx = C.global_avgpool_backward(g, h, w)
    assert dx.shape == (n, c, h, w) and dx.dtype == dtype and dx.is_contiguous(memory_format=torch.channels_last)
    ref = (g.double() / (h * w)).view(n, c, 1, 1).expand(n, c, h, w)
    bound = 2 * R.U * ref.abs() + (R.BF16_HALF_ULP * ref.abs() if dtype == BF16 else 0)
    err = (dx.double() - ref).abs()
    print(f"gap backward {dtype} HW={h * w}: worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    if h * w == 4 and dtype == F32:
        assert torch.equal(dx.double(), ref)
