"""The depthwise 3x3 kernels (csrc/conv/depthwise.hip) exactly at their
work-split edges, against the fp64 references of tests/exact_ref.py.

Two kinds of input, each with a bound that needs no measurement:
  * small integers (x, w, dy in [-3, 3]): every fp32 partial sum is an integer
    below 2^24 and every bf16-stored output an integer of magnitude <= 81, so
    fp32 accumulation, the fp64 column reduce and bf16 rounding are all exact
    and the kernel must equal the reference bit for bit (atol = rtol = 0).  A
    bf16 weight gradient above 256 is the exact integer rounded once to bf16.
  * randn: with U = 2^-24 and T the same convolution of the absolute values,
    forward / dgrad  |out - ref64| <= 16*U*T  (+ 2^-8*|ref64| for a bf16 output),
    wgrad            |out - ref64| <= n*U*T, n = N*OH*OW (+ 2^-8*|ref64| for bf16),
    which is what fp32 fused-multiply-add accumulation gives; accumulating in
    bf16 or dropping a boundary column in some strips breaks them.
A case that exists to reach a branch reads the host's own work split
(``dwconv3x3_plan``) and asserts that the branch is still reached."""
import pytest
import torch

from distributed_model_parallel_amd import _native
from tests import exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ints(shape, dtype, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, device=DEV).to(dtype)


def _exact(out, ref, what):
    assert out.shape == ref.shape, what
    torch.testing.assert_close(out.double(), ref, atol=0, rtol=0, msg=lambda m: f"{what}: {m}")


def _once(ref, dtype):
    """An exact integer result (below 2^24) as `dtype` stores it: rounded once."""
    return ref.float().to(dtype).double()


def _within(out, ref, bound, what):
    err = (out.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: err/bound = {worst:.3f}"


def _half_ulp(ref, dtype):
    return R.BF16_HALF_ULP * ref.abs() if dtype == BF16 else torch.zeros_like(ref)


def _check_ints(C, n, c, h, w, stride, dtype, wdtype=None, moments=False):
    """forward, dgrad and wgrad on integer data, all compared exactly."""
    wdtype = wdtype or dtype
    what = f"N={n} C={c} {h}x{w} s{stride} {dtype} w {wdtype}"
    x = _cl(_ints((n, c, h, w), dtype))
    wt = _ints((c, 1, 3, 3), wdtype)
    oh, ow = R.dw_out(h, stride), R.dw_out(w, stride)
    dy = _cl(_ints((n, c, oh, ow), dtype))
    y, mom = C.dwconv3x3_forward(x, wt, stride, moments)
    assert y.is_contiguous(memory_format=torch.channels_last) and y.dtype == dtype
    yr = R.dw_forward(x, wt, stride)
    _exact(y, yr, "forward " + what)
    if moments:
        assert mom.dtype == torch.float64 and mom.shape == (2 * c + 1,)
        _exact(mom[:c], yr.sum(dim=(0, 2, 3)), "moments sum " + what)
        _exact(mom[c:2 * c], (yr * yr).sum(dim=(0, 2, 3)), "moments sum of squares " + what)
        assert mom[2 * c].item() == n * oh * ow
    else:
        assert mom is None
    dx = C.dwconv3x3_dgrad(dy, wt, stride, h, w)
    _exact(dx, R.dw_dgrad(dy, wt, stride, h, w), "dgrad " + what)
    dwr = R.dw_wgrad(dy, x, stride)
    assert float(dwr.abs().max()) < 2 ** 24
    dw = C.dwconv3x3_wgrad(dy, x, stride, wdtype)
    assert dw.shape == (c, 1, 3, 3) and dw.dtype == wdtype
    _exact(dw, _once(dwr, wdtype), "wgrad " + what)
    return x, dy, dwr


def _check_real(C, n, c, h, w, stride, dtype, wdtype):
    """forward, dgrad and wgrad on randn data under the derived fp32-FMA bounds."""
    what = f"N={n} C={c} {h}x{w} s{stride} {dtype} w {wdtype}"
    x = _cl(torch.randn(n, c, h, w, device=DEV).to(dtype))
    wt = (torch.randn(c, 1, 3, 3, device=DEV) * 0.5).to(wdtype)
    oh, ow = R.dw_out(h, stride), R.dw_out(w, stride)
    dy = _cl(torch.randn(n, c, oh, ow, device=DEV).to(dtype))
    y, _ = C.dwconv3x3_forward(x, wt, stride, False)
    yr = R.dw_forward(x, wt, stride)
    _within(y, yr, 16 * R.U * R.dw_forward_abs(x, wt, stride) + _half_ulp(yr, dtype), "forward " + what)
    dx = C.dwconv3x3_dgrad(dy, wt, stride, h, w)
    dxr = R.dw_dgrad(dy, wt, stride, h, w)
    _within(dx, dxr, 16 * R.U * R.dw_dgrad_abs(dy, wt, stride, h, w) + _half_ulp(dxr, dtype), "dgrad " + what)
    dw = C.dwconv3x3_wgrad(dy, x, stride, wdtype)
    dwr = R.dw_wgrad(dy, x, stride)
    _within(dw, dwr, n * oh * ow * R.U * R.dw_wgrad_abs(dy, x, stride) + _half_ulp(dwr, wdtype), "wgrad " + what)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_geometry_sweep_integers(dtype, stride):
    """Every OW % 4 and W % 4 remainder, H = 1, W = 1, stride 2 on odd and even
    sizes: forward, dgrad and wgrad exact.  N=2, C=16 is one block with idle
    lanes (tc = 2 or 4), so the strip masks are what is tested."""
    C = _native.require("dw")
    torch.manual_seed(0)
    sizes = (1, 2, 3, 4, 5, 7, 8, 9)
    for h in sizes:
        for w in sizes:
            _check_ints(C, 2, 16, h, w, stride, dtype)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c,dtype,tc,spp,idle", [(24, BF16, 3, 85, 1), (960, BF16, 120, 2, 16),
                                                 (960, F32, 240, 1, 16)])
def test_idle_lanes(c, dtype, tc, spp, idle, stride):
    """Channel counts whose vector count does not divide the 256-lane block:
    lanes with ls >= spp must neither store nor add to the block's partials."""
    C = _native.require("dw")
    torch.manual_seed(1)
    n, h, w = 2, 5, 6
    g = C.dwconv3x3_plan(n, c, h, w, stride, dtype)
    assert (g["tc"], g["spp"], g["idle"]) == (tc, spp, idle)
    _check_ints(C, n, c, h, w, stride, dtype, moments=True)
    _check_real(C, n, c, h, w, stride, dtype, dtype)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c,dtype", [(2056, BF16), (1028, F32)])
def test_two_channel_chunks(c, dtype, stride):
    """blockIdx.y = 1 with a single active lane: every other lane of the second
    chunk has cvec >= cv.  Forward with moments, dgrad and wgrad."""
    C = _native.require("dw")
    torch.manual_seed(2)
    g = C.dwconv3x3_plan(1, c, 5, 5, stride, dtype)
    assert g["cchunks"] == 2 and g["last_chunk_lanes"] == 1
    _check_ints(C, 1, c, 5, 5, stride, dtype, moments=True)
    _check_real(C, 1, c, 5, 5, stride, dtype, dtype)


def _wgrad_all_outputs(C, x, dy, dwr, stride, what):
    """Both out_dtype values, then out= accumulation into a non-zero integer gradient."""
    c = x.shape[1]
    for od in (F32, BF16):
        dw = C.dwconv3x3_wgrad(dy, x, stride, od)
        assert dw.dtype == od
        _exact(dw, _once(dwr, od), f"wgrad {what} out {od}")
        prev = _ints((c, 1, 3, 3), od, -5, 5)
        prev[prev == 0] = 7
        acc = prev.clone()
        ret = C.dwconv3x3_wgrad(dy, x, stride, od, out=acc)
        assert ret.data_ptr() == acc.data_ptr()
        _exact(acc, _once(dwr + prev.double(), od), f"wgrad {what} out= {od}")


def test_wgrad_several_strips_per_lane_one_chunk():
    """strips_per_lane = 2 with one channel chunk (CIFAR-sized maps at a large
    batch run this loop): 1561 lane-passes over 781 blocks, the last block's
    first pass partly and its second pass wholly past `total`."""
    C = _native.require("dw")
    torch.manual_seed(3)
    n, c, h, w, stride = 32, 96, 64, 64, 1
    g = C.dwconv3x3_plan(n, c, h, w, stride, BF16)
    assert g["cchunks"] == 1 and g["passes"] == 1561 and g["spl"] >= 2
    assert g["total"] % g["spp"] != 0 and g["wgrad_past_total"] > g["spp"]
    x = _cl(_ints((n, c, h, w), BF16))
    dy = _cl(_ints((n, c, h, w), BF16))
    dwr = R.dw_wgrad(dy, x, stride)
    assert 256 < float(dwr.abs().max()) < 2 ** 24  # a bf16 result is really rounded
    _wgrad_all_outputs(C, x, dy, dwr, stride, "C=96 N=32 64x64")
    # the same split with real data
    x = _cl(torch.randn(n, c, h, w, device=DEV).bfloat16())
    dy = _cl(torch.randn(n, c, h, w, device=DEV).bfloat16())
    dwr = R.dw_wgrad(dy, x, stride)
    T = R.dw_wgrad_abs(dy, x, stride)
    for od in (F32, BF16):
        dw = C.dwconv3x3_wgrad(dy, x, stride, od)
        _within(dw, dwr, n * h * w * R.U * T + _half_ulp(dwr, od), f"wgrad real C=96 N=32 64x64 out {od}")


@pytest.mark.parametrize("n,h,w,past", [(2, 17, 62, 0), (1, 35, 60, 1)])
def test_wgrad_several_strips_per_lane_two_chunks(n, h, w, past):
    """strips_per_lane = 2 with two channel chunks (C = 2056 bf16, spp = 1).
    (2, 17, 62) fills 272 blocks x 2 passes exactly; (1, 35, 60) has 525
    lane-passes, so the last block's second pass is past `total` and breaks."""
    C = _native.require("dw")
    torch.manual_seed(4)
    c, stride = 2056, 1
    g = C.dwconv3x3_plan(n, c, h, w, stride, BF16)
    assert g["cchunks"] == 2 and g["spp"] == 1 and g["spl"] >= 2
    assert g["wgrad_past_total"] == past
    x = _cl(_ints((n, c, h, w), BF16))
    dy = _cl(_ints((n, c, h, w), BF16))
    dwr = R.dw_wgrad(dy, x, stride)
    assert float(dwr.abs().max()) < 2 ** 24
    _wgrad_all_outputs(C, x, dy, dwr, stride, f"C=2056 N={n} {h}x{w}")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c,dtype", [(24, BF16), (960, BF16), (2056, BF16), (24, F32), (960, F32)])
def test_forward_moments_integers(c, dtype, stride):
    """sum and sum of squares of the stored output, exact, with OW % 4 != 0 and
    enough strips that every lane row of a block (spp up to 85) has work and a
    second, partly filled block follows: the fold over all spp rows is tested."""
    C = _native.require("dw")
    torch.manual_seed(5)
    n, h, w = 4, 11, 26
    g = C.dwconv3x3_plan(n, c, h, w, stride, dtype)
    assert g["OW"] % 4 != 0 and g["total"] > g["spp"] and g["passes"] >= 2
    _check_ints(C, n, c, h, w, stride, dtype, moments=True)


def test_forward_moments_more_than_256_partial_rows():
    """288 partial rows: the forward kernel zeroes the sums itself and the
    reduce adds two row chunks with fp64 atomics.  The second run's sums land
    on memory that may still hold the first run's: equal results need the
    self-zeroing.  Integer data exact; real data within rows*U*sum|.| of the
    fp64 sums of the stored y (every fp32 partial adds TW*spp = 8 <= rows terms)."""
    C = _native.require("dw")
    torch.manual_seed(6)
    n, c, h, w, stride = 3, 960, 16, 48, 1
    g = C.dwconv3x3_plan(n, c, h, w, stride, BF16)
    rows = g["passes"]
    assert rows == 288 and rows > 256 and 4 * g["spp"] <= rows
    x = _cl(_ints((n, c, h, w), BF16))
    wt = _ints((c, 1, 3, 3), BF16)
    yr = R.dw_forward(x, wt, stride)
    y1, mom1 = C.dwconv3x3_forward(x, wt, stride, True)
    first = mom1.clone()
    del mom1
    y2, mom2 = C.dwconv3x3_forward(x, wt, stride, True)
    for y, mom in ((y1, first), (y2, mom2)):
        _exact(y, yr, "forward 288 rows")
        _exact(mom[:c], yr.sum(dim=(0, 2, 3)), "moments sum 288 rows")
        _exact(mom[c:2 * c], (yr * yr).sum(dim=(0, 2, 3)), "moments sum of squares 288 rows")
        assert mom[2 * c].item() == n * h * w
    assert torch.equal(first, mom2)
    x = _cl(torch.randn(n, c, h, w, device=DEV).bfloat16())
    wt = (torch.randn(c, 1, 3, 3, device=DEV) * 0.5).bfloat16()
    y, mom = C.dwconv3x3_forward(x, wt, stride, True)
    y64 = y.double()
    _within(mom[:c], y64.sum(dim=(0, 2, 3)), rows * R.U * y64.abs().sum(dim=(0, 2, 3)), "real moments sum")
    _within(mom[c:2 * c], (y64 * y64).sum(dim=(0, 2, 3)), rows * R.U * (y64 * y64).sum(dim=(0, 2, 3)),
            "real moments sum of squares")
    assert mom[2 * c].item() == n * h * w


@pytest.mark.parametrize("dtype,wdtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
@pytest.mark.parametrize("n,c,h,w,stride", [(4, 96, 32, 32, 1), (3, 144, 32, 32, 2), (2, 960, 4, 4, 1)])
def test_real_data_within_fp32_fma_bounds(n, c, h, w, stride, dtype, wdtype):
    """randn data, weights in bf16 and in fp32 beside bf16 activations: integers
    cannot show low-precision accumulation, these bounds do."""
    C = _native.require("dw")
    torch.manual_seed(7)
    _check_real(C, n, c, h, w, stride, dtype, wdtype)


def test_plan_reports_the_documented_work_splits():
    """The host's own integers (``dwconv3x3_plan`` reads the structs the launches
    read; it launches nothing) at the splits the cases above are placed on."""
    C = _native.require("dw")
    plan = C.dwconv3x3_plan
    g = plan(32, 96, 64, 64, 1, BF16)
    assert (g["tc"], g["spp"], g["strips"], g["cchunks"], g["passes"], g["spl"]) == (12, 21, 16, 1, 1561, 2)
    assert g["wgrad_past_total"] > 0
    assert plan(4, 96, 32, 32, 1, BF16)["passes"] == 49 and plan(4, 96, 32, 32, 1, BF16)["spl"] == 1
    assert plan(1, 24, 4, 4, 1, BF16)["idle"] == 1
    g = plan(1, 960, 4, 4, 1, BF16)
    assert (g["tc"], g["spp"], g["idle"]) == (120, 2, 16)
    g = plan(1, 960, 4, 4, 1, F32)
    assert (g["tc"], g["spp"], g["idle"]) == (240, 1, 16)
    for c, dt in ((2056, BF16), (1028, F32)):
        g = plan(1, c, 5, 5, 2, dt)
        assert (g["cchunks"], g["last_chunk_lanes"]) == (2, 1)
    assert plan(3, 960, 16, 48, 1, BF16)["passes"] == 288
    g = plan(2, 2056, 17, 62, 1, BF16)
    assert (g["cchunks"], g["spl"], g["wgrad_past_total"]) == (2, 2, 0)
    # the data gradient walks input rows: 62 columns are 16 strips of 4, 2 * 17 * 16 rows of them
    assert (g["vec"], g["cv"], g["dgrad_strips"], g["dgrad_grid_x"]) == (8, 257, 16, 544)


def test_plans_refuse_tensors_beyond_the_index_range():
    """N*H*W*C = 2^47 elements: past what the kernels' offsets are checked for.
    Host-only, nothing is allocated."""
    C = _native.require("dw")
    with pytest.raises(RuntimeError, match="too large"):
        C.dwconv3x3_plan(1 << 20, 8, 4096, 4096, 1, BF16)
    with pytest.raises(RuntimeError, match="too large"):
        C.dwconv7x7_plan(1 << 20, 8, 4096, 4096)
