"""The depthwise 7x7 kernels (csrc/conv/depthwise7.hip) against the fp64
references of tests/exact_ref_dw7.py, at ConvNeXt's shapes in small, at maps
smaller than the kernel, and exactly at the edges of the host's work split
(read from ``dwconv7x7_plan``, so a case that exists to reach an edge asserts
that the edge is still reached).

Two kinds of input, each with a bound that needs no measurement:
  * integers in [-2, 2] (x, w, bias, dy, add): every forward / dgrad output
    has magnitude <= 49*4 + 2 = 198 < 256, so fp32 accumulation and the one
    bf16 rounding are exact: atol = rtol = 0.  dw / db are exact integers
    below 2^24; as bf16 they are that integer rounded once.
  * randn: U = 2^-24, T the same stencil of absolute values (with |bias| /
    |add|): forward / dgrad |out - ref64| <= 128*U*T + 2^-8*|ref64| (50 terms,
    product and add possibly rounded separately: 2 x 50 rounded up);
    wgrad / bias gradient |out - ref64| <= (n + 16)*U*T (+ 2^-8*|ref64| for a
    bf16 result), n = N*H*W."""
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import depthwise7 as D7
from distributed_model_parallel_amd.ops.fused import GradSlot, grad_tap
from tests import exact_ref_dw7 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

SHAPES = [(1, 8, 1, 1), (2, 8, 3, 5), (1, 16, 7, 7), (2, 96, 7, 7), (3, 128, 14, 14), (2, 136, 9, 13),
          (1, 64, 28, 30), (2, 256, 6, 20)]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ints(shape, dtype, lo=-2, hi=2):
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


def _check_ints(C, n, c, h, w, wdtype):
    """forward (+ bias), dgrad (with and without add) and wgrad on integer data, all exact."""
    what = f"N={n} C={c} {h}x{w} w {wdtype}"
    x = _cl(_ints((n, c, h, w), BF16))
    dy = _cl(_ints((n, c, h, w), BF16))
    add = _cl(_ints((n, c, h, w), BF16))
    wt, b = _ints((c, 1, 7, 7), wdtype), _ints((c,), wdtype)
    y = C.dwconv7x7_forward(x, wt, b)
    assert y.is_contiguous(memory_format=torch.channels_last) and y.dtype == BF16
    _exact(y, R.forward(x, wt, b), "forward " + what)
    _exact(C.dwconv7x7_forward(x, wt), R.forward(x, wt), "forward, no bias " + what)
    _exact(C.dwconv7x7_dgrad(dy, wt), R.dgrad(dy, wt), "dgrad " + what)
    dx = C.dwconv7x7_dgrad(dy, wt, add)
    assert dx.is_contiguous(memory_format=torch.channels_last) and dx.dtype == BF16
    _exact(dx, R.dgrad(dy, wt, add), "dgrad + add " + what)
    dwr, dbr = R.wgrad(dy, x)
    assert float(dwr.abs().max()) < 2 ** 24 and float(dbr.abs().max()) < 2 ** 24
    for od in (wdtype, F32 if wdtype == BF16 else BF16):
        dw, db = C.dwconv7x7_wgrad(dy, x, od)
        assert dw.shape == (c, 1, 7, 7) and db.shape == (c,) and dw.dtype == od and db.dtype == od
        _exact(dw, _once(dwr, od), f"wgrad {what} out {od}")
        _exact(db, _once(dbr, od), f"bias grad {what} out {od}")
        dw2, db2 = C.dwconv7x7_wgrad(dy, x, od)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "wgrad is not reproducible " + what


def _check_real(C, n, c, h, w, wdtype):
    """forward, dgrad and wgrad on randn data under the derived fp32 bounds."""
    what = f"N={n} C={c} {h}x{w} w {wdtype}"
    x = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    dy = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    add = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    wt = (torch.randn(c, 1, 7, 7, device=DEV) * 0.2).to(wdtype)
    b = torch.randn(c, device=DEV).to(wdtype)
    yr = R.forward(x, wt, b)
    _within(C.dwconv7x7_forward(x, wt, b), yr, 128 * R.U * R.forward_abs(x, wt, b) + _half_ulp(yr, BF16),
            "forward " + what)
    for a in (None, add):
        dxr = R.dgrad(dy, wt, a)
        _within(C.dwconv7x7_dgrad(dy, wt, a), dxr, 128 * R.U * R.dgrad_abs(dy, wt, a) + _half_ulp(dxr, BF16),
                f"dgrad add={a is not None} " + what)
    dwr, dbr = R.wgrad(dy, x)
    tw, tb = R.wgrad_abs(dy, x)
    m = n * h * w + 16
    for od in (F32, BF16):
        dw, db = C.dwconv7x7_wgrad(dy, x, od)
        _within(dw, dwr, m * R.U * tw + _half_ulp(dwr, od), f"wgrad {what} out {od}")
        _within(db, dbr, m * R.U * tb + _half_ulp(dbr, od), f"bias grad {what} out {od}")
        dw2, db2 = C.dwconv7x7_wgrad(dy, x, od)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "wgrad is not reproducible " + what


@pytest.mark.parametrize("wdtype", [BF16, F32])
@pytest.mark.parametrize("n,c,h,w", SHAPES)
def test_integers_exact(n, c, h, w, wdtype):
    C = _native.require("dw7")
    torch.manual_seed(0)
    _check_ints(C, n, c, h, w, wdtype)


@pytest.mark.parametrize("wdtype", [BF16, F32])
@pytest.mark.parametrize("n,c,h,w", SHAPES)
def test_real_data_within_fp32_bounds(n, c, h, w, wdtype):
    C = _native.require("dw7")
    torch.manual_seed(1)
    _check_real(C, n, c, h, w, wdtype)


@pytest.mark.parametrize("k", [-1, 0, 1])
@pytest.mark.parametrize("axis", ["h", "w"])
def test_tile_multiple_edges(axis, k):
    """H and W one below, at and one above a multiple of the tile (two tiles):
    the last tile's masked rows / columns and the halo beside them."""
    C = _native.require("dw7")
    torch.manual_seed(2)
    p0 = C.dwconv7x7_plan(1, 8, 1, 1)
    th, tw, thw = p0["tile_h"], p0["tile_w"], p0["wgrad_tile_h"]
    h, w = (2 * th + k, 5) if axis == "h" else (3, 2 * tw + k)
    p = C.dwconv7x7_plan(2, 16, h, w)
    assert p["tiles_h"] == (2 if k <= 0 else 3) if axis == "h" else p["tiles_w"] == (2 if k <= 0 else 3)
    assert p["wgrad_tiles"] == 2 * -(-h // thw) * p["tiles_w"]
    _check_ints(C, 2, 16, h, w, BF16)
    _check_real(C, 2, 16, h, w, F32)


@pytest.mark.parametrize("below", [True, False])
def test_channels_beside_a_block(below):
    """C one 8-vector below the channels a block covers (one chunk, idle lanes)
    and one above (a second chunk with 4 active lanes)."""
    C = _native.require("dw7")
    torch.manual_seed(3)
    full = C.dwconv7x7_plan(1, 4096, 5, 6)["channels_per_block"]
    c = full - 8 if below else full + 8
    p = C.dwconv7x7_plan(1, c, 5, 6)
    if below:
        assert p["grid_y"] == 1 and p["channels_per_block"] == c and p["tiles_per_block"] == 1
    else:
        assert p["grid_y"] == 2 and p["channels_per_block"] == full
    _check_ints(C, 1, c, 5, 6, BF16)
    _check_real(C, 1, c, 5, 6, BF16)


def test_wgrad_one_tile_over_a_chunk_boundary():
    """Two tiles per lane in the weight gradient, the last block holding
    exactly one tile: its second pass is past the end and must add nothing."""
    C = _native.require("dw7")
    torch.manual_seed(4)
    n, c, h, w = 1, 1024, 514, 8
    p = C.dwconv7x7_plan(n, c, h, w)
    per_block = p["wgrad_tiles_per_lane"] * p["tiles_per_block"]
    assert p["wgrad_tiles_per_lane"] >= 2 and p["grid_y"] == 2
    assert p["wgrad_tiles"] == (p["wgrad_blocks"] - 1) * per_block + 1
    x = _cl(_ints((n, c, h, w), BF16))
    dy = _cl(_ints((n, c, h, w), BF16))
    dwr, dbr = R.wgrad(dy, x)
    assert 256 < float(dwr.abs().max()) < 2 ** 24  # a bf16 result is really rounded
    for od in (F32, BF16):
        dw, db = C.dwconv7x7_wgrad(dy, x, od)
        _exact(dw, _once(dwr, od), f"wgrad chunk edge out {od}")
        _exact(db, _once(dbr, od), f"bias grad chunk edge out {od}")
    x = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    dy = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    dwr, dbr = R.wgrad(dy, x)
    tw, tb = R.wgrad_abs(dy, x)
    dw, db = C.dwconv7x7_wgrad(dy, x, F32)
    _within(dw, dwr, (n * h * w + 16) * R.U * tw, "wgrad chunk edge real")
    _within(db, dbr, (n * h * w + 16) * R.U * tb, "bias grad chunk edge real")


@pytest.mark.parametrize("wdtype", [BF16, F32])
def test_autograd_equals_the_raw_calls(wdtype):
    """The op's forward, backward and the grad_slot's parked residual gradient
    are the three raw calls, bit for bit."""
    C = _native.require("dw7")
    torch.manual_seed(5)
    n, c, h, w = 2, 64, 9, 11
    x = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16)).requires_grad_()
    conv = D7.DepthwiseConv7x7(c).to(DEV, wdtype)
    with torch.no_grad():
        conv.bias.normal_()
    gy = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    gr = _cl(torch.randn(n, c, h, w, device=DEV).to(BF16))
    before = dict(D7._STATS)
    slot = GradSlot()
    y = conv(x, slot)
    res = grad_tap(x, slot)
    assert slot.consumer and res is not x
    ((y * gy).sum() + (res * gr).sum()).backward()
    assert D7._STATS["native"] == before["native"] + 1 and D7._STATS["torch"] == before["torch"]
    assert D7._STATS["fused_residual_grad"] == before["fused_residual_grad"] + 1
    assert torch.equal(y, C.dwconv7x7_forward(x.detach(), conv.weight.detach(), conv.bias.detach()))
    assert torch.equal(x.grad, C.dwconv7x7_dgrad(gy, conv.weight.detach(), gr))
    dw, db = C.dwconv7x7_wgrad(gy, x.detach(), wdtype)
    assert torch.equal(conv.weight.grad, dw) and torch.equal(conv.bias.grad, db)
    # without a slot: the plain data gradient
    x.grad = None
    (conv(x) * gy).sum().backward()
    assert torch.equal(x.grad, C.dwconv7x7_dgrad(gy, conv.weight.detach()))


def test_set_enabled_false_routes_to_torch():
    torch.manual_seed(6)
    x = _cl(torch.randn(2, 32, 7, 7, device=DEV).to(BF16))
    conv = D7.DepthwiseConv7x7(32).to(DEV, BF16)
    with torch.no_grad():
        y_native = conv(x)
    D7.set_enabled(False)
    try:
        before = dict(D7._STATS)
        with torch.no_grad():
            y = conv(x)
        assert D7._STATS["torch"] == before["torch"] + 1 and D7._STATS["native"] == before["native"]
    finally:
        D7.set_enabled(True)
    yr = R.forward(x, conv.weight.detach(), conv.bias.detach())
    assert float((y.double() - yr).abs().max()) <= 2.0 ** -6 * float(yr.abs().max())
    assert float((y_native.double() - yr).abs().max()) <= 2.0 ** -6 * float(yr.abs().max())
    # fp32 activations are outside the kernel's contract: torch, not an error
    before = dict(D7._STATS)
    conv32 = D7.DepthwiseConv7x7(32).to(DEV)
    conv32(_cl(torch.randn(2, 32, 7, 7, device=DEV)))
    assert D7._STATS["torch"] == before["torch"] + 1
