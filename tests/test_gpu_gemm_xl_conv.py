"""gemm_xl conv epilogues (moments / add / bnbwd) on the glds-ring kernel must
agree with the 4-wave NT kernel's (gemm_nt / gemm_nt_bnbwd) -- same math,
same rounding points -- and with fp64 sums of what they store."""
import pytest
import torch

from distributed_model_parallel_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"


def C():
    return _native.require("gemm_xl_conv tests")


@pytest.mark.parametrize("M,N,K", [(4096, 256, 64), (3001, 512, 128), (50176, 1024, 256), (700, 128, 192)])
def test_xl_moments_matches_nt(M, N, K):
    torch.manual_seed(0)
    a = torch.randn(M, K, device=DEV).bfloat16()
    b = (torch.randn(N, K, device=DEV) * 0.1).bfloat16()
    c, mom = C().gemm_xl_conv(a, b, "moments")
    c0, _ = C().gemm_nt(a, b)
    torch.testing.assert_close(c.float(), c0.float(), atol=2e-2, rtol=1e-2)
    cd = c.double()
    torch.testing.assert_close(mom[:N], cd.sum(0), atol=1e-2, rtol=1e-4)
    torch.testing.assert_close(mom[N:2 * N], (cd * cd).sum(0), atol=1e-2, rtol=1e-4)
    assert mom[2 * N].item() == M


@pytest.mark.parametrize("M,N,K", [(4096, 256, 64), (1999, 512, 256)])
def test_xl_add_matches_nt(M, N, K):
    torch.manual_seed(1)
    a = torch.randn(M, K, device=DEV).bfloat16()
    b = (torch.randn(N, K, device=DEV) * 0.1).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    c, _ = C().gemm_xl_conv(a, b, "add", residual=r)
    c0, _ = C().gemm_nt(a, b, mode="add", residual=r)
    torch.testing.assert_close(c.float(), c0.float(), atol=2e-2, rtol=1e-2)


@pytest.mark.parametrize("mask_from_y", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_xl_bnbwd_matches_nt(mask_from_y, with_res):
    torch.manual_seed(2)
    M, N, K = 5000, 256, 128
    dy = torch.randn(M, K, device=DEV).bfloat16()
    wt = (torch.randn(N, K, device=DEV) * 0.1).bfloat16()
    x = torch.randn(M, N, device=DEV).bfloat16()
    mean = x.float().mean(0)
    inv = torch.rand(N, device=DEV) + 0.5
    bw = torch.rand(N, device=DEV) + 0.5
    bb = torch.randn(N, device=DEV) * 0.5
    res = torch.randn(M, N, device=DEV).bfloat16() if with_res else None
    y = torch.relu(x.float() * inv * bw + bb - mean * inv * bw).bfloat16() if mask_from_y else None
    i_, w_, b_ = (None, None, None) if mask_from_y else (inv, bw, bb)
    dz, sums = C().gemm_xl_conv(dy, wt, "bnbwd", residual=res, bn_x=x, bn_y=y, mean=mean, invstd=i_,
                                weight=w_, bias=b_)
    dz0, sums0 = C().gemm_nt_bnbwd(dy, wt, res, x, y, mean, i_, w_, b_)
    torch.testing.assert_close(dz.float(), dz0.float(), atol=2e-2, rtol=1e-2)
    dzd = dz.double()
    torch.testing.assert_close(sums[:N], dzd.sum(0), atol=1e-2, rtol=1e-4)
    torch.testing.assert_close(sums[N:2 * N], (dzd * (x.double() - mean.double())).sum(0), atol=1e-2, rtol=1e-4)


@pytest.mark.parametrize("pipe", [10, 11])
@pytest.mark.parametrize("mode", ["moments", "bnbwd"])
def test_xl_conv_pingpong_schedule(mode, pipe):
    """The 256 x 256 main loops (PIPE 10: 8-wave ping-pong, PIPE 11: 4 waves)
    under the conv epilogues equal the half-step ring kernel."""
    C = _native.require("gemm_xl_conv")
    torch.manual_seed(11)
    M, N, K = 5000, 512, 576
    a = torch.randn(M, K, device=DEV).bfloat16()
    b = (torch.randn(N, K, device=DEV) * 0.05).bfloat16()
    kw = {}
    if mode == "bnbwd":
        x = torch.randn(M, N, device=DEV).bfloat16()
        kw = dict(bn_x=x, mean=torch.zeros(N, device=DEV), invstd=torch.ones(N, device=DEV))
    C.set_gemm_xl_bn(256, 1)
    try:
        ref, rs = C.gemm_xl_conv(a, b, mode, **kw)
        C.set_gemm_xl_bn(256, pipe)
        got, gs = C.gemm_xl_conv(a, b, mode, **kw)
    finally:
        C.set_gemm_xl_bn(0)
    torch.testing.assert_close(got.float(), ref.float(), atol=0.02, rtol=1e-2)
    torch.testing.assert_close(gs, rs, atol=1e-2 * M ** 0.5, rtol=1e-3)


# ---- every conv epilogue under every main-loop / tile-width / x2 setting ----
# M = 300: one full 256-row tile and a ragged one.  N = 384 = 128 + 256: the
# two-blocks-per-CU route at x2 mode 1, a ragged last 256-wide tile otherwise.
# K = 192: three K tiles (prologue, steady state, drain of every main loop).
_RM, _RN, _RK = 300, 384, 192
_ROUTE_CASES = ["moments", "add", "affine", "affine-res-relu", "bnbwd-x", "bnbwd-xy", "bnbwd-y"]


@pytest.fixture(scope="module")
def route_ref():
    """Operands of every case and this file's reference for it (gemm_nt /
    gemm_nt_bnbwd, which the xl knobs do not reach), computed once."""
    C = _native.require("gemm_xl_conv")
    M, N, K = _RM, _RN, _RK
    torch.manual_seed(21)
    a = torch.randn(M, K, device=DEV).bfloat16()
    b = (torch.randn(N, K, device=DEV) * 0.1).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    x = torch.randn(M, N, device=DEV).bfloat16()
    mean = x.float().mean(0)
    inv = torch.rand(N, device=DEV) + 0.5
    bw = torch.rand(N, device=DEV) + 0.5
    bb = torch.randn(N, device=DEV) * 0.5
    y = torch.relu(x.float() * inv * bw + bb - mean * inv * bw).bfloat16()
    sc = torch.rand(N, device=DEV) + 0.5
    sh = torch.randn(N, device=DEV)
    kw = {
        "moments": {},
        "add": dict(residual=r),
        "affine": dict(scale=sc, shift=sh),
        "affine-res-relu": dict(scale=sc, shift=sh, residual=r, relu=True),
        "bnbwd-x": dict(residual=r, bn_x=x, mean=mean, invstd=inv, weight=bw, bias=bb),
        "bnbwd-xy": dict(residual=r, bn_x=x, bn_y=y, mean=mean),
        "bnbwd-y": dict(residual=r, bn_y=y),
    }
    ref = {
        "moments": C.gemm_nt(a, b)[0],
        "add": C.gemm_nt(a, b, mode="add", residual=r)[0],
        "affine": C.gemm_nt(a, b, mode="affine", epi_scale=sc, epi_shift=sh)[0],
        "affine-res-relu": C.gemm_nt(a, b, mode="affine", epi_scale=sc, epi_shift=sh, residual=r, relu=True)[0],
        "bnbwd-x": C.gemm_nt_bnbwd(a, b, r, x, None, mean, inv, bw, bb)[0],
        "bnbwd-xy": C.gemm_nt_bnbwd(a, b, r, x, y, mean, None, None, None)[0],
        "bnbwd-y": C.gemm_nt_bnbwd(a, b, r, None, y, None, None, None, None)[0],
    }
    return a, b, kw, {k: v.float() for k, v in ref.items()}, x.double() - mean.double()


@pytest.mark.parametrize("x2", [0, 1])
@pytest.mark.parametrize("setting", [(0, -1), (128, 1), (256, 1), (128, 0), (256, 0), (256, 10), (256, 11)],
                         ids=["auto", "bn128", "bn256", "bn128-pipe0", "bn256-pipe0", "bn256-pingpong", "bn256-w4"])
@pytest.mark.parametrize("case", _ROUTE_CASES)
def test_xl_conv_every_route(route_ref, case, setting, x2):
    """Each gemm_xl_conv mode and bnbwd operand form lands on the right
    kernel instantiation under every (bn, pipe) setting of test_gpu_gemm_xl's
    `bn` fixture and both x2 modes.  This file's references are the gemm_nt
    kernels (same math, same rounding points) and fp64 sums of what was
    stored, at this file's tolerances; the affine cases, which it did not
    cover, take gemm_nt's affine epilogue at the same tolerance as "add"."""
    C = _native.require("gemm_xl_conv")
    a, b, kw, ref, xc = route_ref
    N = _RN
    old_pipe, old_x2 = C.get_gemm_xl_pipe(), C.get_gemm_xl_x2()
    C.set_gemm_xl_bn(*setting)
    C.set_gemm_xl_x2(x2)
    try:
        c, sums = C.gemm_xl_conv(a, b, case.split("-")[0], **kw[case])
    finally:
        C.set_gemm_xl_bn(0, old_pipe)
        C.set_gemm_xl_x2(old_x2)
    torch.testing.assert_close(c.float(), ref[case], atol=2e-2, rtol=1e-2)
    if case == "moments" or case.startswith("bnbwd"):
        cd = c.double()
        second = cd * cd if case == "moments" else cd * xc if "x" in case.split("-")[1] else torch.zeros_like(cd)
        torch.testing.assert_close(sums[:N], cd.sum(0), atol=1e-2, rtol=1e-4)
        torch.testing.assert_close(sums[N:2 * N], second.sum(0), atol=1e-2, rtol=1e-4)
        assert sums[2 * N].item() == _RM
