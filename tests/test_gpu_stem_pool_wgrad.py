"""stem_halo_wgrad_pool (csrc/conv/stem_halo.hip): the stem's folded backward in
one pass over y -- the pool / ReLU backward dz is formed per tile in LDS and
feeds dz^T P next to y^T P -- against fp64 and against the three launches it
replaces (maxpool2d_bn_backward + two stem_halo_wgrad)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (images, image height); the kernel is fixed to a 224-px-wide image (112 output columns):
#   (1, 8)    2 tiles, both touch the image top and bottom
#   (3, 24)   interior tiles; 18 tiles on 18 blocks
#   (130, 8)  260 tiles on up to 256 blocks: some blocks run two tiles (double buffer, carried
#             dy / argmax prefetch)
#   (100, 64) 1,600 tiles, six to seven consecutive tiles per block across image boundaries
SHAPES = [(1, 8), (3, 24), (130, 8), (100, 64)]
CASES = [(n, h, pad) for (n, h) in SHAPES for pad in (0, 1)]


def _native():
    from distributed_model_parallel_amd import _native as nat
    return nat.require("stem pool wgrad test")


@functools.lru_cache(maxsize=None)
def _case(n, h, pad):
    """Inputs, the three separate launches' results and the fp64 references of one case."""
    C = _native()
    torch.manual_seed(1000 * n + 10 * h + pad)
    dev = "cuda"
    ho, wo, co = h // 2, 112, 64
    img = torch.randn(n, 3, h, 224, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
    s = C.space_to_depth2(img, 3)
    y = (torch.randn(n, co, ho, wo, device=dev) + 0.3).bfloat16().contiguous(memory_format=torch.channels_last)
    sc = torch.rand(co, device=dev) + 0.5
    sc[3], sc[17], sc[40] = -0.7, -1.2, -0.4  # negative scales flip the mask and the pool's order
    sc[9] = 0.0                               # exact zero: the mask is sign(shift) everywhere
    sh = torch.randn(co, device=dev) * 0.3
    mean = torch.randn(co, device=dev) * 0.1
    sc, sh, mean = sc.contiguous(), sh.contiguous(), mean.contiguous()
    _, idx = C.maxpool2d_bn_forward(y, sc, sh, 3, 2, pad)
    hp, wp = (ho + 2 * pad - 3) // 2 + 1, (wo + 2 * pad - 3) // 2 + 1
    dy = torch.randn(n, co, hp, wp, device=dev)
    dy = torch.where(torch.rand_like(dy) < 0.1, torch.zeros_like(dy), dy)  # some exact zeros
    dy = dy.bfloat16().contiguous(memory_format=torch.channels_last)
    # today's three launches (dz is pinned bit-exactly by test_bn_pool_backward_kernel_vs_fp32)
    dz, sums_sep = C.maxpool2d_bn_backward(dy, idx, y, sc, sh, mean, 3, 2, pad)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(n * ho * wo, co)  # noqa: E731
    t_dz_sep = C.stem_halo_wgrad(rows(dz), s, ho, torch.float32)
    t_y_sep = C.stem_halo_wgrad(rows(y), s, ho, torch.float32)
    # fp64 dz^T P and y^T P from the same bf16 dz, y, s; P by unfold on the s2d image,
    # columns reordered from unfold's (c, kh, kw) to the kernel's (kh, kw, c)
    ref_dz = torch.zeros(co, 256, device=dev, dtype=torch.float64)
    ref_y = torch.zeros_like(ref_dz)
    step = 10
    for i in range(0, n, step):
        sl = slice(i, min(n, i + step))
        p = F.unfold(s[sl, :, : ho + 3].double(), kernel_size=4)  # [b, 16 * 16, ho * 112]
        b = p.shape[0]
        p = p.view(b, 16, 16, ho * wo).permute(0, 2, 1, 3).reshape(b, 256, ho * wo)
        dzr = dz[sl].permute(0, 2, 3, 1).reshape(b, ho * wo, co).double()
        yr = y[sl].permute(0, 2, 3, 1).reshape(b, ho * wo, co).double()
        ref_dz += torch.einsum("blo,bkl->ok", dzr, p)
        ref_y += torch.einsum("blo,bkl->ok", yr, p)
    d64 = rows(dz).double()
    y64 = rows(y).double()
    ref_sums = (d64.sum(0), (d64 * (y64 - mean.double())).sum(0))
    fused = C.stem_halo_wgrad_pool(dy, idx, y, s, sc, sh, mean, ho, pad)
    torch.cuda.synchronize()
    return dict(fused=fused, t_dz_sep=t_dz_sep, t_y_sep=t_y_sep, sums_sep=sums_sep, ref_dz=ref_dz, ref_y=ref_y,
                ref_sums=ref_sums, rows=n * ho * wo)


@pytest.mark.parametrize("n,h,pad", CASES)
def test_fused_products_vs_fp64(n, h, pad):
    """t_dz = dz^T P and t_y = y^T P against fp64: at most twice the max-abs error of
    today's two stem_halo_wgrad calls against the same reference, plus one fp32 ulp
    of the largest entry (both are fp32 sums of identical products).

    The fused kernel keeps stem_wgrad_kernel's tile partition, k order and MFMA
    sequence per accumulator and forms dz with bnpool_bwd_kernel's arithmetic, so
    bit equality with the separate calls is expected; on MI355X it held in all
    eight cases (asserted below, the stronger check)."""
    c = _case(n, h, pad)
    t_dz, t_y, _ = c["fused"]
    assert t_dz.shape == (64, 256) and t_y.shape == (64, 256) and t_dz.dtype == torch.float32
    for name, got, sep, ref in (("t_dz", t_dz, c["t_dz_sep"], c["ref_dz"]), ("t_y", t_y, c["t_y_sep"], c["ref_y"])):
        err_sep = (sep.double() - ref).abs().max().item()
        err_fused = (got.double() - ref).abs().max().item()
        ulp = float(np.spacing(np.float32(ref.abs().max().item())))
        print(f"{name} n={n} h={h} pad={pad}: separate {err_sep:.3e} fused {err_fused:.3e} ulp {ulp:.3e} "
              f"bit-equal {torch.equal(got, sep)}")
        assert err_fused <= 2.0 * err_sep + ulp, (name, err_fused, err_sep, ulp)
        assert torch.equal(got, sep), name


@pytest.mark.parametrize("n,h,pad", CASES)
def test_fused_bn_sums_vs_fp64(n, h, pad):
    """sums = (sum dz, sum dz (y - mean), rows) against fp64, with
    test_bn_pool_backward_kernel_vs_fp32's tolerances."""
    c = _case(n, h, pad)
    sums = c["fused"][2]
    assert sums.dtype == torch.float64 and sums.numel() == 129
    for k, ref in enumerate(c["ref_sums"]):
        got = sums[64 * k: 64 * (k + 1)]
        print(f"sums[{k}] n={n} h={h} pad={pad}: max abs err {(got - ref).abs().max().item():.3e} "
              f"(separate {(c['sums_sep'][64 * k: 64 * (k + 1)] - ref).abs().max().item():.3e})")
        torch.testing.assert_close(got, ref, atol=1e-3, rtol=1e-4)
    assert sums[128].item() == c["rows"] == n * (h // 2) * 112


@pytest.mark.parametrize("pad", [0, 1])
def test_stem_step_fused_vs_separate(pad):
    """conv_bn_maxpool on 8 x 3 x 224 x 224 with the one-pass route on and off: equal
    forwards; conv weight / BN weight / BN bias gradients within
    test_stem_bn_backward_folded_into_wgrad's bound (relative L2 < 2e-2) of the
    dx-materialising path, and on against off far tighter (observed on MI355X:
    conv weight 0 -- the products are bit-equal and only the fp32 order of the BN sums moves --
    BN weight / bias below 1e-6).  A silent fallback fails the route counter."""
    import copy

    from distributed_model_parallel_amd.ops import fused
    from distributed_model_parallel_amd.ops.batchnorm import BatchNormAct2d
    from distributed_model_parallel_amd.ops.pool import MaxPool2d
    from distributed_model_parallel_amd.ops.stem import StemConv2d
    torch.manual_seed(0)
    conv = StemConv2d(3, 64).cuda().bfloat16().to(memory_format=torch.channels_last)
    bn = BatchNormAct2d(64, act="relu").cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0.0, 0.2)
    pool = MaxPool2d(3, 2, pad)
    x = torch.randn(8, 3, 224, 224, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    g = None
    outs, grads, routed = {}, {}, {}
    old = (fused._FUSE_STEM_POOL_WGRAD, fused._FUSE_STEM_WGRAD)
    try:
        for arm, (one_pass, fold) in (("on", (True, True)), ("off", (False, True)), ("dx", (False, False))):
            fused._FUSE_STEM_POOL_WGRAD, fused._FUSE_STEM_WGRAD = one_pass, fold
            cv, b = copy.deepcopy(conv), copy.deepcopy(bn)
            r0 = fused._STATS_FUSED["stem_pool_wgrad"]
            y = fused.conv_bn_maxpool(cv, b, pool, x)
            if g is None:
                g = torch.randn_like(y)
            y.backward(g)
            torch.cuda.synchronize()
            routed[arm] = fused._STATS_FUSED["stem_pool_wgrad"] - r0
            outs[arm] = y.detach()
            grads[arm] = (cv.weight.grad, b.weight.grad, b.bias.grad)
    finally:
        fused._FUSE_STEM_POOL_WGRAD, fused._FUSE_STEM_WGRAD = old
    assert routed == {"on": 1, "off": 0, "dx": 0}, routed
    assert torch.equal(outs["on"], outs["off"]) and torch.equal(outs["on"], outs["dx"])
    for i, name in enumerate(("conv w", "bn w", "bn b")):
        a, off, dx = (grads[k][i].float() for k in ("on", "off", "dx"))
        e_dx = ((a - dx).norm() / dx.norm()).item()
        e_off = ((a - off).norm() / off.norm()).item()
        print(f"pad {pad} {name}: vs dx path {e_dx:.3e}, on vs off {e_off:.3e}")
        assert e_dx < 2e-2, (name, e_dx)
        assert e_off < 2e-2, (name, e_off)
