"""PatchEmbed (ops/patch_embed.py) on patch vectors that are not a multiple of
the GEMM's K step of 64 -- the ConvNeXt stem's 4 x 4 x 3 = 48, zero-padded to
64 -- and on the 2 x 2 downsampling conv of a channels-last activation.  Both
against ``F.conv2d`` in fp32 (output and all three gradients) with the cosine /
norm-ratio bounds of tests/test_gpu_models.py::_compare; and a shape that was
already native (16 x 16 x 3 = 768) bit-equal to the parent's forward."""
import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import patch_embed as PE

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(a, b, what, min_cos=0.95):
    a, b = a.float().flatten(), b.float().flatten()
    cos = F.cosine_similarity(a, b, dim=0).item()
    rel = (a.norm() / b.norm()).item()
    print(f"{what}: cos {cos:.5f} norm ratio {rel:.4f}")
    assert cos >= min_cos and 0.9 < rel < 1.1, f"{what}: cos={cos:.4f} norm_ratio={rel:.3f}"


@pytest.mark.parametrize("cin,dim,p,shape", [(3, 128, 4, (256, 3, 32, 32)), (128, 256, 2, (256, 128, 8, 8))])
def test_matches_conv2d(cin, dim, p, shape):
    torch.manual_seed(0)
    pe = PE.PatchEmbed(cin, dim, p).to(DEV)
    with torch.no_grad():
        pe.bias.normal_(std=0.1)
    ref_w = pe.weight.detach().bfloat16().float().requires_grad_()
    ref_b = pe.bias.detach().bfloat16().float().requires_grad_()
    pe = pe.bfloat16().to(memory_format=torch.channels_last)
    x32 = torch.randn(*shape, device=DEV).bfloat16().float().contiguous(memory_format=torch.channels_last)
    x = x32.bfloat16().requires_grad_()
    x32.requires_grad_()
    rows = shape[0] * (shape[2] // p) * (shape[3] // p)
    assert rows >= 4096  # the fused GEMM path's minimum: 16384 for the stem, 4096 for the downsampling conv
    gy = torch.randn(shape[0], rows // shape[0], dim, device=DEV).bfloat16()
    n0, t0 = PE._STATS["native"], PE._STATS["torch"]
    y = pe(x)
    assert PE._STATS["native"] == n0 + 1 and PE._STATS["torch"] == t0
    y.backward(gy)
    yr = F.conv2d(x32, ref_w, ref_b, stride=p).flatten(2).transpose(1, 2)
    yr.backward(gy.float())
    assert y.shape == yr.shape and pe.weight.grad.shape == ref_w.shape and x.grad.shape == x32.shape
    _close(y, yr, "output")
    _close(x.grad, x32.grad, "input gradient")
    _close(pe.weight.grad, ref_w.grad, "weight gradient")
    _close(pe.bias.grad, ref_b.grad, "bias gradient")


def test_multiple_of_64_is_bit_equal_to_the_unpadded_forward():
    """16 x 16 x 3 = 768: the padding code is not reached; the output equals the
    parent's two-line forward (patchify, gemm_xl with the bias) bit for bit."""
    C = _native.require("patch embed")
    torch.manual_seed(1)
    pe = PE.PatchEmbed(3, 768, 16).to(DEV).bfloat16()
    x = torch.randn(64, 3, 128, 128, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    n0 = PE._STATS["native"]
    y = pe(x)
    assert PE._STATS["native"] == n0 + 1
    b, c, h, w = x.shape
    patches = x.reshape(b, c, h // 16, 16, w // 16, 16).permute(0, 2, 4, 3, 5, 1).reshape(b * 64, 768)
    wmat = pe.weight.permute(0, 2, 3, 1).reshape(768, -1).contiguous()
    yp = C.gemm_xl(patches, wmat, "bias", bias=pe.bias).view(b, 64, 768)
    assert torch.equal(y, yp)
