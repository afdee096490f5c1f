"""Streamed long-sequence attention (csrc/attn/attention_long.hip, S > 256)
against the fp32 PyTorch reference of tests/test_gpu_attention.py, with that
file's input scale and bounds: forward atol = rtol = 2e-2; per-part gradient
error <= 2e-2 |ref part| + 1e-3 |ref grad|.  Lengths: one full 256-key chunk
plus one row (257), a ragged tail (300), an exact chunk multiple (512), ViT-B/16
at 384 px (577), more than three chunks (785), a chunk multiple plus one
(1025); keys ramped along the sequence so the online-softmax maximum keeps
moving (or never moves); the long kernels forced onto short and padded
lengths; determinism; row-strided qkv; and the ViT block / model path."""
import functools
import math

import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import attention as A

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref(qkv, heads):
    b, s, d3 = qkv.shape
    d = d3 // 3
    hd = d // heads
    q, k, v = qkv.float().view(b, s, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    att = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    o = att.softmax(-1) @ v
    return o.transpose(1, 2).reshape(b, s, d)


@functools.lru_cache(maxsize=None)
def _case(B, S, H, ramp=0):
    """(qkv bf16, upstream gradient fp32, reference output, reference gradient): computed
    once per shape and shared, never modified.  ramp = +1 / -1 scales the K rows by a
    ramp from 0.25 to 2.0 along the sequence / the reverse."""
    torch.manual_seed(0)
    d = H * 64
    x = torch.randn(B, S, 3 * d, device=DEV) * 1.5
    if ramp:
        r = torch.linspace(0.25, 2.0, S, device=DEV)
        x[..., d:2 * d] *= (r if ramp > 0 else r.flip(0)).view(1, S, 1)
    qkv = x.bfloat16()
    ref_in = qkv.float().requires_grad_()
    ref = _ref(ref_in, H)
    go = torch.randn_like(ref)
    ref.backward(go)
    return qkv, go, ref.detach(), ref_in.grad


def _check(o, grad, case, H):
    _, _, ref, gr = case
    d = H * 64
    print(f"fwd max err {(o.float() - ref).abs().max().item():.4g}")
    torch.testing.assert_close(o.float(), ref, atol=2e-2, rtol=2e-2)
    g = grad.float().view_as(gr)
    for i in range(3):
        a, r = g[..., i * d:(i + 1) * d], gr[..., i * d:(i + 1) * d]
        err = (a - r).norm().item()
        bound = 2e-2 * r.norm().item() + 1e-3 * gr.norm().item()
        print(f"part {i}: err {err:.4g} bound {bound:.4g}")
        assert err <= bound, (i, err, r.norm().item())


def _run_packed(case, H):
    """Through the public op; asserts it took the native path exactly once."""
    qkv, go = case[0].clone().requires_grad_(), case[1]
    n0, t0 = A._STATS["native"], A._STATS["torch"]
    o = A.self_attention_packed(qkv, H)
    assert A._STATS["native"] == n0 + 1 and A._STATS["torch"] == t0, "long sequence left the native path"
    o.backward(go.bfloat16())
    return o.detach(), qkv.grad


@pytest.mark.parametrize("B,S,H", [(2, 257, 2), (1, 300, 2), (1, 512, 2), (2, 577, 3), (1, 785, 2), (1, 1025, 1)])
def test_long_attention_fwd_bwd(B, S, H):
    C = _native.require("attention test")
    assert C.attention_supported(S, 64) and C.get_attention_long_from() == 257
    case = _case(B, S, H)
    o, g = _run_packed(case, H)
    _check(o, g, case, H)


@pytest.mark.parametrize("ramp", [1, -1])
@pytest.mark.parametrize("B,S,H", [(2, 300, 2), (2, 577, 2)])
def test_long_attention_online_softmax_rescaling(B, S, H, ramp):
    _native.require("attention test")
    case = _case(B, S, H, ramp)
    o, g = _run_packed(case, H)
    _check(o, g, case, H)


@pytest.mark.parametrize("S", [1, 17, 64, 130, 197, 256])
def test_long_kernels_at_short_lengths(S):
    C = _native.require("attention test")
    B, H = 2, 2
    case = _case(B, S, H)
    o_short = A.self_attention_packed(case[0], H) if S == 197 else None
    old = C.get_attention_long_from()
    try:
        C.set_attention_long_from(1)
        o, g = _run_packed(case, H)
    finally:
        C.set_attention_long_from(old)
    _check(o, g, case, H)
    if o_short is not None:
        torch.testing.assert_close(o.float(), o_short.float(), atol=2e-2, rtol=2e-2)


def test_long_attention_is_deterministic():
    C = _native.require("attention test")
    B, S, H = 2, 577, 3
    qkv, go, _, _ = _case(B, S, H)
    q2, do = qkv.view(B * S, -1), go.bfloat16().view(B * S, -1)
    outs = []
    for _ in range(2):
        o, lse = C.attention_forward(q2, B, S, H, 0.125)
        outs.append((o, lse, C.attention_backward(do, q2, o, lse, B, S, H, 0.125)))
    (o0, l0, g0), (o1, l1, g1) = outs
    assert l0.shape == (B * H, 640)  # S rounded up to 64
    assert torch.equal(o0, o1) and torch.equal(l0[:, :S], l1[:, :S]) and torch.equal(g0, g1)


def test_long_attention_strided_qkv():
    C = _native.require("attention test")
    B, S, H = 1, 300, 2
    case = _case(B, S, H)
    d = H * 64
    wide = torch.full((B * S, 3 * d + 64), float("nan"), device=DEV, dtype=torch.bfloat16)
    q2 = wide[:, :3 * d]
    q2.copy_(case[0].view(B * S, 3 * d))
    assert q2.stride(0) == 3 * d + 64
    o, lse = C.attention_forward(q2, B, S, H, 0.125)
    g = C.attention_backward(case[1].bfloat16().view(B * S, d), q2, o, lse, B, S, H, 0.125)
    _check(o.view(B, S, d), g.view(B, S, 3 * d), case, H)


def test_long_attention_in_vit_block_and_model():
    from distributed_model_parallel_amd.models.vit import EncoderBlock, VisionTransformer
    _native.require("attention test")
    torch.manual_seed(1)
    blk = EncoderBlock(128, 2, 256).to(DEV).bfloat16()
    x = torch.randn(2, 290, 128, device=DEV).bfloat16()  # 272 px / 16-px patches: 17^2 + 1 tokens
    y = blk(x)
    with torch.no_grad():
        h = blk.ln1(x)
        qkv = blk.attn.qkv(h)
        ref = blk.attn.proj(_ref(qkv, 2).bfloat16())
    n0, t0 = A._STATS["native"], A._STATS["torch"]
    got = blk.attn(h)
    assert A._STATS["native"] == n0 + 1 and A._STATS["torch"] == t0
    torch.testing.assert_close(got.float(), ref.float(), atol=3e-2, rtol=3e-2)
    assert torch.isfinite(y).all()

    model = VisionTransformer(image_size=272, patch_size=16, num_layers=2, num_heads=2, hidden_dim=128,
                              mlp_dim=256, num_classes=10)
    torch.nn.init.normal_(model.head.weight, std=0.05)  # zero-initialised: it would zero every gradient below it
    model = model.to(DEV).bfloat16().train()
    img = torch.randn(2, 3, 272, 272, device=DEV).bfloat16()
    n0, t0 = A._STATS["native"], A._STATS["torch"]
    loss = torch.nn.functional.cross_entropy(model(img).float(), torch.tensor([1, 7], device=DEV))
    loss.backward()
    assert A._STATS["native"] == n0 + 2 and A._STATS["torch"] == t0
    assert torch.isfinite(loss).item()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.blocks[0].attn.qkv.weight.grad.abs().max().item() > 0
