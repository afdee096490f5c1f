"""ConvNeXt on the native routes against a plain-torch fp32 mirror
(tests/convnext_mirror.py) loaded from the same state dict.

Model: ConvNeXt(depths=(2, 2), dims=(128, 256), 10 classes), bf16
channels-last, batch 256 at 32 px: 8 x 8 tokens per image after the stem
(16384 rows) and 4 x 4 in the second stage (4096 rows, the fused GEMM path's
minimum), so every native route is taken in both stages.  Bounds are
those of tests/test_gpu_models.py::_compare: every parameter's gradient cosine
>= 0.95 and norm ratio in (0.9, 1.1), median cosine >= 0.99."""
import copy

import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd.models import convnext as CN
from distributed_model_parallel_amd.ops import depthwise7, layernorm, linear, patch_embed
from distributed_model_parallel_amd.utils.precision import cast_model
from tests.convnext_mirror import grads, mirror_of
from tests.test_gpu_models import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, PX, NCLS = 256, 32, 10


def _build(layer_scale, drop_path_rate=0.0, seed=0):
    torch.manual_seed(seed)
    ref_src = CN.ConvNeXt((2, 2), (128, 256), num_classes=NCLS, layer_scale=layer_scale,
                          drop_path_rate=drop_path_rate).to(DEV)
    with torch.no_grad():  # non-zero biases, so their gradients' paths carry data too
        for p in ref_src.parameters():
            if p.dim() == 1 and float(p.abs().sum()) == 0:
                p.normal_(std=0.02)
    nat = cast_model(copy.deepcopy(ref_src), torch.bfloat16, keep_batchnorm_fp32=False)
    nat = nat.to(memory_format=torch.channels_last).train()
    ref = mirror_of(nat).train()  # the mirror holds the bf16-rounded weights, in fp32
    x = torch.randn(B, 3, PX, PX, device=DEV).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, NCLS, (B,), device=DEV)
    return nat, ref, x, y


def _counters():
    return {"dw": depthwise7._STATS["native"], "dw_torch": depthwise7._STATS["torch"],
            "dw_res": depthwise7._STATS["fused_residual_grad"], "xl": linear._STATS["xl"],
            "pe": patch_embed._STATS["native"], "pe_torch": patch_embed._STATS["torch"],
            "ln": layernorm._STATS["native"], "ln_torch": layernorm._STATS["torch"]}


@pytest.fixture(scope="module")
def case():
    """One native run and one mirror run at layer_scale = 1, shared."""
    nat, ref, x, y = _build(1.0)
    c0 = _counters()
    l_nat, g_nat = grads(nat, x.bfloat16(), y)
    used = {k: v - c0[k] for k, v in _counters().items()}
    l_ref, g_ref = grads(ref, x, y)
    return dict(nat=nat, ref=ref, x=x, y=y, l_nat=l_nat, g_nat=g_nat, l_ref=l_ref, g_ref=g_ref, used=used)


def test_every_native_route_is_taken(case):
    u = case["used"]
    assert u["dw"] == 4 and u["dw_torch"] == 0 and u["dw_res"] == 4, u
    assert u["xl"] == 4, u
    assert u["pe"] == 2 and u["pe_torch"] == 0, u
    assert u["ln"] == 7 and u["ln_torch"] == 0, u  # stem, 1 downsample, 4 blocks, head


def test_loss_and_gradients_match_the_fp32_mirror(case):
    assert set(case["g_nat"]) == set(case["g_ref"])
    _compare(case["l_nat"], case["g_nat"], case["l_ref"], case["g_ref"])


def test_layer_scale_1e6_gamma_gradients():
    """At the published init gamma = 1e-6 the branch barely reaches the loss;
    gamma's own gradient does not depend on gamma's size and is checked alone."""
    nat, ref, x, y = _build(1e-6, seed=1)
    _, g_nat = grads(nat, x.bfloat16(), y)
    _, g_ref = grads(ref, x, y)
    names = [n for n in g_ref if n.endswith("gamma")]
    assert len(names) == 4
    for n in names:
        cos = F.cosine_similarity(g_nat[n].flatten(), g_ref[n].flatten(), dim=0).item()
        print(f"{n}: cos {cos:.4f}")
        assert cos >= 0.95, f"{n}: cos={cos:.4f}"


def test_fixed_drop_path_scales_match_the_mirror(monkeypatch):
    nat, ref, x, y = _build(1.0, drop_path_rate=0.3, seed=2)
    g = torch.Generator(device="cpu").manual_seed(3)
    keep = 0.7
    scales = [((torch.rand(B, generator=g) < keep).float() / keep).to(DEV) for _ in range(4)]
    assert all(0 < int((s == 0).sum()) < B for s in scales)
    it = iter(scales[1:])  # block 0 has rate 0: no draw

    def fixed(n, batch, rate, device):
        assert n == 1 and batch == B
        return next(it).view(1, B)

    monkeypatch.setattr(CN, "sample_scales", fixed)
    xl0 = linear._STATS["xl"]
    l_nat, g_nat = grads(nat, x.bfloat16(), y)
    assert linear._STATS["xl"] == xl0 + 4  # the scaled blocks stay on the fused route
    l_ref, g_ref = grads(ref, x, y, scales=[None] + scales[1:])
    _compare(l_nat, g_nat, l_ref, g_ref)


def test_block_under_graph_capture_equals_eager():
    """One block's forward + backward captured and replayed: bitwise the eager result."""
    torch.manual_seed(4)
    blk = CN.ConvNeXtBlock(128, layer_scale=1.0).to(DEV).bfloat16().train()
    x = torch.randn(64, 64, 128, device=DEV).bfloat16().requires_grad_()
    gy = torch.randn(64, 64, 128, device=DEV).bfloat16()

    def run():
        for p in blk.parameters():
            p.grad = None
        x.grad = None
        y = blk(x, (8, 8))
        y.backward(gy)
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in blk.parameters()]

    eager = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = blk(x, (8, 8))
        grads_ = torch.autograd.grad(y, [x] + list(blk.parameters()), gy)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, [y] + list(grads_)):
        assert torch.equal(a, b)


def test_depthwise_through_torch_passes_the_same_comparison(case):
    """set_enabled(False): the A/B arm computes the same thing."""
    nat = case["nat"]
    depthwise7.set_enabled(False)
    try:
        t0 = depthwise7._STATS["torch"]
        l_ab, g_ab = grads(nat, case["x"].bfloat16(), case["y"])
        assert depthwise7._STATS["torch"] == t0 + 4
    finally:
        depthwise7.set_enabled(True)
    _compare(l_ab, g_ab, case["l_ref"], case["g_ref"])
