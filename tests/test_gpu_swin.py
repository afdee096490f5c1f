"""Swin on the GPU: a two-stage model (dims 128 / 256, heads 4 / 8, window 7,
56 px: a 14 x 14 grid with shifted blocks, then one window) in bf16 on the
native LayerNorm / GEMM route against its fp32 copy on stock PyTorch ops
(_native.reference_mode), within tests/test_gpu_models.py::_compare's bounds.
Shifted-window attention runs the torch composition on both sides."""
import copy

import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.models.swin import SwinTransformer
from distributed_model_parallel_amd.ops import linear, window_attention as WA
from tests.test_gpu_models import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grads(m, x, y):
    m.zero_grad()
    loss = F.cross_entropy(m(x).float(), y)
    loss.backward()
    return loss.item(), {n: p.grad.float().clone() for n, p in m.named_parameters()}


def test_model_matches_its_fp32_copy_on_stock_ops():
    torch.manual_seed(0)
    ref = SwinTransformer(4, 128, (2, 2), (4, 8), 7, num_classes=10).to(DEV).train()
    with torch.no_grad():
        for b in ref.blocks:
            b.attn.relative_position_bias_table.normal_(std=0.5)
    nat = copy.deepcopy(ref).bfloat16()
    ref.load_state_dict({k: v.float() for k, v in nat.state_dict().items()})
    x = torch.randn(32, 3, 56, 56, device=DEV)
    y = torch.randint(0, 10, (32,), device=DEV)
    xl0, t0 = linear._STATS["xl"], WA._STATS["torch"]
    l_nat, g_nat = _grads(nat, x.bfloat16(), y)
    assert linear._STATS["xl"] >= xl0 + 4  # proj and the MLP of stage 1's blocks (6272 rows) on the fused-epilogue GEMMs
    assert WA._STATS["torch"] == t0 + 4
    with _native.reference_mode():
        l_ref, g_ref = _grads(ref, x, y)
    assert set(g_nat) == set(g_ref)
    _compare(l_nat, g_nat, l_ref, g_ref)
