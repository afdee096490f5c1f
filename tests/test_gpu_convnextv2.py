"""ConvNeXt V2 on the GPU against a plain-torch fp32 mirror with the published
GRN on NHWC, loaded from the same state dict: ConvNeXt((2, 2), (128, 256), 10,
grn=True) as in tests/test_gpu_convnext.py (bf16 channels-last, batch 256 at
32 px), zero 1-D parameters re-drawn so that GRN's gamma and beta carry data.
Bounds are those of tests/test_gpu_models.py::_compare."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_model_parallel_amd.models import convnext as CN
from distributed_model_parallel_amd.utils.precision import cast_model
from tests.convnext_mirror import Mirror, grads
from tests.test_gpu_models import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, PX, NCLS = 256, 32, 10


class _MirrorGRN(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma, self.beta = nn.Parameter(torch.zeros(dim)), nn.Parameter(torch.zeros(dim))

    def forward(self, x):  # NHWC
        gx = torch.norm(x, p=2, dim=(1, 2), keepdim=True)
        return self.gamma * (x * (gx / (gx.mean(dim=-1, keepdim=True) + 1e-6))) + self.beta + x


class _MirrorBlockV2(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dwconv, self.norm = nn.Conv2d(dim, dim, 7, padding=3, groups=dim), nn.LayerNorm(dim, eps=1e-6)
        self.fc1, self.grn, self.fc2 = nn.Linear(dim, 4 * dim), _MirrorGRN(4 * dim), nn.Linear(4 * dim, dim)

    def forward(self, x, scale=None):
        h = self.fc2(self.grn(F.gelu(self.fc1(self.norm(self.dwconv(x).permute(0, 2, 3, 1)))))).permute(0, 3, 1, 2)
        return x + (h if scale is None else scale.to(h.dtype).view(-1, 1, 1, 1) * h)


def _build(drop_path_rate, seed):
    torch.manual_seed(seed)
    src = CN.ConvNeXt((2, 2), (128, 256), num_classes=NCLS, drop_path_rate=drop_path_rate, grn=True).to(DEV)
    with torch.no_grad():
        for n, p in src.named_parameters():
            if p.dim() == 1 and float(p.abs().sum()) == 0:
                p.normal_(std=0.5 if ".grn." in n else 0.02)
    nat = cast_model(copy.deepcopy(src), torch.bfloat16, keep_batchnorm_fp32=False)
    nat = nat.to(memory_format=torch.channels_last).train()
    ref = Mirror(nat.depths, nat.dims, NCLS, 3)
    ref.stages = nn.ModuleList(nn.ModuleList(_MirrorBlockV2(d) for _ in range(n)) for n, d in zip(nat.depths, nat.dims))
    ref.load_state_dict({k: v.detach().float() for k, v in nat.state_dict().items()})
    x = torch.randn(B, 3, PX, PX, device=DEV).contiguous(memory_format=torch.channels_last)
    return nat, ref.to(DEV).train(), x, torch.randint(0, NCLS, (B,), device=DEV)


@pytest.mark.parametrize("drop_path", [False, True])
def test_model_matches_the_fp32_mirror(drop_path, monkeypatch):
    nat, ref, x, y = _build(0.3 if drop_path else 0.0, int(drop_path))
    scales = None
    if drop_path:  # fixed per-sample scales; block 0 has rate 0: no draw
        gen = torch.Generator(device="cpu").manual_seed(3)
        scales = [None] + [((torch.rand(B, generator=gen) < 0.7).float() / 0.7).to(DEV) for _ in range(3)]
        it = iter(scales[1:])
        monkeypatch.setattr(CN, "sample_scales", lambda n, batch, rate, device: next(it).view(1, B))
    l_nat, g_nat = grads(nat, x.bfloat16(), y)
    l_ref, g_ref = grads(ref, x, y, scales=scales)
    assert set(g_nat) == set(g_ref) and sum(".grn." in n for n in g_ref) == 8
    _compare(l_nat, g_nat, l_ref, g_ref)


def test_v2_block_under_graph_capture_equals_eager():
    """One V2 block's forward + backward captured and replayed twice: bitwise the eager result."""
    torch.manual_seed(4)
    blk = CN.ConvNeXtBlock(128, grn=True).to(DEV).bfloat16().train()
    with torch.no_grad():
        blk.grn.gamma.normal_()
        blk.grn.beta.normal_()
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
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, [y] + list(grads_)):
            assert torch.equal(a, b)
