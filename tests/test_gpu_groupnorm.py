"""Native GroupNorm (csrc/norm/groupnorm.hip) against an fp64 reference formed
from the same bf16 / fp32 inputs, on shapes that groupnorm_plan puts on the
edges of the work split; then one MobileNetV2 and one ResNet block with GN
against their fp32 copies on stock ops, and the ResNet block under graph capture.

Bounds (n = elements per group, rows = N * HW):
  y, dx      |err| <= rel * |ref| + n * 2^-24 * max|ref|, rel = 2^-8 for bf16
             storage (one rounding, 2^-9, with a factor two), 2^-22 for fp32;
  dgamma, dbeta  |err| <= rows * 2^-24 * sum|summand|.
An element whose fp64 pre-activation lies within that y bound of a clip point
(0, or 6 for ReLU6) may fall on either side of the mask: the reference takes
the side the kernel took (read from dres), every other element must have the
reference's side, and such elements are under 1 % (a condition on the
inputs: gamma = 1.5 and beta in {-4, 3, 10} per channel put a third of the
values below 0, a third above 6 and little mass at the clip points).

The plan never yields a streamed sample of one block: a sample whose rows fit
one block's LDS is resident by construction, so that case has no shape."""
import copy

import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.models.mobilenetv2 import InvertedResidual
from distributed_model_parallel_amd.models.resnet import Bottleneck
from distributed_model_parallel_amd.ops import groupnorm as GN
from distributed_model_parallel_amd.utils.precision import cast_model
from tests.test_gpu_models import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")


def _plan(n, hw, c, g, dtype=torch.bfloat16):
    return _native.require("test").groupnorm_plan(n, hw, c, g, dtype)


def _edge_hw(c, g):
    """The largest HW that is still resident for (c, g) in bf16."""
    lo, hi = 1, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _plan(1, mid, c, g)["path"] == 0 else (lo, mid)
    return lo


def _k_hw(k):
    """An HW at which C = 192, G = 24 runs k groups per block (a last block with fewer)."""
    return next(hw for hw in range(64, 2048) if _plan(1, hw, 192, 24)["groups_per_block"] == k)


# name -> (N, HW, C, G, path, offset); HW may be a callable evaluated on the GPU machine's plan
CASES = {
    "resident_cg8": (3, 49, 64, 8, 0, 0.0),
    "resident_cg2": (2, 25, 64, 32, 0, 0.0),
    "resident_cg4": (2, 25, 128, 32, 0, 0.0),
    "resident_cg1": (2, 9, 16, 16, 0, 0.0),
    "resident_k7": (2, lambda: _k_hw(7), 192, 24, 0, 0.0),
    "resident_k5": (1, lambda: _k_hw(5), 192, 24, 0, 0.0),
    "hw1": (4, 1, 64, 4, 0, 0.0),
    "hw169": (2, 169, 64, 8, 0, 0.0),
    "hw251": (2, 251, 32, 32, 0, 0.0),
    "resident_edge": (1, lambda: _edge_hw(64, 8), 64, 8, 0, 0.0),
    "streamed_edge": (2, lambda: _edge_hw(64, 8) + 1, 64, 8, 1, 0.0),
    "streamed_cg2_wide": (1, lambda: _edge_hw(1024, 512) + 3, 1024, 512, 1, 0.0),
    "resident_offset": (2, 169, 64, 8, 0, 100.0),
    "streamed_offset": (1, lambda: _edge_hw(64, 32) + 77, 64, 32, 1, 100.0),
}


def _ref_forward(x, w, b, res, G, eps, clip):
    """fp64: xhat, rstd, the pre-activation and y."""
    N, HW, C = x.shape
    xg = x.view(N, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = ((xg - mean).square().mean((1, 3), keepdim=True) + eps).rsqrt()
    xhat = ((xg - mean) * rstd).view(N, HW, C)
    pre = xhat * w + b + (res if res is not None else 0)
    return xhat, rstd, pre, (pre if clip is None else pre.clamp(0, clip))


def _ref_backward(dz, xhat, rstd, w, G):
    """fp64: dx, dgamma, dbeta and the sums of absolute summands, from the masked gradient."""
    N, HW, C = dz.shape
    gg, xh = (dz * w).view(N, HW, G, C // G), xhat.view(N, HW, G, C // G)
    c1, c2 = gg.mean((1, 3), keepdim=True), (gg * xh).mean((1, 3), keepdim=True)
    return dict(dx=(rstd * (gg - c1 - xh * c2)).view(N, HW, C), dgamma=(dz * xhat).sum((0, 1)),
                dbeta=dz.sum((0, 1)), agamma=(dz * xhat).abs().sum((0, 1)), abeta=dz.abs().sum((0, 1)))


@pytest.mark.parametrize("name", list(CASES))
def test_native_against_fp64(name):
    C_ = _native.require("test")
    N, HW, C, G, path, offset = CASES[name]
    HW = HW() if callable(HW) else HW
    n, rows, eps = HW * (C // G), N * HW, 1e-5
    assert n <= (1 << 15) + 8 * (C // G)
    gen = torch.Generator().manual_seed(len(name) + HW)
    w = torch.full((C,), 1.5, device=DEV)
    b = torch.tensor([-4.0, 3.0, 10.0], device=DEV).repeat(C)[torch.randperm(3 * C, generator=gen)[:C].to(DEV)]
    base = (torch.randn(4, N, HW, C, generator=gen)).to(DEV)
    for dtype, rel in ((torch.bfloat16, 2.0 ** -8), (torch.float32, 2.0 ** -22)):
        plan = _plan(N, HW, C, G, dtype)
        if dtype == torch.bfloat16:
            assert plan["path"] == path, plan
            if name.startswith("resident_k"):
                assert plan["groups_per_block"] == int(name[-1]) and G % plan["groups_per_block"] != 0, plan
            if path == 1:
                assert HW % plan["rows_per_block"] != 0 and plan["blocks"] > N, plan
        x = (base[0] * (1 + 0.5 * torch.tanh(base[3][:, :1, :1])) + offset).to(dtype)   # per-sample scale: statistics differ
        res, dy = base[1].to(dtype), base[2].to(dtype)
        for clip in (None, INF, 6.0):
            for r in (None, res):
                rd = None if r is None else r.double()
                xhat, rstd64, pre, y_ref = _ref_forward(x.double(), w.double(), b.double(), rd, G, eps, clip)
                act = clip is not None
                y, mean, rstd = C_.groupnorm_forward(x, w, b, r, G, eps, act, clip if act else INF)
                saved = y if (act and r is not None) else None
                out = C_.groupnorm_backward(dy, x, saved, w, b, mean, rstd, G, act, clip if act else INF,
                                            True, torch.float32)
                tag = (name, dtype, clip, r is not None)

                def bound(t):
                    return rel * t.abs() + n * 2.0 ** -24 * t.abs().max()

                assert ((y.double() - y_ref).abs() <= bound(y_ref)).all(), tag
                dz = dy.double()
                if act:  # elements near a clip point keep the side the kernel took; all others the reference's
                    near = torch.zeros_like(pre, dtype=torch.bool)
                    for c in (0.0,) if clip == INF else (0.0, clip):
                        near |= (pre - c).abs() <= rel * abs(c) + n * 2.0 ** -24 * pre.abs().max()
                    assert near.double().mean() < 0.01, tag
                    clipped = ((pre <= 0).double().mean(), (pre >= clip).double().mean())
                    assert clipped[0] > 0.1 and (clip == INF or clipped[1] > 0.1), (tag, clipped)
                    got = out[3].double()
                    assert ((got[near] == 0) | (got[near] == dz[near])).all(), tag
                    dz = torch.where(near, got, dz * ((pre > 0) & (pre < clip)))
                assert torch.equal(out[3].double(), dz), tag
                ref = _ref_backward(dz, xhat, rstd64, w.double(), G)
                assert ((out[0].double() - ref["dx"]).abs() <= bound(ref["dx"])).all(), tag
                for k, a, o in (("dgamma", "agamma", out[1]), ("dbeta", "abeta", out[2])):
                    assert ((o.double() - ref[k]).abs() <= rows * 2.0 ** -24 * ref[a]).all(), (tag, k)
                # a second run on the same inputs: bit-identical
                y2, mean2, rstd2 = C_.groupnorm_forward(x, w, b, r, G, eps, act, clip if act else INF)
                out2 = C_.groupnorm_backward(dy, x, saved, w, b, mean, rstd, G, act, clip if act else INF,
                                             True, torch.float32)
                assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2), tag
                assert all(torch.equal(p, q) for p, q in zip(out, out2)), tag


def _block(kind, px=8, batch=4):
    torch.manual_seed(7)
    if kind == "inverted_residual":
        blk, x = InvertedResidual(32, 32, 6, 1, norm="gn"), torch.randn(4, 32, 8, 8)
    else:
        blk, x = Bottleneck(256, 64, norm="gn"), torch.randn(batch, 256, px, px)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.normal_(1.0 if float(p.sum()) != 0 else 0.0, 0.2)
    ref = copy.deepcopy(blk).to(DEV).train()
    nat = cast_model(blk.to(DEV), torch.bfloat16, keep_batchnorm_fp32=False).to(memory_format=torch.channels_last)
    return nat.train(), ref, x.to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("kind", ["inverted_residual", "bottleneck"])
def test_block_matches_its_fp32_copy(kind):
    nat, ref, x = _block(kind)
    before = GN.stats()
    xn = x.bfloat16().requires_grad_()
    yn = nat(xn)
    assert GN.stats()["native_fwd"] - before["native_fwd"] == 3 and GN.stats()["torch_fwd"] == before["torch_fwd"]
    ln = yn.float().square().mean()
    ln.backward()
    xr = x.clone().requires_grad_()
    with _native.reference_mode():
        lr = ref(xr).square().mean()
        lr.backward()
    g_nat = dict({k: p.grad.float() for k, p in nat.named_parameters()}, x=xn.grad.float())
    g_ref = dict({k: p.grad for k, p in ref.named_parameters()}, x=xr.grad)
    _compare(ln.item(), g_nat, lr.item(), g_ref)


def test_bottleneck_under_graph_capture_equals_eager():
    """Forward + backward captured and replayed twice: bitwise the eager result.

    On ResNet-50's layer-1 map (56 x 56), where the 3x3 conv runs the halo
    kernels both eagerly and under capture: a captured conv never takes the
    library (ops/conv_igemm.py _capturing), so at a map the library serves
    eagerly the two runs would compare different conv kernels, not GroupNorm."""
    nat, _, x = _block("bottleneck", px=56, batch=2)
    x = x.bfloat16().requires_grad_()
    gy = torch.randn(2, 256, 56, 56, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)

    def run():
        for p in nat.parameters():
            p.grad = None
        x.grad = None
        y = nat(x)
        y.backward(gy)
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in nat.parameters()]

    eager = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = nat(x)
        grads_ = torch.autograd.grad(y, [x] + list(nat.parameters()), gy)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, [y] + list(grads_)):
            assert torch.equal(a, b)
