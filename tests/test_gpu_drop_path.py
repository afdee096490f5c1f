"""Stochastic depth on the GPU: the gemm_xl "bias_res_scale" epilogue (bitwise
against "bias_res" and against its rounding contract), the rowscale_bias_grad
side pass, linear_residual / mlp_residual with a per-sample scale against fp32
autograd, the ViT model on the fused and the unfused route, and fresh masks
at every replay of a captured graph.

Scales are explicit vectors (kept and dropped samples by construction); the
shapes are the smallest at which the row -> sample index can go wrong: T does
not divide the tile height, samples straddle tile edges, M has a tail."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import drop_path as DP
from distributed_model_parallel_amd.ops import linear as L

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, T, N, K): 300 rows in 256-row tiles; ViT's 197 tokens, 3 column tiles; one
# sample over more than two tiles; T = 1 on the 256 x 128 tile
SHAPES = [(6, 50, 256, 64), (7, 197, 768, 128), (3, 577, 256, 64), (300, 1, 128, 64)]
GENERAL = [0.0, 1.0, 0.0, 1.25, 1.0, 0.0, 3.0]
# (bm, (bn, pipe)): default 4-wave kernel; its 224-row tiles; the 8-wave
# ping-pong; the 128-wide ring
DEFAULT, BM224, PIPE10, BN128 = (0, None), (224, None), (0, (256, 10)), (0, (128, 1))
ROUTES = [(s, DEFAULT) for s in SHAPES] + [(s, BM224) for s in SHAPES] + [(SHAPES[1], PIPE10), (SHAPES[1], BN128)]


def C():
    return _native.require("drop path test")


def _cycle(vals, n):
    return torch.tensor([vals[i % len(vals)] for i in range(n)], dtype=torch.float32, device=DEV)


_OPERANDS = {}


def _operands(shape):
    """A, W, bias, residual of one shape: made once, shared, never written."""
    if shape not in _OPERANDS:
        b, t, n, k = shape
        g = torch.Generator(device=DEV).manual_seed(b * 1000 + t)
        a = torch.randn(b * t, k, device=DEV, generator=g).bfloat16()
        w = (torch.randn(n, k, device=DEV, generator=g) * k ** -0.5).bfloat16()
        bias = torch.randn(n, device=DEV, generator=g).bfloat16()
        res = torch.randn(b * t, n, device=DEV, generator=g).bfloat16()
        _OPERANDS[shape] = (a, w, bias, res)
    return _OPERANDS[shape]


@pytest.fixture
def route(request):
    bm, bn = request.param
    c = C()
    old = c.get_gemm_xl_pipe()
    try:
        c.set_gemm_xl_bm(bm)
        if bn is not None:
            c.set_gemm_xl_bn(*bn)
        yield request.param
    finally:
        c.set_gemm_xl_bm(0)
        c.set_gemm_xl_bn(0, old)


# ---------------------------------------------------------------- 1. epilogue, bitwise
@pytest.mark.parametrize("shape,route", ROUTES, indirect=["route"])
def test_epilogue_bitwise_against_bias_res(shape, route):
    b, t, n, k = shape
    a, w, bias, res = _operands(shape)
    plain = C().gemm_xl(a, w, "bias_res", bias=bias, residual=res)
    ones = C().gemm_xl(a, w, "bias_res_scale", bias=bias, residual=res,
                       row_scale=torch.ones(b, device=DEV), rows_per_sample=t)
    assert torch.equal(ones, plain)
    s = _cycle([0.0, 1.0, 1.0, 0.0, 0.0], b)
    y = C().gemm_xl(a, w, "bias_res_scale", bias=bias, residual=res, row_scale=s, rows_per_sample=t)
    keep = s.bool().repeat_interleave(t)
    assert keep.any() and not keep.all()
    assert torch.equal(y[keep], plain[keep])
    assert torch.equal(y[~keep], res[~keep])


# ---------------------------------------------------------------- 2. epilogue, general scales
@pytest.mark.parametrize("shape,route", ROUTES, indirect=["route"])
def test_epilogue_general_scales_match_the_rounding_contract(shape, route):
    b, t, n, k = shape
    a, w, bias, res = _operands(shape)
    s = _cycle(GENERAL, b)
    y = C().gemm_xl(a, w, "bias_res_scale", bias=bias, residual=res, row_scale=s, rows_per_sample=t)
    staged = (a.float() @ w.float().t() + bias.float()).bfloat16()
    ref = (staged.float() * s.repeat_interleave(t)[:, None] + res.float()).bfloat16()
    torch.testing.assert_close(y.float(), ref.float(), atol=0.05, rtol=2e-2)


def test_epilogue_argument_checks():
    a, w, bias, res = _operands(SHAPES[0])
    kw = dict(bias=bias, residual=res)
    with pytest.raises(RuntimeError, match="row_scale"):
        C().gemm_xl(a, w, "bias_res_scale", **kw)
    with pytest.raises(RuntimeError, match="row_scale"):
        C().gemm_xl(a, w, "bias_res_scale", row_scale=torch.ones(6, device=DEV).double(), rows_per_sample=50, **kw)
    with pytest.raises(RuntimeError, match="row_scale"):
        C().gemm_xl(a, w, "bias_res_scale", row_scale=torch.ones(6), rows_per_sample=50, **kw)
    with pytest.raises(RuntimeError, match="rows_per_sample"):
        C().gemm_xl(a, w, "bias_res_scale", row_scale=torch.ones(6, device=DEV), rows_per_sample=0, **kw)
    with pytest.raises(RuntimeError, match="rows_per_sample"):
        C().gemm_xl(a, w, "bias_res_scale", row_scale=torch.ones(7, device=DEV), rows_per_sample=50, **kw)


# ---------------------------------------------------------------- 3. backward side pass
# tests/test_gpu_linear.py's bias-gradient (M, N) as (B, T, N), then ViT's 197
# tokens, T = 1 and a sample longer than a block's row chunk
@pytest.mark.parametrize("B,T,N", [(128, 197, 768), (125, 8, 2304), (1, 37, 3072), (1, 1, 256), (4099, 1, 512),
                                   (7, 197, 768), (300, 1, 256), (3, 577, 512)])
def test_rowscale_bias_grad(B, T, N):
    M = B * T
    dy = torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(M)).bfloat16()
    s = _cycle(GENERAL[3:] + GENERAL[:3], B)  # (1.25 first: the one-sample cases are scaled too)
    want = (dy.float() * s.repeat_interleave(T)[:, None]).bfloat16()
    ref = want.float().sum(0)
    for dt in (torch.bfloat16, torch.float32):
        g, db = C().rowscale_bias_grad(dy, s, T, dt)
        assert db.dtype == dt and g.dtype == torch.bfloat16
        assert torch.equal(g, want)
        # the bound of test_gpu_linear.py::test_bias_grad, against the sum of the stored g
        torch.testing.assert_close(db.float(), ref, atol=2e-2 * (M ** 0.5) / 10 + 1e-2, rtol=1e-2)
    g, db = C().rowscale_bias_grad(dy, torch.ones(B, device=DEV), T, torch.float32)
    assert torch.equal(g, dy)
    assert torch.equal(db, C().bias_grad(dy, torch.float32))  # same grid, same order of sums
    with pytest.raises(RuntimeError, match="rows_per_sample"):
        C().rowscale_bias_grad(dy, s, T + 1, torch.float32)


# ---------------------------------------------------------------- 4. ops level
OB, OT, OD, OH = 21, 197, 256, 1024  # 4137 rows: the smallest ViT-shaped count past _XL_MIN_ROWS


def _leaves(*ts):
    return [t.detach().clone().requires_grad_() for t in ts]


def _run_linear(proj, x, res, g, s):
    xb, rb = _leaves(x, res)
    proj.zero_grad()
    y = L.linear_residual(xb, rb, proj.weight, proj.bias, s)
    y.backward(g)
    return [y.detach(), xb.grad, rb.grad, proj.weight.grad.clone(), proj.bias.grad.clone()]


def _run_mlp(fc1, fc2, x, res, g, s):
    xb, rb = _leaves(x, res)
    fc1.zero_grad()
    fc2.zero_grad()
    y = L.mlp_residual(xb, rb, fc1, fc2, 0.0, True, s)
    y.backward(g)
    return [y.detach(), xb.grad, rb.grad] + [p.grad.clone() for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]


@pytest.fixture
def xl_on(monkeypatch):
    monkeypatch.setattr(L, "_XL", True)
    monkeypatch.setattr(DP, "_FUSED", True)


def test_linear_residual_row_scale_matches_fp32(xl_on):
    assert OB * OT >= L._XL_MIN_ROWS > (OB - 1) * OT
    torch.manual_seed(1)
    proj = nn.Linear(OD, OD).to(DEV).bfloat16()
    x = torch.randn(OB, OT, OD, device=DEV).bfloat16()
    res = torch.randn(OB, OT, OD, device=DEV).bfloat16()
    g = torch.randn(OB, OT, OD, device=DEV)
    s = _cycle(GENERAL, OB)
    n0 = L._STATS["xl"]
    y, dx, dr, dw, db = _run_linear(proj, x, res, g.bfloat16(), s)
    assert L._STATS["xl"] == n0 + 1, "fused path not taken"
    xf, rf, w, b = _leaves(x.float(), res.float(), proj.weight.float(), proj.bias.float())
    yr = rf + s.view(OB, 1, 1) * F.linear(xf, w, b)
    yr.backward(g)
    rows = OB * OT
    # the tolerances of test_gpu_vit_xl.py::test_linear_residual_matches_fp32
    torch.testing.assert_close(y.float(), yr, atol=0.05, rtol=2e-2)
    torch.testing.assert_close(dx.float(), xf.grad, atol=0.1, rtol=3e-2)
    torch.testing.assert_close(dw.float(), w.grad, atol=0.02 * rows ** 0.5, rtol=3e-2)
    torch.testing.assert_close(db.float(), b.grad, atol=0.02 * rows ** 0.5, rtol=3e-2)
    assert torch.equal(dr, g.bfloat16())  # the residual's gradient is the upstream gradient itself
    dropped = s == 0
    assert dropped.any() and torch.count_nonzero(dx[dropped]) == 0 and torch.count_nonzero(dx[~dropped]) > 0
    # s == 1: the bits of the call without a scale (the side pass sums in bias_grad's order)
    plain = _run_linear(proj, x, res, g.bfloat16(), None)
    ones = _run_linear(proj, x, res, g.bfloat16(), torch.ones(OB, device=DEV))
    assert L._STATS["xl"] == n0 + 3
    for name, p, o in zip(("y", "dx", "dres", "dw", "db"), plain, ones):
        assert torch.equal(p, o), name


def test_mlp_residual_row_scale_matches_fp32(xl_on):
    torch.manual_seed(0)
    fc1, fc2 = nn.Linear(OD, OH).to(DEV).bfloat16(), nn.Linear(OH, OD).to(DEV).bfloat16()
    x = torch.randn(OB, OT, OD, device=DEV).bfloat16()
    res = torch.randn(OB, OT, OD, device=DEV).bfloat16()
    g = torch.randn(OB, OT, OD, device=DEV)
    s = _cycle(GENERAL, OB)
    n0 = L._STATS["xl"]
    y, dx, dr, dw1, db1, dw2, db2 = _run_mlp(fc1, fc2, x, res, g.bfloat16(), s)
    assert L._STATS["xl"] == n0 + 1, "fused path not taken"
    xf, rf, w1, b1, w2, b2 = _leaves(x.float(), res.float(), fc1.weight.float(), fc1.bias.float(),
                                     fc2.weight.float(), fc2.bias.float())
    yr = rf + s.view(OB, 1, 1) * F.linear(F.gelu(F.linear(xf, w1, b1)), w2, b2)
    yr.backward(g)
    rows = OB * OT
    # the tolerances of test_gpu_vit_xl.py::test_mlp_residual_matches_fp32
    torch.testing.assert_close(y.float(), yr, atol=0.05, rtol=2e-2)
    torch.testing.assert_close(dx.float(), xf.grad, atol=0.05 * OH ** 0.5 / 8, rtol=3e-2)
    for got, ref in ((dw1, w1.grad), (dw2, w2.grad), (db1, b1.grad), (db2, b2.grad)):
        torch.testing.assert_close(got.float(), ref, atol=0.02 * rows ** 0.5, rtol=3e-2)
    assert torch.equal(dr, g.bfloat16())
    dropped = s == 0
    assert torch.count_nonzero(dx[dropped]) == 0 and torch.count_nonzero(dx[~dropped]) > 0
    plain = _run_mlp(fc1, fc2, x, res, g.bfloat16(), None)
    ones = _run_mlp(fc1, fc2, x, res, g.bfloat16(), torch.ones(OB, device=DEV))
    for name, p, o in zip(("y", "dx", "dres", "dw1", "db1", "dw2", "db2"), plain, ones):
        assert torch.equal(p, o), name


def test_unfused_switch_runs_torch_ops(monkeypatch):
    monkeypatch.setattr(L, "_XL", True)
    monkeypatch.setattr(DP, "_FUSED", False)
    torch.manual_seed(2)
    proj = nn.Linear(OD, OD).to(DEV).bfloat16()
    x = torch.randn(OB, OT, OD, device=DEV).bfloat16()
    n0 = L._STATS["xl"]
    s = _cycle(GENERAL, OB)
    y = L.linear_residual(x, x, proj.weight, proj.bias, s)
    assert L._STATS["xl"] == n0
    ref = x.float() + s.view(OB, 1, 1) * F.linear(x.float(), proj.weight.float(), proj.bias.float())
    torch.testing.assert_close(y.float(), ref, atol=0.05, rtol=2e-2)


# ---------------------------------------------------------------- 5. model level
def test_vit_fused_route_matches_unfused(monkeypatch):
    from distributed_model_parallel_amd.models.vit import VisionTransformer
    monkeypatch.setattr(L, "_XL", True)
    B = 21
    torch.manual_seed(0)
    model = VisionTransformer(224, 16, 2, 4, 256, 1024, 10, drop_path_rate=0.5)
    with torch.no_grad():  # the head starts at zero: the logits would not depend on the blocks
        model.head.weight.normal_(std=0.05)
    model = model.to(DEV).bfloat16().to(memory_format=torch.channels_last).train()
    assert [blk.drop_path for blk in model.blocks] == [0.0, 0.5]
    x = torch.randn(B, 3, 224, 224, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    gw = torch.randn(B, 10, device=DEV)
    # block 1's draw is the first random call after the seed (block 0 has rate 0):
    # both of its rows must hold kept and dropped samples
    torch.manual_seed(0)
    draw = DP.sample_scales(2, B, 0.5, DEV)
    assert all(0 < int((row == 0).sum()) < B for row in draw), draw

    def run(fused):
        monkeypatch.setattr(DP, "_FUSED", fused)
        model.zero_grad()
        n0 = L._STATS["xl"]
        torch.manual_seed(0)
        out = model(x)
        (out.float() * gw).sum().backward()
        return L._STATS["xl"] - n0, [out.detach().float()] + [p.grad.detach().float().clone()
                                                             for p in model.parameters()]

    n_fused, fused = run(True)
    assert n_fused == 4, "proj / fc2 of both blocks must run on the fused-epilogue GEMM"
    n_plain, plain = run(False)
    assert n_plain == 2  # block 0 (rate 0) only
    names = ["logits"] + [n for n, _ in model.named_parameters()]
    for name, a, b in zip(names, fused, plain):
        assert b.norm() > 0, name
        err = ((a - b).norm() / b.norm()).item()
        assert err < 2e-2, (name, err)  # the bound of test_weight_grads_on_tn_kernel_match_fp32


# ---------------------------------------------------------------- 6. graph replay
def test_captured_draw_is_fresh_at_every_replay():
    out = torch.empty(2, 64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out.copy_(DP.sample_scales(2, 64, 0.5, DEV))  # eager warm-up, as train/graphed.py does
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.copy_(DP.sample_scales(2, 64, 0.5, DEV))
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1])
    for s in seen:
        assert bool(((s == 0) | (s == 2)).all()) and bool((s == 0).any()) and bool((s == 2).any())
