"""csrc/optim/fused_adamw.hip on the MI355X: the flat AdamW update against
torch.optim.AdamW (fp32, same device, the same gradients upcast), the
global-norm clipping kernels against a float64 norm and ``clip_grad_norm_``,
a ``MasterAdamW.step()`` captured into a hipGraph, and ``FlatAdamW`` under
DDP on a small ViT.

Tolerances.  Master / fp32 weights: atol = rtol = 1e-5 at lr = 1e-2, the bound
of the SGD kernel test (test_gpu_kernels.py): an update of magnitude O(lr)
through about ten fp32 operations of 1-3 ulp each is off by ~1e-2 * 10 * 2e-7
= 2e-8 per step, and the weight itself (|w| < 5) carries half an ulp, 2.4e-7,
per rounding: tenfold inside the bound.  tests/test_adamw.py checks on the CPU
that the same arithmetic in fp32 stays within 1e-6 of a float64 AdamW.  bf16
working copy: 1e-2 (8 mantissa bits), as in the SGD test.
"""
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops.optim import _SUMSQ_BLOCKS, MasterAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD, B1, B2, EPS = 1e-2, 0.1, 0.9, 0.999, 1e-8
BF16, F32 = torch.bfloat16, torch.float32


def _C():
    return _native.require("gpu tests")


def _big_n() -> int:
    """Three vectors more than one full grid of adamw_flat_step covers in one
    pass: lanes 0-2 of block 0 take a second grid-stride iteration."""
    return 8 * (_C().adamw_grid_cap() * 256 + 3)


def _segments(n):
    """[(start, length, decay?)]: lengths cycle 8, 24, 800; decay alternates."""
    out, o, i = [], 0, 0
    while o < n:
        ln = min((8, 24, 800)[i % 3], n - o)
        out.append((o, ln, i % 2 == 0))
        o += ln
        i += 1
    return out


def _hyper(step_t, clip=1.0):
    return torch.tensor([1 - B1 ** step_t, 1 - B2 ** step_t, 0.0, clip], device=DEV)


@pytest.mark.parametrize("gdtype,pdtype,master", [(BF16, BF16, True), (F32, F32, False), (F32, BF16, True),
                                                  (BF16, F32, False)])
@pytest.mark.parametrize("size", ["one_vector", "255_vectors", "second_grid_pass"])
def test_adamw_flat_step_matches_torch(gdtype, pdtype, master, size):
    n = {"one_vector": 8, "255_vectors": 8 * 255, "second_grid_pass": _big_n()}[size]
    torch.manual_seed(1)
    segs = _segments(n)
    decay = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask = torch.zeros(n // 8, dtype=torch.uint8, device=DEV)
    for o, ln, d in segs:
        decay[o:o + ln] = d
        mask[o // 8:(o + ln) // 8] = int(d)
    zero = torch.zeros(n, dtype=torch.bool, device=DEV)  # gradient exactly zero on every step
    for o, ln, _d in segs[2:4]:                           # an 800-element decayed and an 8-element undecayed one
        zero[o:o + ln] = True
    w0 = torch.randn(n, device=DEV)
    if pdtype == BF16:
        w0 = w0.bfloat16().float()  # master and working copy start equal
    ref_d = w0[decay].clone().requires_grad_()
    ref_n = w0[~decay].clone().requires_grad_()
    opt = torch.optim.AdamW([{"params": [ref_d], "weight_decay": WD}, {"params": [ref_n], "weight_decay": 0.0}],
                            lr=LR, betas=(B1, B2), eps=EPS)
    mst = w0.clone() if master else None
    param = w0.clone().to(pdtype)  # (w0.to(float32) would alias w0)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hyper = torch.zeros(4, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(4):
        g = torch.randn(n, device=DEV).to(gdtype)
        g[zero] = 0
        ref_d.grad, ref_n.grad = g.float()[decay], g.float()[~decay]
        opt.step()
        _C().adamw_prepare(None, hyper, step, 0.0, B1, B2)
        _C().adamw_flat_step(mst, m, v, g, param, mask, hyper, LR, B1, B2, EPS, WD)
    assert int(step) == 4
    torch.testing.assert_close(hyper, _hyper(4), atol=0, rtol=1e-6)
    want = torch.empty(n, device=DEV)
    want[decay], want[~decay] = ref_d.detach(), ref_n.detach()
    got = mst if master else param
    assert torch.isfinite(got).all() and torch.isfinite(m).all() and torch.isfinite(v).all()
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    if pdtype == BF16:
        torch.testing.assert_close(param.float(), want, atol=1e-2, rtol=1e-2)
        assert torch.equal(param, mst.bfloat16())
    # zero-gradient segments: moments stay 0, weights move by decay alone (an
    # m * rsqrt(v) shortcut gives 0 * inf = NaN here)
    if zero.any():
        assert torch.all(m[zero] == 0) and torch.all(v[zero] == 0)
        zd, zn = zero & decay, zero & ~decay
        torch.testing.assert_close(got[zd], w0[zd] * (1 - LR * WD) ** 4, atol=1e-6, rtol=1e-6)
        assert torch.equal(got[zn], w0[zn])


def test_adamw_flat_step_without_mask_decays_everywhere_and_int32_step():
    n = 8 * 255
    torch.manual_seed(2)
    w0 = torch.randn(n, device=DEV)
    ref = w0.clone().requires_grad_()
    opt = torch.optim.AdamW([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    w, m, v = w0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hyper = torch.zeros(4, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(4):
        g = torch.randn(n, device=DEV)
        ref.grad = g.clone()
        opt.step()
        _C().adamw_prepare(None, hyper, step, 0.0, B1, B2)
        _C().adamw_flat_step(None, m, v, g, w, None, hyper, LR, B1, B2, EPS, WD)
    assert int(step) == 4
    torch.testing.assert_close(w, ref.detach(), atol=1e-5, rtol=1e-5)
    with pytest.raises(RuntimeError, match="master"):
        _C().adamw_flat_step(None, m, v, g, w.bfloat16(), None, hyper, LR, B1, B2, EPS, WD)
    with pytest.raises(RuntimeError, match="decay_mask"):
        _C().adamw_flat_step(None, m, v, g, w, torch.ones(n // 8 - 1, dtype=torch.uint8, device=DEV), hyper,
                             LR, B1, B2, EPS, WD)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _C().adamw_flat_step(None, m[:12], v[:12], g[:12], w[:12], None, hyper, LR, B1, B2, EPS, WD)


# --------------------------------------------------------------------------- #
# clipping
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("gdtype", [BF16, F32])
@pytest.mark.parametrize("size", ["one_vector", "second_grid_pass"])
def test_grad_norm_matches_float64_and_is_reproducible(gdtype, size):
    """Observed on the MI355X: relative error of the norm 2.5e-8 to 4.1e-8
    over both sizes and dtypes (the fp32 rounding of the stored norm)."""
    n = 8 if size == "one_vector" else _big_n()
    torch.manual_seed(3)
    g1 = torch.randn(n, device=DEV).to(gdtype)
    g2 = (torch.randn(n, device=DEV) * 3).to(gdtype)
    want = torch.cat([g1.double(), g2.double()]).norm()
    part = torch.full((2, _SUMSQ_BLOCKS), float("nan"), device=DEV)  # the kernel writes every slot
    hyper = torch.zeros(4, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    max_norm = 0.5 * float(want)
    out = []
    for _ in range(2):
        _C().flat_sumsq_partials(g1, part[0])
        _C().flat_sumsq_partials(g2, part[1])
        _C().adamw_prepare(part, hyper, step, max_norm, B1, B2)
        out.append((part.clone(), hyper.clone()))
        part.fill_(float("nan"))
    blocks = min((n // 8 + 255) // 256, _SUMSQ_BLOCKS)
    p0 = out[0][0]
    assert torch.isfinite(p0).all() and torch.all(p0[:, blocks:] == 0) and torch.all(p0[:, :blocks] > 0)
    norm, coef = out[0][1][2].double(), out[0][1][3].double()
    print("grad norm rel err", float((norm - want).abs() / want))
    torch.testing.assert_close(norm, want, atol=0, rtol=1e-5)
    torch.testing.assert_close(coef, max_norm / (want + 1e-6), atol=0, rtol=1e-5)
    assert torch.equal(out[0][0], out[1][0])                     # bitwise on a second call
    assert torch.equal(out[0][1][2:], out[1][1][2:])
    assert int(step) == 2


def test_non_finite_norm_propagates_like_torch():
    """clip_grad_norm_'s coefficient is clamp(max_norm / (norm + 1e-6), max=1):
    0 for an infinite norm, NaN for a NaN one (the update then poisons every
    weight, which is how torch reports it too)."""
    g = torch.randn(64, device=DEV)
    hyper, step = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    part = torch.zeros(1, _SUMSQ_BLOCKS, device=DEV)
    for bad in (float("inf"), float("nan")):
        g[3] = bad
        _C().flat_sumsq_partials(g, part[0])
        _C().adamw_prepare(part, hyper, step, 1.0, B1, B2)
        want = (1.0 / (torch.linalg.vector_norm(g) + 1e-6)).clamp(max=1.0)
        torch.testing.assert_close(hyper[3], want, atol=0, rtol=0, equal_nan=True)
        torch.testing.assert_close(hyper[2], torch.linalg.vector_norm(g), atol=0, rtol=0, equal_nan=True)


def _two_dtype_params(n_bf16, n_f32, seed=4):
    torch.manual_seed(seed)
    a = torch.randn(n_bf16, device=DEV).bfloat16()
    b = torch.randn(40, n_f32 // 40, device=DEV)
    c = torch.randn(n_f32 // 40, device=DEV)  # 1-D: no decay
    return [torch.nn.Parameter(t.clone()) for t in (a.view(8, -1), b, c)]


def _stock(params):
    ref = [p.detach().float().clone().requires_grad_() for p in params]
    opt = torch.optim.AdamW([{"params": [r for r in ref if r.dim() > 1], "weight_decay": WD},
                             {"params": [r for r in ref if r.dim() <= 1], "weight_decay": 0.0}],
                            lr=LR, betas=(B1, B2), eps=EPS)
    return ref, opt


def _masters(opt, params):
    """fp32 value of every parameter as the optimizer holds it (master where there is one)."""
    out = {}
    for st in opt._groups:
        src = st.get("master", st["param"])
        for p, off in zip(st["params"], st["offs"]):
            out[id(p)] = src.as_strided(p.shape, p.stride(), off).float()
    return [out[id(p)] for p in params]


def test_clipped_update_matches_clip_grad_norm_then_adamw():
    params = _two_dtype_params(8 * 300, 40 * 50)
    ref, ropt = _stock(params)
    opt = MasterAdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.5)
    for _ in range(4):
        for p, r in zip(params, ref):
            p.grad.copy_(torch.randn_like(p))
            r.grad = p.grad.detach().float().clone()
        want_norm = torch.cat([r.grad.double().flatten() for r in ref]).norm()
        tn = torch.nn.utils.clip_grad_norm_(ref, 0.5)
        assert float(tn) > 0.5
        ropt.step()
        opt.step()
        torch.testing.assert_close(opt.last_grad_norm.double(), want_norm, atol=0, rtol=1e-5)
    for got, r in zip(_masters(opt, params), ref):
        torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5)
    for p, r in zip(params, ref):
        if p.dtype == BF16:
            torch.testing.assert_close(p.detach().float(), r.detach(), atol=1e-2, rtol=1e-2)


def test_norm_below_max_leaves_update_identical_to_unclipped():
    pa, pb = _two_dtype_params(8 * 300, 40 * 50), _two_dtype_params(8 * 300, 40 * 50)
    oa = MasterAdamW(pa, lr=LR, weight_decay=WD, max_grad_norm=1e6)
    ob = MasterAdamW(pb, lr=LR, weight_decay=WD, max_grad_norm=None)
    for _ in range(3):
        for a, b in zip(pa, pb):
            a.grad.copy_(torch.randn_like(a))
            b.grad.copy_(a.grad)
        oa.step()
        ob.step()
    assert float(oa._dev_state[pa[0].device]["hyper"][3]) == 1.0
    for a, b in zip(_masters(oa, pa), _masters(ob, pb)):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- #
# graph replay
# --------------------------------------------------------------------------- #
def test_step_captured_in_a_graph_advances_step_count_and_bias_correction():
    """Two eager steps, then step() captured once and replayed three times with
    fresh gradients in the flat gradient buffers: the step count, the bias
    corrections and the clip coefficient must advance on the device (a host
    value would be frozen at its capture-time value, t = 3)."""
    params = _two_dtype_params(8 * 300, 40 * 50, seed=6)
    ref, ropt = _stock(params)
    opt = MasterAdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.5)
    gen = torch.Generator(device=DEV).manual_seed(7)
    grads = [[torch.randn(p.shape, device=DEV, generator=gen).to(p.dtype) for p in params] for _ in range(5)]

    def feed(t):
        for p, r, g in zip(params, ref, grads[t]):
            p.grad.copy_(g)
            r.grad = g.float().clone()
        torch.nn.utils.clip_grad_norm_(ref, 0.5)
        ropt.step()

    def check(t):
        for got, r in zip(_masters(opt, params), ref):
            torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, msg=lambda m: f"step {t}: {m}")

    for t in range(2):
        feed(t)
        opt.step()
        check(t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    feed(2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    before = [m.clone() for m in _masters(opt, params)]
    for t in range(2, 5):
        if t > 2:
            feed(t)
        graph.replay()
        torch.cuda.synchronize()
        check(t)
    assert opt.state_dict()["steps"] == 5
    assert not any(torch.equal(a, b) for a, b in zip(before, _masters(opt, params)))


# --------------------------------------------------------------------------- #
# model level
# --------------------------------------------------------------------------- #
@pytest.fixture
def _pg():
    import torch.distributed as dist
    made = not dist.is_initialized()
    if made:  # one rank: an in-process store, no TCP port to race for
        dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1)
    yield
    if made:
        from distributed_model_parallel_amd.comm.rccl import reset_default_communicator
        reset_default_communicator()
        dist.destroy_process_group()


def test_flat_adamw_trains_a_small_vit_under_ddp(_pg):
    from distributed_model_parallel_amd.models import VisionTransformer
    from distributed_model_parallel_amd.ops import wt_cache
    from distributed_model_parallel_amd.ops.loss import cross_entropy
    from distributed_model_parallel_amd.ops.optim import FlatAdamW
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    from distributed_model_parallel_amd.utils.precision import cast_model
    torch.manual_seed(0)
    m = VisionTransformer(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256,
                          num_classes=10).to(DEV).to(memory_format=torch.channels_last)
    cast_model(m, BF16)
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.25, first_bucket_mb=0.05, flat_parameters=True)
    opt = FlatAdamW(ddp, lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD)
    plist = list(ddp._params)
    ref = [p.detach().float().clone().requires_grad_() for p in plist]
    ropt = torch.optim.AdamW([{"params": [r for r in ref if r.dim() > 1], "weight_decay": WD},
                              {"params": [r for r in ref if r.dim() <= 1], "weight_decay": 0.0}],
                             lr=1e-3, betas=(B1, B2), eps=EPS)
    assert any(p.dim() == 3 for p in plist), "cls_token / pos_embedding are 3-D and keep decay"
    x = torch.randn(16, 3, 32, 32, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,), device=DEV)
    w_probe = m.blocks[0].mlp.fc1.weight
    for t in range(3):
        cross_entropy(ddp(x), y).backward()
        wt_cache.transposed(w_probe)  # as a backward wanting W^T does: the optimizer's step keeps it from now on
        flats, layout = ddp.flat_groups(), ddp.param_layout()
        for p, r, (g, off) in zip(plist, ref, layout):
            r.grad = flats[g][1].as_strided(p.shape, p.stride(), off).float().contiguous()
        ropt.step()
        opt.step()
        for p, r, (g, off) in zip(plist, ref, ddp.param_layout()):
            st = opt._flat_state[g]
            got = st.get("master", st["param"]).as_strided(p.shape, p.stride(), off)
            torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, msg=lambda s: f"step {t}: {s}")
            assert torch.equal(p.detach(), got.to(p.dtype))
        # every cached W^T the optimizer owns was refreshed from the UPDATED weight
        seen = 0
        for k, e in wt_cache._GLOBAL.items():
            w = e[0]()
            if len(k) == 2 and w is not None and any(w is p for p in plist):
                assert e[2] == wt_cache._GEN[0]
                assert torch.equal(e[1], w.detach().reshape(w.shape[0], -1).t())
                seen += 1
        assert seen > 0
        opt.zero_grad()
    assert opt.state_dict()["steps"] == 3
    # the next forward / backward reads the refreshed cache: same as with the cache cleared
    outs = []
    try:
        for on in (True, False):
            wt_cache.set_enabled(on)
            opt.zero_grad()
            out = ddp(x)
            cross_entropy(out, y).backward()
            outs.append((out.detach().clone(), [g.clone() for _p, g in ddp.flat_groups()]))
    finally:
        wt_cache.set_enabled(True)
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        # same kernels on equal operands; two bf16 ulp for sums whose order is not fixed (a stale
        # W^T, one AdamW step of lr = 1e-3 behind on weights of ~0.1, is off by percents)
        torch.testing.assert_close(a.float(), b.float(), rtol=2 ** -6, atol=2 ** -6 * float(b.float().abs().max()))
