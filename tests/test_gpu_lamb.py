"""csrc/optim/fused_lamb.hip on the MI355X against tests/lamb_oracle.py (float64,
per tensor, from the definition; hyper-parameters and weight scales there).
Bounds: norms and trust ratios rtol 1e-5, atol 0 (tests/test_gpu_lars.py's: fp32
sums of at most 8192 terms folded in double); fp32 weights, m and v atol = rtol
= 1e-5 after 4 steps (the AdamW and LARS kernel tests'); bf16 parameters 1e-2
and exactly the rounded master.  The EMA is checked per step against
``e + (1 - d)(w - e)`` in float64 on the kernel's own previous e and new w at
atol = rtol = 1e-6: one subtraction and one fmaf, at most 1.5 ulp = 1.8e-7 relative.
"""
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops.optim import MasterLAMB
from tests.lamb_oracle import BETAS, EPS, HP, LR, SCALES, WD, Oracle
from tests.test_gpu_lars import _Flat, _masters, _pg, _trusts, _two_dtype_params  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ZERO_G_EXCLUDED, ZERO_W, ZERO_G = 7, 8, 10


def _C():
    return _native.require("gpu tests")


def _case(seed):
    """Every edge of the split (tensor 6 has more items than one stride of the folding
    wave), then four small tensors for the special cases; adapted and excluded alternate."""
    c, f = _C().lars_chunk_elems(), _C().lars_fold_threads()
    sizes = [8, 10, c, c + 8, 3 * c + 24, 24, (f + 1) * c + 24, 24, 8, 10, 24]
    adapted = [i % 2 == 0 for i in range(len(sizes))]
    torch.manual_seed(seed)
    ws = [torch.randn(n, device=DEV) * SCALES[i % 3] for i, n in enumerate(sizes)]
    ws[ZERO_W].zero_()
    return _Flat(sizes, adapted), sizes, adapted, ws


def _grads(sizes, dtype):
    gs = [torch.randn(n, device=DEV).to(dtype) for n in sizes]
    gs[ZERO_G_EXCLUDED].zero_()
    gs[ZERO_G].zero_()
    return gs


def _prepare(hyper, step, grad=None, max_norm=0.0):
    part = None
    if max_norm > 0:
        part = torch.zeros(1, 1024, device=DEV)
        _C().flat_sumsq_partials(grad, part[0])
    _C().adamw_prepare(part, hyper, step, max_norm, *BETAS)


def _close(got, want, tol, **kw):
    torch.testing.assert_close(got.double().cpu(), want.double().cpu(), atol=tol, rtol=tol, **kw)


@pytest.mark.parametrize("gdtype", [BF16, F32])
def test_norms_and_trust_ratios_match_float64_and_are_reproducible(gdtype):
    fl, sizes, adapted, ws = _case(3)
    weight, grad = fl.scatter(ws, F32), fl.scatter(_grads(sizes, gdtype), gdtype)
    want = Oracle(ws, adapted).step(fl.gather(grad))
    hyper, step = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    _prepare(hyper, step)
    out = []
    for _ in range(2):
        m, v = torch.zeros(fl.n, device=DEV), torch.zeros(fl.n, device=DEV)
        fl.partials.fill_(float("nan"))  # the kernels write every slot
        fl.coef.fill_(float("nan"))
        _C().lamb_moments(None, m, v, grad, weight, fl.items, fl.tensors, hyper, fl.partials, *BETAS, EPS, WD)
        _C().lamb_trust(fl.partials, fl.tensors, fl.coef, WD)
        out.append((fl.partials.clone(), fl.coef.clone()))
    part, coef = out[0]
    assert torch.isfinite(part).all() and torch.isfinite(coef).all()
    for col, name in ((0, "trust"), (2, "|w|"), (3, "|u|")):
        torch.testing.assert_close(coef[:, col].double().cpu(), want[:, (0, 0, 1, 2)[col]], atol=0, rtol=1e-5,
                                   msg=lambda s: f"{name}: {s}")
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])  # bitwise on a second call


@pytest.mark.parametrize("max_norm", [0.0, 1.0])  # |g| is about 800: 1.0 clips
@pytest.mark.parametrize("gdtype,pdtype,master", [(BF16, BF16, True), (F32, F32, False), (F32, BF16, True),
                                                  (BF16, F32, False)])
def test_lamb_step_matches_oracle(gdtype, pdtype, master, max_norm):
    fl, sizes, adapted, ws = _case(1)
    if pdtype == BF16:
        ws = [w.bfloat16().float() for w in ws]  # master and working copy start equal
    orc = Oracle(ws, adapted, max_norm)
    w0 = fl.scatter(ws, F32)
    mst, param = (w0.clone() if master else None), w0.clone().to(pdtype)
    m, v = torch.zeros(fl.n, device=DEV), torch.zeros(fl.n, device=DEV)
    decay = 0.9
    ema = w0.clone() if (pdtype == BF16 and gdtype == BF16 and not max_norm) else None
    hyper, step = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    ex = ~torch.tensor(adapted, device=DEV)
    for t in range(4):
        grad = fl.scatter(_grads(sizes, gdtype), gdtype)
        want = orc.step(fl.gather(grad))
        e0 = None if ema is None else ema.double()
        _prepare(hyper, step, grad, max_norm)
        _C().lamb_moments(mst, m, v, grad, param, fl.items, fl.tensors, hyper, fl.partials, *BETAS, EPS, WD)
        _C().lamb_trust(fl.partials, fl.tensors, fl.coef, WD)
        _C().lamb_flat_step(mst, m, v, param, fl.items, fl.coef, hyper, LR, EPS, ema, 0.0 if ema is None else decay)
        torch.testing.assert_close(fl.coef[:, 0].double().cpu(), want[:, 0], atol=0, rtol=1e-5)
        assert torch.all(fl.coef[ex, 0] == 1) and torch.all(fl.coef[ex, 1] == 0) and torch.all(fl.coef[~ex, 1] == WD)
        assert (float(fl.coef[ZERO_W, 0]) == 1.0) == (t == 0)  # |w| = 0 on the first step only
        assert float(fl.coef[ZERO_G_EXCLUDED, 3]) == 0.0       # zero gradients without decay: |u| = 0
        if ema is not None:
            _close(ema, e0 + (1 - decay) * ((mst if master else param).double() - e0), 1e-6)
    got = mst if master else param
    for name, flat, ref in (("w", got, orc.w), ("m", m, orc.m), ("v", v, orc.v)):
        for i, (a, b) in enumerate(zip(fl.gather(flat), ref)):
            _close(a, b, 1e-5, msg=lambda s: f"{name} of tensor {i}: {s}")
    if pdtype == BF16:
        _close(param.float(), fl.scatter(orc.w, torch.float64), 1e-2)
        assert torch.equal(param, mst.bfloat16())
    assert torch.equal(fl.gather(got)[ZERO_G_EXCLUDED], ws[ZERO_G_EXCLUDED])  # trust 1, u = 0: untouched
    for flat in (got, param, m, v) + (() if ema is None else (ema,)):
        assert torch.all(fl.padding(flat) == 0)  # slot padding stays zero in every buffer


def test_argument_checks_and_plan_entries_that_do_not_fit():
    """The flats are the front halves of buffers twice their size, so the bad
    entries below stay inside allocated memory whatever a kernel does with them."""
    fl = _Flat([800, 24], [True, False])
    n = fl.n
    wbuf, gbuf, mbuf, vbuf = torch.randn(2 * n, device=DEV), torch.randn(2 * n, device=DEV), *torch.zeros(2, 2 * n, device=DEV)
    w, m, v, g, coef = wbuf[:n], mbuf[:n], vbuf[:n], gbuf[:n], torch.ones(16, 4, device=DEV)[:2]
    hyper = torch.tensor([0.1, 0.01, 0.0, 1.0], device=DEV)
    mom = lambda **k: _C().lamb_moments(**{**dict(  # noqa: E731
        master=None, exp_avg=m, exp_avg_sq=v, grad=g, param=w, items=fl.items, tensors=fl.tensors, hyper=hyper,
        partials=fl.partials, beta1=0.9, beta2=0.99, eps=EPS, weight_decay=WD), **k})
    stp = lambda **k: _C().lamb_flat_step(**{**dict(  # noqa: E731
        master=None, exp_avg=m, exp_avg_sq=v, param=w, items=fl.items, coef=coef, hyper=hyper, lr=LR, eps=EPS), **k})
    for call, kw, match in ((mom, dict(param=w.bfloat16()), "master"), (stp, dict(param=w.bfloat16()), "master"),
                            (mom, dict(hyper=hyper[:3]), "hyper"), (stp, dict(exp_avg_sq=v[:8]), "exp_avg_sq"),
                            (mom, dict(partials=fl.partials[:-1].contiguous()), "one row per work item"),
                            (mom, dict(items=fl.items.long()), "items"), (mom, dict(eps=0.0), "eps"),
                            (stp, dict(coef=coef[:, :2].contiguous()), "coef"),
                            (mom, dict(grad=g[:12], param=w[:12]), "multiple of 8")):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    w0, bad = wbuf.clone(), fl.items.clone()
    bad[0, 0] = n // 8 - 1   # 100 vectors from the flat's last one
    bad[1, 2] = 7            # no such tensor
    fl.partials.fill_(float("nan"))
    mom(items=bad)
    stp(items=bad)
    torch.cuda.synchronize()
    assert torch.equal(wbuf, w0) and torch.all(mbuf == 0) and torch.all(vbuf == 0) and torch.all(fl.partials == 0)


def test_master_lamb_eager_then_captured_follows_fresh_gradients():
    """Two eager steps, then step() captured once and replayed three times."""
    params = _two_dtype_params(8 * 300, 40 * 50, seed=6)
    with torch.no_grad():
        for i, p in enumerate(params):
            p.mul_(SCALES[i % 3])
    opt = MasterLAMB(params, **HP)  # max_grad_norm = 1.0, the default, clips
    orc = Oracle(params, [p.dim() > 1 for p in params], max_norm=1.0)
    gen = torch.Generator(device=DEV).manual_seed(7)
    grads = [[torch.randn(p.shape, device=DEV, generator=gen).to(p.dtype) for p in params] for _ in range(5)]

    def feed(t):
        for p, g in zip(params, grads[t]):
            p.grad.copy_(g)
        return orc.step(grads[t])

    def check(t, want):
        for got, r in zip(_masters(opt, params), orc.w):
            _close(got, r, 1e-5, msg=lambda s: f"step {t}: {s}")
        torch.testing.assert_close(_trusts(opt, params), want[:, 0], atol=0, rtol=1e-5)

    for t in range(2):
        want = feed(t)
        opt.step()
        check(t, want)
    plans = [id(p[k]) for p in opt._plans for k in ("items", "tensors", "partials", "coef")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    want = feed(2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    assert plans == [id(p[k]) for p in opt._plans for k in ("items", "tensors", "partials", "coef")]
    seen = []
    for t in range(2, 5):
        if t > 2:
            want = feed(t)
        graph.replay()
        torch.cuda.synchronize()
        check(t, want)
        seen.append(_trusts(opt, params))
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert opt.state_dict()["steps"] == 5 and float(opt.last_grad_norm) > 1.0


def test_flat_lamb_trains_a_small_resnet_under_ddp(_pg):  # noqa: F811
    from distributed_model_parallel_amd.models import build_model
    from distributed_model_parallel_amd.ops.loss import cross_entropy
    from distributed_model_parallel_amd.ops.optim import FlatLAMB
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    from distributed_model_parallel_amd.utils.precision import cast_model
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10).to(DEV).to(memory_format=torch.channels_last)
    cast_model(model, BF16)
    ddp = DistributedDataParallel(model, bucket_cap_mb=4.0, first_bucket_mb=1.0, flat_parameters=True)
    opt = FlatLAMB(ddp, **HP)
    plist = list(ddp._params)
    orc = Oracle(plist, [p.dim() > 1 for p in plist], max_norm=1.0)
    x = torch.randn(8, 3, 32, 32, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), device=DEV)
    for t in range(3):
        cross_entropy(ddp(x), y).backward()
        flats, layout = ddp.flat_groups(), ddp.param_layout()
        want = orc.step([flats[g][1].as_strided(p.shape, p.stride(), off) for p, (g, off) in zip(plist, layout)])
        opt.step()
        torch.testing.assert_close(_trusts(opt, plist), want[:, 0], atol=0, rtol=1e-5)
        for p, r, (g, off) in zip(plist, orc.w, ddp.param_layout()):
            st = opt._flat_state[g]
            got = st.get("master", st["param"]).as_strided(p.shape, p.stride(), off)
            _close(got, r, 1e-5, msg=lambda s: f"step {t}: {s}")
            assert torch.equal(p.detach(), got.to(p.dtype))
        opt.zero_grad()
    assert opt.state_dict()["steps"] == 3 and opt.state_dict()["kind"] == "lamb"
