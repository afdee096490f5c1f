"""The weight EMA inside the flat step kernels (csrc/optim/fused_sgd.hip,
fused_adamw.hip, fused_lars.hip, ``ema`` / ``ema_decay``) on the MI355X: the
kernels' EMA against the float64 recurrence over their own master output and
as a pure side output (everything else bit-identical to the call without it),
the optimizers on a bf16 plus an fp32 group on both routes, a step captured
into a hipGraph, and ``FlatAdamW`` with ``ema_weights()`` under DDP on a small
ViT.

Tolerance of the recurrence: atol = rtol = 5e-6.  One ``fmaf`` and one
subtraction per step, at most 1.5 ulp of ``|e| < 5``, i.e. 7.2e-7 per step and
2.9e-6 over 4 steps before the decay contracts it.  On the CPU the same fp32
recurrence stayed within 5.2e-7 of float64 over 8 steps at d = 0.5 / 0.9 /
0.9999."""
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import optim
from distributed_model_parallel_amd.ops.optim import MasterAdamW, MasterLARS, MasterSGD

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 5e-6
LR, WD, B1, B2, EPS, MU = 1e-2, 0.1, 0.9, 0.999, 1e-8, 0.9
BF16, F32 = torch.bfloat16, torch.float32
COMBOS = [(BF16, BF16, True), (F32, F32, False), (F32, BF16, True), (BF16, F32, False)]  # grad, param, master?
STEPS = 4


def _C():
    return _native.require("gpu tests")


def _sizes():
    # one vector; 255 vectors; three vectors more than one full grid covers in one pass
    return {"one_vector": 8, "255_vectors": 8 * 255, "second_grid_pass": 8 * (_C().adamw_grid_cap() * 256 + 3)}


def _close(got, want, msg):
    torch.testing.assert_close(got.double(), want, atol=TOL, rtol=TOL, msg=lambda s: f"{msg}: {s}")


class _Flat:
    """One flat group at the kernel level, with slot tails: every 5th vector's
    last 3 elements are padding (weight and gradient exactly 0, as the layouts
    leave them)."""

    def __init__(self, n, pdtype, master, seed=1):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.pad = torch.zeros(n, dtype=torch.bool, device=DEV)
        idx = torch.arange(n, device=DEV)
        self.pad[(idx // 8 % 5 == 4) & (idx % 8 >= 5)] = True
        w0 = torch.randn(n, device=DEV, generator=g)
        if pdtype == BF16:
            w0 = w0.bfloat16().float()  # master and working copy start equal
        w0[self.pad] = 0
        self.master = w0.clone() if master else None
        self.param = w0.clone().to(pdtype)
        self.state = [torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
        self.n = n

    def weights(self):
        return self.master if self.master is not None else self.param

    def tensors(self):
        return [t for t in (self.master, self.param, *self.state) if t is not None]


def _grads(n, gdtype, pad, seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(STEPS):
        t = torch.randn(n, device=DEV, generator=g).to(gdtype)
        t[pad] = 0
        out.append(t)
    return out


def _sgd_step(f, grad, t, ema, decay):
    _C().sgd_flat_step(f.master, f.state[0], grad, f.param, 0.1, 1e-4, MU, 0.0, False, 1.0, t == 0, ema, decay)


class _AdamW:
    def __init__(self):
        self.hyper = torch.zeros(4, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)

    def __call__(self, f, grad, t, ema, decay):
        mask = (torch.arange(f.n // 8, device=DEV) % 3 != 0).to(torch.uint8)
        _C().adamw_prepare(None, self.hyper, self.step, 0.0, B1, B2)
        _C().adamw_flat_step(f.master, f.state[0], f.state[1], grad, f.param, mask, self.hyper, LR, B1, B2, EPS, WD,
                             ema, decay)


def _check_side_output(twins, step_fns, grads, decay):
    """`twins` = (with EMA, without): after every step (b) the EMA follows the
    float64 recurrence over the kernel's own master output and (c) stays 0 on the
    padding; at the end (a) every other buffer is bit-identical to the twin's."""
    a, b = twins
    ema = a.weights().clone()
    assert ema.dtype == F32
    e64 = ema.double()
    for t, g in enumerate(grads):
        step_fns[0](a, g, t, ema, decay)
        step_fns[1](b, g, t, None, 0.0)
        e64 += (1.0 - decay) * (a.weights().double() - e64)
        _close(ema, e64, f"step {t}")
        assert torch.all(ema[a.pad] == 0)
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)
    assert not torch.equal(ema, a.weights().float())  # it lags the weights
    return ema


@pytest.mark.parametrize("gdtype,pdtype,master", COMBOS)
@pytest.mark.parametrize("size", ["one_vector", "255_vectors", "second_grid_pass"])
@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_flat_step_ema_is_the_recurrence_and_a_pure_side_output(rule, size, gdtype, pdtype, master):
    n = _sizes()[size]
    twins = (_Flat(n, pdtype, master), _Flat(n, pdtype, master))
    fns = (_sgd_step, _sgd_step) if rule == "sgd" else (_AdamW(), _AdamW())
    _check_side_output(twins, fns, _grads(n, gdtype, twins[0].pad), 0.9)


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_flat_step_ema_at_decay_0_9999(rule):
    n = _sizes()["255_vectors"]
    twins = (_Flat(n, BF16, True), _Flat(n, BF16, True))
    fns = (_sgd_step, _sgd_step) if rule == "sgd" else (_AdamW(), _AdamW())
    start = twins[0].weights().clone()
    ema = _check_side_output(twins, fns, _grads(n, BF16, twins[0].pad), 0.9999)
    assert float((ema - start).abs().max()) > 0  # it moved, by ~1e-4 of the weights' movement


# --------------------------------------------------------------------------- #
LARS_SIZES = (8, 24, 800, 8200, 13)  # 8200 spans two work items; 13 leaves a 3-element slot tail


class _LarsFlat:
    """The flats and the plan of a MasterLARS over tensors of LARS_SIZES; the
    gradient flat is our own so that its dtype can differ from the parameters'."""

    def __init__(self, gdtype, pdtype):
        g = torch.Generator(device=DEV).manual_seed(3)
        params = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=g).to(pdtype)) for s in LARS_SIZES]
        self.opt = MasterLARS(params, lr=LR, momentum=MU, weight_decay=1e-4, exclude_1d=False)
        st = self.opt._groups[0]
        self.plan = self.opt._lars_plans(self.opt._current_groups())[0]
        assert 8200 > _C().lars_chunk_elems() and self.plan["items"].shape[0] == len(LARS_SIZES) + 1
        self.master, self.param, self.mom = st.get("master"), st["param"], st["momentum"]
        self.n = self.param.numel()
        self.pad = torch.ones(self.n, dtype=torch.bool, device=DEV)
        for p, off in zip(st["params"], st["offs"]):
            self.pad[off:off + p.numel()] = False
        assert int(self.pad.sum()) == 3
        self.gdtype = gdtype

    def weights(self):
        return self.master if self.master is not None else self.param

    def tensors(self):
        return [t for t in (self.master, self.param, self.mom, self.plan["coef"]) if t is not None]


def _lars_step(f, grad, t, ema, decay):
    C, p = _C(), f.plan
    C.lars_norm_partials(f.master, grad, f.param, p["items"], p["partials"])
    C.lars_trust(p["partials"], p["tensors"], p["coef"], 1e-3, 1e-4, 1e-8)
    C.lars_flat_step(f.master, f.mom, grad, f.param, p["items"], p["coef"], 50.0, MU, ema, decay)  # trust ~1e-3


@pytest.mark.parametrize("gdtype,pdtype,master,decay", [c + (0.9,) for c in COMBOS] + [(BF16, BF16, True, 0.9999)])
def test_lars_flat_step_ema_is_the_recurrence_and_a_pure_side_output(gdtype, pdtype, master, decay):
    twins = (_LarsFlat(gdtype, pdtype), _LarsFlat(gdtype, pdtype))
    assert (twins[0].master is not None) == master
    _check_side_output(twins, (_lars_step, _lars_step), _grads(twins[0].n, gdtype, twins[0].pad), decay)


# --------------------------------------------------------------------------- #
def _calls(n=64):
    """The three entry points as f(ema, decay) on valid buffers of n elements, and their master."""
    f = _Flat(n, BF16, True)
    g = torch.randn(n, device=DEV).bfloat16()
    adamw = _AdamW()
    lf = _LarsFlat(BF16, BF16)
    lg = torch.zeros(lf.n, device=DEV).bfloat16()
    return [("sgd", f.n, f.master, lambda e, d: _sgd_step(f, g, 1, e, d)),
            ("adamw", f.n, f.master, lambda e, d: adamw(f, g, 0, e, d)),
            ("lars", lf.n, lf.master, lambda e, d: _lars_step(lf, lg, 0, e, d))]


def test_ema_argument_checks():
    for name, n, master, call in _calls():
        before = master.clone()
        with pytest.raises(RuntimeError, match="ema"):
            call(torch.zeros(n, device=DEV).bfloat16(), 0.9)  # not fp32
        with pytest.raises(RuntimeError, match="ema"):
            call(torch.zeros(n - 8, device=DEV), 0.9)  # wrong numel
        with pytest.raises(RuntimeError, match="ema"):
            call(master, 0.9)  # aliases the master
        with pytest.raises(RuntimeError, match="ema"):
            call(master[:], 0.9)
        with pytest.raises(RuntimeError, match="ema"):
            call(torch.zeros(2 * n, device=DEV)[::2], 0.9)  # not contiguous
        with pytest.raises(RuntimeError, match="ema"):
            call(torch.zeros(n), 0.9)  # not on the device
        for bad in (1.0, -0.1):
            with pytest.raises(RuntimeError, match="ema_decay"):
                call(torch.zeros(n, device=DEV), bad)
        assert torch.equal(master, before), name  # nothing was launched
        call(torch.zeros(n, device=DEV), 0.0)  # the ends of the range are valid
        call(None, 1.0)  # no EMA: the decay is not looked at


# --------------------------------------------------------------------------- #
# optimizer level
# --------------------------------------------------------------------------- #
def _two_dtype_params(seed=4):
    torch.manual_seed(seed)
    a = torch.randn(8 * 300, device=DEV).bfloat16()
    b = torch.randn(40, 50, device=DEV)
    c = torch.randn(53, device=DEV)  # 1-D, with a slot tail
    return [torch.nn.Parameter(t.clone()) for t in (a.view(8, -1), b, c)]


def _masters(opt):
    views = {}
    for gi, st in enumerate(opt._current_groups()):
        src = st.get("master", st["param"])
        for p, off in opt._slots(gi):
            views[id(p)] = src.as_strided(p.shape, p.stride(), off)
    return [views[id(p)] for grp in opt.param_groups for p in grp["params"]]


OPTS = {"sgd": (MasterSGD, dict(lr=0.1, momentum=MU, weight_decay=1e-4)),
        "adamw": (MasterAdamW, dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.5)),
        "lars": (MasterLARS, dict(lr=0.5, momentum=MU, weight_decay=1e-4))}


@pytest.mark.parametrize("kind", sorted(OPTS))
def test_optimizer_ema_fused_and_unfused(kind):
    cls, kw = OPTS[kind]
    pa, pb = _two_dtype_params(), _two_dtype_params()
    oa, ob = cls(pa, ema_decay=0.9, **kw), cls(pb, ema_decay=0.9, **kw)
    e64 = [m.double().clone() for m in _masters(oa)]
    gen = torch.Generator(device=DEV).manual_seed(5)
    assert optim.fused_ema()
    try:
        for t in range(STEPS):
            for p, q in zip(pa, pb):
                p.grad.copy_(torch.randn(p.shape, device=DEV, generator=gen).to(p.dtype))
                q.grad.copy_(p.grad)
            oa.step()
            optim.set_fused_ema(False)
            ob.step()
            optim.set_fused_ema(True)
            for e, m, got, unf in zip(e64, _masters(oa), oa.ema_tensors(), ob.ema_tensors()):
                e += 0.1 * (m.double() - e)  # 1 - 0.9 in double, as the host forms it
                _close(got, e, f"fused, step {t}")
                _close(unf, e, f"unfused, step {t}")
    finally:
        optim.set_fused_ema(True)
    for a, b in zip(_masters(oa), _masters(ob)):
        assert torch.equal(a, b)
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
    for st in oa._groups:  # slot tails
        used = torch.zeros(st["ema"].numel(), dtype=torch.bool, device=DEV)
        for p, off in zip(st["params"], st["offs"]):
            used[off:off + p.numel()] = True
        assert torch.all(st["ema"][~used] == 0)
    assert oa.state_dict()["ema_updates"] == STEPS


# --------------------------------------------------------------------------- #
# graph replay
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_step_with_constant_ema_decay_captured_in_a_graph(kind):
    """Two eager steps, then step() captured once and replayed three times with
    fresh gradients in the flat gradient buffers: the decay is a host scalar,
    constant, so every replay makes the same update of the EMA from the master
    it has just written."""
    cls, kw = OPTS[kind]
    params = _two_dtype_params(seed=6)
    opt = cls(params, ema_decay=0.9, **kw)
    e64 = [m.double().clone() for m in _masters(opt)]
    gen = torch.Generator(device=DEV).manual_seed(7)
    grads = [[torch.randn(p.shape, device=DEV, generator=gen).to(p.dtype) for p in params] for _ in range(5)]

    def feed(t):
        for p, g in zip(params, grads[t]):
            p.grad.copy_(g)

    def check(t):
        for e, m, got in zip(e64, _masters(opt), opt.ema_tensors()):
            e += 0.1 * (m.double() - e)
            _close(got, e, f"step {t}")

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
    before = [e.clone() for e in opt.ema_tensors()]
    for t in range(2, 5):
        if t > 2:
            feed(t)
        graph.replay()
        torch.cuda.synchronize()
        check(t)
    assert not any(torch.equal(a, b) for a, b in zip(before, opt.ema_tensors()))


def test_ema_warmup_refuses_capture_before_anything_is_launched():
    params = _two_dtype_params(seed=8)
    opt = MasterAdamW(params, lr=LR, ema_decay=0.9, ema_warmup=True)
    for p in params:
        p.grad.copy_(torch.randn_like(p))
    opt.step()  # eager steps are fine
    torch.cuda.synchronize()
    masters = [m.clone() for m in _masters(opt)]
    ema = [e.clone() for e in opt.ema_tensors()]
    marker = torch.zeros(8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(ValueError, match="ema_warmup cannot be captured"):
                opt.step()
            marker.add_(1.0)  # the capture itself goes on and ends cleanly
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.all(marker == 1.0)
    for m, m0 in zip(_masters(opt), masters):
        assert torch.equal(m, m0)  # the replayed graph holds nothing of the step
    for e, e0 in zip(opt.ema_tensors(), ema):
        assert torch.equal(e, e0)
    assert opt.state_dict()["ema_updates"] == 1 and opt.state_dict()["steps"] == 1


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


def test_flat_adamw_ema_and_ema_weights_on_a_small_vit_under_ddp(_pg):
    from distributed_model_parallel_amd.models import VisionTransformer
    from distributed_model_parallel_amd.ops import wt_cache
    from distributed_model_parallel_amd.ops.loss import cross_entropy
    from distributed_model_parallel_amd.ops.optim import FlatAdamW
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    from distributed_model_parallel_amd.utils.precision import cast_model

    def make():
        torch.manual_seed(0)
        m = VisionTransformer(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256,
                              num_classes=10).to(DEV).to(memory_format=torch.channels_last)
        cast_model(m, BF16)
        ddp = DistributedDataParallel(m, bucket_cap_mb=0.25, first_bucket_mb=0.05, flat_parameters=True)
        return m, ddp, FlatAdamW(ddp, lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, ema_decay=0.9)

    def slot(opt, ddp, key):
        out = []
        for p, (g, off) in zip(ddp._params, ddp.param_layout()):
            st = opt._flat_state[g]
            out.append(st.get(key, st["param"]).as_strided(p.shape, p.stride(), off))
        return out

    torch.manual_seed(1)
    x = torch.randn(16, 3, 32, 32, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,), device=DEV)
    ma, da, oa = make()
    oa._ensure_state()
    e64 = [m.double().clone() for m in slot(oa, da, "master")]
    for t in range(3):
        cross_entropy(da(x), y).backward()
        wt_cache.transposed(ma.blocks[0].mlp.fc1.weight)  # as a backward wanting W^T does
        oa.step()
        oa.zero_grad()
        for e, m, got in zip(e64, slot(oa, da, "master"), slot(oa, da, "ema")):
            assert got.dtype == F32
            e += 0.1 * (m.double() - e)
            _close(got, e, f"step {t}")
    plist = list(da._params)
    ema = [e.clone() for e in slot(oa, da, "ema")]
    ma.eval()
    with torch.no_grad():
        live_out = ma(x).clone()
    with oa.ema_weights():
        for p, e in zip(plist, ema):
            assert torch.equal(p.detach(), e.to(p.dtype))
        with torch.no_grad():
            ema_out = ma(x).clone()
    ma.train()
    assert torch.isfinite(ema_out.float()).all()
    assert not torch.equal(ema_out, live_out)
    for p, m in zip(plist, slot(oa, da, "master")):
        assert torch.equal(p.detach(), m.to(p.dtype))
    for e, e0 in zip(slot(oa, da, "ema"), ema):
        assert torch.equal(e, e0)
    # the next forward / backward reads the weights and the caches of the live side again: the same
    # as a twin with the same live weights that never swapped (and has no cache entry yet)
    mb, db, _ob = make()
    mb.load_state_dict(ma.state_dict())
    outs = []
    for ddp in (da, db):
        out = ddp(x)
        cross_entropy(out, y).backward()
        outs.append((out.detach().clone(), torch.cat([p.grad.detach().float().flatten() for p in ddp._params])))
    assert torch.equal(outs[0][0], outs[1][0])
    a, b = outs[0][1], outs[1][1]
    # same kernels on equal operands; two bf16 ulp for sums whose order is not fixed (a stale
    # W^T, the EMA's instead of the live weights', is off by percents)
    torch.testing.assert_close(a, b, rtol=2 ** -6, atol=2 ** -6 * float(b.abs().max()))
