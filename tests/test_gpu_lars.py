"""csrc/optim/fused_lars.hip on the MI355X: the segmented norms and trust
ratios against float64, the flat LARS update against an oracle written here
(per tensor the trust ratio in float64 from the definition, ``d = trust (g +
wd w)`` handed as the gradient to a stock ``torch.optim.SGD(lr, momentum,
weight_decay=0)`` on an fp32 copy), ``MasterLARS.step()`` captured into a
hipGraph, and ``FlatLARS`` under DDP on a small channels-last ResNet.

Hyper-parameters lr = 1e-2, mu = 0.9, wd = 0.1, eta = 1, eps = 1e-8; weights
randn, gradients randn x s with s cycling 0.1, 1, 10 from tensor to tensor.
These are not training values: with eta = 1e-3 every update would be ~1e-5 and
a wrong trust ratio would hide inside the tolerance.  Here the float64 trust
ratios range from ~0.1 to ~6 and neighbours differ about tenfold, per-step
updates are 1e-2 to 5e-2, so a ratio taken from the neighbouring tensor is
wrong by ~1e-2, a thousand times the bound.

Tolerances.  Norms and trust ratios: rtol = 1e-5, atol = 0 against float64 (a
CPU emulation of the kernel's arithmetic -- 32 sequential fp32 accumulations
per lane, an fp32 tree per 8192-element chunk, a double fold, fp32 storage --
is off by 3e-9 to 7.4e-8).  fp32 master / fp32 weights: atol = rtol = 1e-5
after 4 steps, the bound of the SGD and AdamW kernel tests (the trust error
times the update size is below 1e-8 per step; the weight itself, |w| < 5,
carries half an ulp, 2.4e-7, per rounding).  bf16 working copy: 1e-2 (8
mantissa bits) and ``param == master.bfloat16()`` exactly.

The tests print the observed maxima (run with ``-s``).  Observed on the
MI355X: norms off by 4.1e-8 to 6.5e-8 relative, trust ratios by up to 6.0e-8
(the fp32 rounding of the stored values), over the flat of the kernel tests
and the 62 tensors of the ResNet-18; fp32 master / fp32 weights after 4 steps
within 4.8e-7 absolute of the oracle in all four dtype combinations.
"""
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops.optim import MasterLARS

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, MU, WD, ETA, EPS = 1e-2, 0.9, 0.1, 1.0, 1e-8
HP = dict(lr=LR, momentum=MU, weight_decay=WD, trust_coefficient=ETA, eps=EPS)
BF16, F32 = torch.bfloat16, torch.float32
SCALES = (0.1, 1.0, 10.0)


def _C():
    return _native.require("gpu tests")


def _sizes():
    """8, 10 (slot 16), C, C + 8, 3C + 24, 800, 24, and one tensor with more
    chunks than four strides of the lanes that fold one tensor's partials, plus
    three vectors (305 chunks, 2.5 M elements)."""
    c, fold = _C().lars_chunk_elems(), _C().lars_fold_threads()
    return [8, 10, c, c + 8, 3 * c + 24, 800, 24, (4 * fold + 49) * c + 24]


class _Flat:
    """Tensors laid out back to back in 8-element-padded slots, with the plan
    of work items built here (not by ops/optim.py)."""

    def __init__(self, sizes, adapted):
        chunk = _C().lars_chunk_elems() // 8
        self.sizes, self.adapted, self.offs = list(sizes), list(adapted), []
        items, tensors, o = [], [], 0
        for t, (n, a) in enumerate(zip(sizes, adapted)):
            self.offs.append(o)
            nvec, first = (n + 7) // 8, len(items)
            for v in range(0, nvec, chunk):
                items.append((o // 8 + v, min(chunk, nvec - v), t))
            tensors.append((first, len(items) - first, int(a)))
            o += nvec * 8
        self.n = o
        self.items = torch.tensor(items, dtype=torch.int32, device=DEV)
        self.tensors = torch.tensor(tensors, dtype=torch.int32, device=DEV)
        self.partials = torch.full((len(items), 2), float("nan"), device=DEV)
        self.coef = torch.full((len(sizes), 4), float("nan"), device=DEV)

    def scatter(self, tensors, dtype):
        flat = torch.zeros(self.n, dtype=dtype, device=DEV)  # the padding is zero
        for o, t in zip(self.offs, tensors):
            flat[o:o + t.numel()] = t.to(dtype)
        return flat

    def gather(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offs, self.sizes)]

    def padding(self, flat):
        return torch.cat([flat[o + n:o + (n + 7) // 8 * 8] for o, n in zip(self.offs, self.sizes)])


def _trust64(w, g, adapted=True):
    """The definition, in float64 (python floats)."""
    if not adapted:
        return 1.0
    wn, gn = float(w.double().norm()), float(g.double().norm())
    return 1.0 if wn == 0.0 or gn == 0.0 else ETA * wn / (gn + WD * wn + EPS)


def _oracle(ws):
    ref = [w.detach().float().clone().requires_grad_() for w in ws]
    return ref, torch.optim.SGD(ref, lr=LR, momentum=MU, weight_decay=0.0)


def _oracle_step(ref, ropt, grads, adapted):
    trusts = []
    for r, g, a in zip(ref, grads, adapted):
        w, g = r.detach().double(), g.detach().double().reshape(r.shape)
        trust = _trust64(w, g, a)
        r.grad = (trust * (g + WD * w)).float() if a else g.float()
        trusts.append(trust)
    ropt.step()
    return trusts


def _rel(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


# --------------------------------------------------------------------------- #
# segmented norms and trust ratios
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("gdtype", [BF16, F32])
def test_segmented_norms_match_float64_and_are_reproducible(gdtype):
    """Observed on the MI355X: |w| 4.8e-8, |g| 4.1e-8 (fp32) / 6.5e-8 (bf16), trust
    ratio 5.2e-8 / 5.8e-8 relative; float64 trust ratios from 0.099 to 5.28."""
    sizes = _sizes()
    torch.manual_seed(3)
    fl = _Flat(sizes, [True] * len(sizes))
    ws = [torch.randn(n, device=DEV) for n in sizes]
    gs = [(torch.randn(n, device=DEV) * SCALES[i % 3]).to(gdtype) for i, n in enumerate(sizes)]
    weight, grad = fl.scatter(ws, F32), fl.scatter(gs, gdtype)
    out = []
    for _ in range(2):
        _C().lars_norm_partials(None, grad, weight, fl.items, fl.partials)
        _C().lars_trust(fl.partials, fl.tensors, fl.coef, ETA, WD, EPS)
        out.append((fl.partials.clone(), fl.coef.clone()))
        fl.partials.fill_(float("nan"))  # the kernels write every slot
        fl.coef.fill_(float("nan"))
    part, coef = out[0]
    assert torch.isfinite(part).all() and torch.isfinite(coef).all() and torch.all(part > 0)
    want_w = torch.stack([w.double().norm() for w in ws])
    want_g = torch.stack([g.double().norm() for g in gs])
    want_t = torch.tensor([_trust64(w, g) for w, g in zip(ws, gs)], dtype=torch.float64, device=DEV)
    print("rel err |w| %.2e |g| %.2e trust %.2e; trust range %.3f-%.3f" % (
        _rel(coef[:, 2], want_w), _rel(coef[:, 3], want_g), _rel(coef[:, 0], want_t),
        float(want_t.min()), float(want_t.max())))
    torch.testing.assert_close(coef[:, 2].double(), want_w, atol=0, rtol=1e-5)
    torch.testing.assert_close(coef[:, 3].double(), want_g, atol=0, rtol=1e-5)
    torch.testing.assert_close(coef[:, 0].double(), want_t, atol=0, rtol=1e-5)
    assert torch.all(coef[:, 1] == WD)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])  # bitwise on a second call
    # an fp32 master beside bf16 parameters gives the same norms as the fp32 weights themselves
    _C().lars_norm_partials(weight, grad, weight.bfloat16(), fl.items, fl.partials)
    assert torch.equal(fl.partials, part)


# --------------------------------------------------------------------------- #
# the update
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("gdtype,pdtype,master", [(BF16, BF16, True), (F32, F32, False), (F32, BF16, True),
                                                  (BF16, F32, False)])
def test_lars_flat_step_matches_oracle(gdtype, pdtype, master):
    # adapted and excluded alternate; index 7: excluded, zero gradient; 10: zero weights; 12: zero gradient
    sizes = _sizes()[:7] + [40] + _sizes()[7:] + [800, 808, 24, 800]
    adapted = [i % 2 == 0 for i in range(len(sizes))]
    zero_g, zero_w = (7, 12), (10,)
    assert not adapted[7] and adapted[10] and adapted[12]
    torch.manual_seed(1)
    fl = _Flat(sizes, adapted)
    ws = [torch.randn(n, device=DEV) for n in sizes]
    for i in zero_w:
        ws[i].zero_()
    if pdtype == BF16:
        ws = [w.bfloat16().float() for w in ws]  # master and working copy start equal
    ref, ropt = _oracle(ws)
    w0 = fl.scatter(ws, F32)
    mst = w0.clone() if master else None
    param = w0.clone().to(pdtype)
    mom = torch.zeros(fl.n, device=DEV)
    terr = 0.0
    for step in range(4):
        gs = [(torch.randn(n, device=DEV) * SCALES[i % 3]).to(gdtype) for i, n in enumerate(sizes)]
        for i in zero_g:
            gs[i].zero_()
        grad = fl.scatter(gs, gdtype)
        want_t = _oracle_step(ref, ropt, [g.float() for g in gs], adapted)
        _C().lars_norm_partials(mst, grad, param, fl.items, fl.partials)
        _C().lars_trust(fl.partials, fl.tensors, fl.coef, ETA, WD, EPS)
        _C().lars_flat_step(mst, mom, grad, param, fl.items, fl.coef, LR, MU)
        want_t = torch.tensor(want_t, dtype=torch.float64, device=DEV)
        terr = max(terr, _rel(fl.coef[:, 0], want_t))
        torch.testing.assert_close(fl.coef[:, 0].double(), want_t, atol=0, rtol=1e-5)
        ex = torch.tensor(adapted, device=DEV)
        assert torch.all(fl.coef[~ex, 0] == 1) and torch.all(fl.coef[~ex, 1] == 0) and torch.all(fl.coef[ex, 1] == WD)
        assert (float(want_t[10]) == 1.0) == (step == 0)  # |w| = 0 on the first step only
        assert float(want_t[12]) == 1.0                   # |g| = 0 on every step
    got_flat = mst if master else param
    assert torch.isfinite(got_flat).all() and torch.isfinite(mom).all()
    werr = 0.0
    for i, (got, r) in enumerate(zip(fl.gather(got_flat), ref)):
        werr = max(werr, float((got - r.detach()).abs().max()))
        torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, msg=lambda s: f"tensor {i}: {s}")
    print("max trust rel err %.2e, max weight abs err %.2e" % (terr, werr))
    if pdtype == BF16:
        want = fl.scatter([r.detach() for r in ref], F32)
        torch.testing.assert_close(param.float(), want, atol=1e-2, rtol=1e-2)
        assert torch.equal(param, mst.bfloat16())
    # an excluded tensor with a zero gradient: momentum exactly 0, weights untouched (no decay)
    assert torch.all(fl.gather(mom)[7] == 0) and torch.equal(fl.gather(got_flat)[7], ws[7])
    # an adapted one decays with trust 1: w <- w - lr m, m <- mu m + wd w
    w, m = ws[12].double(), torch.zeros_like(ws[12], dtype=torch.float64)
    for _ in range(4):
        m = MU * m + WD * w
        w = w - LR * m
    torch.testing.assert_close(fl.gather(got_flat)[12].double(), w, atol=1e-6, rtol=1e-6)
    # the slots' padding stays zero in every buffer
    assert torch.all(fl.padding(got_flat) == 0) and torch.all(fl.padding(mom) == 0)
    assert torch.all(fl.padding(param) == 0)


def test_argument_checks():
    fl = _Flat([800, 24], [True, False])
    n = fl.n
    w, m = torch.randn(n, device=DEV), torch.zeros(n, device=DEV)
    g = torch.randn(n, device=DEV)
    fl.coef.fill_(1.0)
    with pytest.raises(RuntimeError, match="master"):
        _C().lars_norm_partials(None, g, w.bfloat16(), fl.items, fl.partials)
    with pytest.raises(RuntimeError, match="master"):
        _C().lars_flat_step(None, m, g, w.bfloat16(), fl.items, fl.coef, LR, MU)
    with pytest.raises(RuntimeError, match="one row per work item"):
        _C().lars_norm_partials(None, g, w, fl.items, fl.partials[:-1].contiguous())
    with pytest.raises(RuntimeError, match="one row per tensor"):
        _C().lars_trust(fl.partials, fl.tensors, fl.coef[:-1].contiguous(), ETA, WD, EPS)
    with pytest.raises(RuntimeError, match="items"):
        _C().lars_flat_step(None, m, g, w, fl.items[:, :2].contiguous(), fl.coef, LR, MU)
    with pytest.raises(RuntimeError, match="coef"):
        _C().lars_flat_step(None, m, g, w, fl.items, fl.coef[:, :2].contiguous(), LR, MU)
    with pytest.raises(RuntimeError, match="items"):
        _C().lars_norm_partials(None, g, w, fl.items.long(), fl.partials)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _C().lars_norm_partials(None, g[:12], w[:12], fl.items, fl.partials)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _C().lars_flat_step(None, m[:12], g[:12], w[:12], fl.items, fl.coef, LR, MU)
    with pytest.raises(RuntimeError, match="GPU"):
        _C().lars_trust(fl.partials.cpu(), fl.tensors, fl.coef, ETA, WD, EPS)


def test_plan_entries_that_do_not_fit_are_skipped():
    """The kernels check every plan entry against the sizes they were given.
    The flats here are the front halves of buffers twice their size, so the
    entries below stay inside allocated memory whatever a kernel does with them."""
    fl = _Flat([800, 24], [True, False])
    n = fl.n
    wbuf, mbuf, gbuf = torch.randn(2 * n, device=DEV), torch.zeros(2 * n, device=DEV), torch.randn(2 * n, device=DEV)
    cbuf = torch.ones(16, 4, device=DEV)
    w, m, g, coef = wbuf[:n], mbuf[:n], gbuf[:n], cbuf[:2]
    w0, bad = wbuf.clone(), fl.items.clone()
    bad[0, 0] = n // 8 - 1   # 100 vectors from the flat's last one
    bad[1, 2] = 7            # no such tensor
    _C().lars_norm_partials(None, g, w, bad, fl.partials)
    _C().lars_flat_step(None, m, g, w, bad, coef, LR, MU)
    torch.cuda.synchronize()
    assert torch.equal(wbuf, w0) and torch.all(mbuf == 0)
    assert torch.all(fl.partials[0] == 0) and torch.all(fl.partials[1] > 0)  # the norm kernel takes no tensor index


def test_non_finite_gradient_stays_in_its_tensor():
    """An infinite |g| gives trust 0 and 0 * inf = NaN at the infinite element
    alone; a NaN |g| poisons the whole tensor.  Neither is skipped or
    special-cased, and the neighbours never see it."""
    sizes, adapted = [800, 24, 808, _C().lars_chunk_elems() + 8], [True, False, True, True]
    torch.manual_seed(5)
    fl = _Flat(sizes, adapted)
    ws = [torch.randn(n, device=DEV) for n in sizes]
    ref, ropt = _oracle(ws)
    param, mom = fl.scatter(ws, F32), torch.zeros(fl.n, device=DEV)
    for bad in (float("inf"), float("nan")):
        gs = [torch.randn(n, device=DEV) * SCALES[i % 3] for i, n in enumerate(sizes)]
        gs[2][5] = bad
        grad = fl.scatter(gs, F32)
        want_t = _oracle_step(ref, ropt, gs, adapted)
        _C().lars_norm_partials(None, grad, param, fl.items, fl.partials)
        _C().lars_trust(fl.partials, fl.tensors, fl.coef, ETA, WD, EPS)
        _C().lars_flat_step(None, mom, grad, param, fl.items, fl.coef, LR, MU)
        torch.testing.assert_close(fl.coef[:, 0].double(), torch.tensor(want_t, dtype=torch.float64, device=DEV),
                                   atol=0, rtol=1e-5, equal_nan=True)
        for i, (got, r) in enumerate(zip(fl.gather(param), ref)):
            torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, equal_nan=True,
                                       msg=lambda s: f"{bad}, tensor {i}: {s}")
            assert torch.isfinite(got).all() == (i != 2)
        if bad == float("inf"):
            assert int(torch.isnan(fl.gather(param)[2]).sum()) == 1
    assert torch.isnan(fl.gather(param)[2]).all()


# --------------------------------------------------------------------------- #
# optimizer level
# --------------------------------------------------------------------------- #
def _two_dtype_params(n_bf16, n_f32, seed=4):
    """The shapes of the AdamW kernel test: a bf16 group and an fp32 group with a 1-D tensor."""
    torch.manual_seed(seed)
    a = torch.randn(n_bf16, device=DEV).bfloat16()
    b = torch.randn(40, n_f32 // 40, device=DEV)
    c = torch.randn(n_f32 // 40, device=DEV)  # 1-D: excluded
    return [torch.nn.Parameter(t.clone()) for t in (a.view(8, -1), b, c)]


def _masters(opt, params):
    """fp32 value of every parameter as the optimizer holds it (master where there is one)."""
    out = {}
    for st in opt._groups:
        src = st.get("master", st["param"])
        for p, off in zip(st["params"], st["offs"]):
            out[id(p)] = src.as_strided(p.shape, p.stride(), off).float()
    return [out[id(p)] for p in params]


def _trusts(opt, params):
    out = {}
    for gi, ratios in enumerate(opt.last_trust_ratios):
        for (p, _off), r in zip(opt._slots(gi), ratios.double().tolist()):
            out[id(p)] = r
    return torch.tensor([out[id(p)] for p in params], dtype=torch.float64)


def test_master_lars_on_a_bf16_and_an_fp32_group():
    params = _two_dtype_params(8 * 300, 40 * 50)
    adapted = [p.dim() > 1 for p in params]
    ref, ropt = _oracle(params)
    opt = MasterLARS(params, **HP)
    assert opt.last_trust_ratios is None and len(opt._groups) == 2
    for _ in range(4):
        for i, p in enumerate(params):
            p.grad.copy_(torch.randn_like(p) * SCALES[i % 3])
        want_t = _oracle_step(ref, ropt, [p.grad.float() for p in params], adapted)
        opt.step()
        torch.testing.assert_close(_trusts(opt, params), torch.tensor(want_t, dtype=torch.float64), atol=0, rtol=1e-5)
    assert [r.dtype for r in opt.last_trust_ratios] == [F32, F32] and opt.last_trust_ratios[0].is_cuda
    lo, hi = opt.last_trust_range()
    assert lo == pytest.approx(min(want_t[:2]), rel=1e-5) and hi == pytest.approx(max(want_t[:2]), rel=1e-5)
    for got, r in zip(_masters(opt, params), ref):
        torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5)
    for p, r, got in zip(params, ref, _masters(opt, params)):
        if p.dtype == BF16:
            torch.testing.assert_close(p.detach().float(), r.detach(), atol=1e-2, rtol=1e-2)
            assert torch.equal(p.detach(), got.bfloat16())


def test_step_captured_in_a_graph_follows_fresh_gradients():
    """Two eager steps, then step() captured once and replayed three times with
    fresh gradients copied into the flat gradient buffers: norms and trust
    ratios are formed on the device on every replay (a value read back to the
    host would be frozen at capture), and nothing is allocated or uploaded in
    the captured step (the plan was built by the first eager step)."""
    params = _two_dtype_params(8 * 300, 40 * 50, seed=6)
    adapted = [p.dim() > 1 for p in params]
    ref, ropt = _oracle(params)
    opt = MasterLARS(params, **HP)
    gen = torch.Generator(device=DEV).manual_seed(7)
    grads = [[(torch.randn(p.shape, device=DEV, generator=gen) * SCALES[(i + t) % 3]).to(p.dtype)
              for i, p in enumerate(params)] for t in range(5)]
    want = []

    def feed(t):
        for p, g in zip(params, grads[t]):
            p.grad.copy_(g)
        want.append(torch.tensor(_oracle_step(ref, ropt, [g.float() for g in grads[t]], adapted),
                                 dtype=torch.float64))

    def check(t):
        for got, r in zip(_masters(opt, params), ref):
            torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, msg=lambda m: f"step {t}: {m}")
        torch.testing.assert_close(_trusts(opt, params), want[t], atol=0, rtol=1e-5)

    for t in range(2):
        feed(t)
        opt.step()
        check(t)
    plans = [id(p["items"]) for p in opt._plans]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    feed(2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    assert plans == [id(p["items"]) for p in opt._plans]
    seen = []
    for t in range(2, 5):
        if t > 2:
            feed(t)
        graph.replay()
        torch.cuda.synchronize()
        check(t)
        seen.append(_trusts(opt, params))
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


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


def test_flat_lars_trains_a_small_resnet_under_ddp(_pg):
    from distributed_model_parallel_amd.models import build_model
    from distributed_model_parallel_amd.ops import wt_cache
    from distributed_model_parallel_amd.ops.loss import cross_entropy
    from distributed_model_parallel_amd.ops.optim import FlatLARS
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    from distributed_model_parallel_amd.utils.precision import cast_model
    torch.manual_seed(0)
    m = build_model("resnet18", num_classes=10).to(DEV).to(memory_format=torch.channels_last)
    cast_model(m, BF16)
    ddp = DistributedDataParallel(m, bucket_cap_mb=4.0, first_bucket_mb=1.0, flat_parameters=True)
    opt = FlatLARS(ddp, **HP)
    plist = list(ddp._params)
    adapted = [p.dim() > 1 for p in plist]
    ref, ropt = _oracle(plist)
    assert any(p.dim() == 4 and not p.is_contiguous() for p in plist), "conv weights are permuted-stride views"
    x = torch.randn(8, 3, 32, 32, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), device=DEV)
    terr = 0.0
    for t in range(3):
        cross_entropy(ddp(x), y).backward()
        wt_cache.transposed(m.fc.weight)  # as a backward wanting W^T does: the optimizer's step keeps it from now on
        flats, layout = ddp.flat_groups(), ddp.param_layout()
        grads = [flats[g][1].as_strided(p.shape, p.stride(), off).float().contiguous()
                 for p, (g, off) in zip(plist, layout)]
        want_t = torch.tensor(_oracle_step(ref, ropt, grads, adapted), dtype=torch.float64)
        opt.step()
        got_t = {}
        for gi, ratios in enumerate(opt.last_trust_ratios):
            for (p, _off), r in zip(opt._slots(gi), ratios.double().tolist()):
                got_t[id(p)] = r
        got_t = torch.tensor([got_t[id(p)] for p in plist], dtype=torch.float64)
        terr = max(terr, float(((got_t - want_t).abs() / want_t).max()))
        torch.testing.assert_close(got_t, want_t, atol=0, rtol=1e-5)
        for p, r, (g, off) in zip(plist, ref, ddp.param_layout()):
            st = opt._flat_state[g]
            got = st.get("master", st["param"]).as_strided(p.shape, p.stride(), off)
            torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, msg=lambda s: f"step {t}: {s}")
            assert torch.equal(p.detach(), got.to(p.dtype))
        # every cached W^T / flipped weight the optimizer owns was refreshed from the UPDATED weight
        seen = 0
        for k, e in wt_cache._GLOBAL.items():
            w = e[0]()
            if w is None or not any(w is p for p in plist) or (len(k) == 3 and k[2] != "flip"):
                continue
            assert e[2] == wt_cache._GEN[0]
            if len(k) == 2:
                assert torch.equal(e[1], w.detach().reshape(w.shape[0], -1).t())
            else:
                assert torch.equal(e[1], w.detach().flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1))
            seen += 1
        assert seen > 0
        opt.zero_grad()
    print("max trust rel err %.2e over %d tensors" % (terr, len(plist)))
    assert opt.state_dict()["steps"] == 3 and opt.state_dict()["kind"] == "lars"
