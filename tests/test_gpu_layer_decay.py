"""adamw_scaled_kernel (csrc/optim/fused_adamw.hip) on the MI355X: the flat AdamW update with a
per-tensor lr scale (one class byte per 8-element vector, a 256-entry table)
against torch.optim.AdamW with one param group per (class, decay); the bits of
``adamw_flat_step`` wherever the scale is 1.0; frozen (scale 0) tensors; the
argument checks; a captured ``MasterAdamW`` step whose scales change between
replays; clipping; ``FlatAdamW`` under DDP and the trainer's ``layer_decay``.

Tolerances are those tests/test_gpu_adamw.py holds the unscaled kernel to:
atol = rtol = 1e-5 on the fp32 weights at lr = 1e-2, 1e-2 on the bf16 working
copy, ``param == master.bfloat16()`` exactly.  They carry over: scales <= 1
shrink the step, and the two extra fp32 roundings (``lr * s``, the decay factor
``fma(-lr s, wd, 1)``) are each half an ulp of a number <= 1, 6e-8, times
|w| < 5 per step: about 1e-6 over 4 steps.
"""
import math

import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops.optim import MasterAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD, B1, B2, EPS = 1e-2, 0.1, 0.9, 0.999, 1e-8
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [(BF16, BF16, True), (F32, F32, False), (F32, BF16, True), (BF16, F32, False)]
NAN = float("nan")
FROZEN = 7  # the class forced to scale 0


def _C():
    return _native.require("gpu tests")


def _sizes():
    return {"one_vector": 8,
            "all_classes": 86 * (8 + 24 + 800),  # 258 segments: every class byte 0..255 is used
            "second_grid_pass": 8 * (_C().adamw_grid_cap() * 256 + 3)}


def _table(kind="mixed"):
    if kind == "ones":
        return torch.ones(256, device=DEV)
    t = torch.tensor([((k * 37) % 256) / 255 for k in range(256)], dtype=torch.float64).float()
    t[0], t[FROZEN] = 1.0, 0.0
    return t.to(DEV)


def _layout(n):
    """Segments cycling 8 / 24 / 800 elements (tests/test_gpu_adamw.py): decay
    alternates, segment i has class i % 256.  Returns per-element decay (bool),
    per-element class (int64), the uint8 decay mask and class bytes per vector."""
    lens, o, i = [], 0, 0
    while o < n:
        ln = min((8, 24, 800)[i % 3], n - o)
        lens.append(ln)
        o += ln
        i += 1
    lens = torch.tensor(lens)
    seg = torch.arange(len(lens))
    vdec = torch.repeat_interleave((seg % 2 == 0), lens // 8)
    vcls = torch.repeat_interleave(seg % 256, lens // 8)
    mask, cls = vdec.to(torch.uint8).to(DEV), vcls.to(torch.uint8).to(DEV)
    return (mask.repeat_interleave(8) != 0), cls.long().repeat_interleave(8), mask, cls


def _problem(n, gdtype, pdtype, steps=4, seed=1):
    torch.manual_seed(seed)
    w0 = torch.randn(n, device=DEV)
    if pdtype == BF16:
        w0 = w0.bfloat16().float()  # master and working copy start equal
    grads = [torch.randn(n, device=DEV).to(gdtype) for _ in range(steps)]
    return w0, grads


def _run_kernel(w0, grads, pdtype, master, mask, cls, table, scaled=True, ema=False):
    n = w0.numel()
    mst = w0.clone() if master else None
    param = w0.clone().to(pdtype)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    e = w0.clone() if ema else None
    hyper = torch.zeros(4, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for g in grads:
        _C().adamw_prepare(None, hyper, step, 0.0, B1, B2)
        if scaled:
            _C().adamw_flat_step_scaled(mst, m, v, g, param, mask, hyper, cls, table, LR, B1, B2, EPS, WD, e,
                                        0.99 if ema else 0.0)
        else:
            _C().adamw_flat_step(mst, m, v, g, param, mask, hyper, LR, B1, B2, EPS, WD, e, 0.99 if ema else 0.0)
    torch.cuda.synchronize()
    return {"w": mst if master else param, "param": param, "m": m, "v": v, "ema": e}


def _torch_oracle(w0, grads, decay, ecls, table, dtype=torch.float32):
    """torch.optim.AdamW, one param group per (class, decay)."""
    groups, refs = [], []
    for k in torch.unique(ecls).tolist():
        for d in (True, False):
            idx = (ecls == k) & (decay == d)
            if idx.any():
                r = w0[idx].to(dtype).clone().requires_grad_()
                refs.append((idx, r))
                groups.append({"params": [r], "lr": LR * float(table[k]), "weight_decay": WD if d else 0.0})
    opt = torch.optim.AdamW(groups, lr=LR, betas=(B1, B2), eps=EPS)
    for g in grads:
        for idx, r in refs:
            r.grad = g[idx].to(dtype)
        opt.step()
    want = torch.empty(w0.numel(), device=DEV, dtype=dtype)
    for idx, r in refs:
        want[idx] = r.detach()
    return want


def _formula64(w0, grads, decay, ecls, table):
    """torch.optim.AdamW's update written out in float64 with a per-element lr = LR * s."""
    lr_e = LR * table.double()[ecls]
    wd_e = decay.double() * WD
    w = w0.double().clone()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    for t, g in enumerate(grads, 1):
        g = g.double()
        w *= 1 - lr_e * wd_e
        m = B1 * m + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        w -= lr_e / (1 - B1 ** t) * m / (v.sqrt() / math.sqrt(1 - B2 ** t) + EPS)
    return w


def _check(out, want, pdtype, master, label):
    got = out["w"]
    assert all(torch.isfinite(out[k]).all() for k in ("w", "m", "v"))
    err = (got.double() - want.double()).abs()
    print(f"{label}: max abs err {float(err.max()):.3g}, max err / (1e-5 + 1e-5 |w|) "
          f"{float((err / (1e-5 + 1e-5 * want.double().abs())).max()):.3g} (bound 1)")
    torch.testing.assert_close(got, want.float(), atol=1e-5, rtol=1e-5)
    if pdtype == BF16:
        torch.testing.assert_close(out["param"].float(), want.float(), atol=1e-2, rtol=1e-2)
        assert torch.equal(out["param"], out["w"].bfloat16())


# --------------------------------------------------------------------------- #
# 1. against the oracle
# --------------------------------------------------------------------------- #
def test_float64_formula_matches_torch_adamw_in_float64():
    """The per-element-lr formula the large case is held to is torch.optim.AdamW:
    both in float64 on `all_classes`, they agree to rounding (1e-12)."""
    n = _sizes()["all_classes"]
    decay, ecls, _mask, _cls = _layout(n)
    assert torch.unique(ecls).numel() == 256
    table = _table()
    w0, grads = _problem(n, F32, F32)
    want = _torch_oracle(w0, grads, decay, ecls, table, dtype=torch.float64)
    got = _formula64(w0, grads, decay, ecls, table)
    err = float((got - want).abs().max())
    print("float64 formula vs float64 torch AdamW: max abs err", err)
    # the same operations in another order: some tens of float64 ulp of |w| < 6 over 4 steps
    assert err <= 1e-12, err


@pytest.mark.parametrize("gdtype,pdtype,master", DTYPES)
@pytest.mark.parametrize("size", ["one_vector", "all_classes", "second_grid_pass"])
def test_scaled_step_matches_the_oracle(gdtype, pdtype, master, size):
    n = _sizes()[size]
    decay, ecls, mask, cls = _layout(n)
    table = _table()
    if size == "one_vector":  # one class in use: every other entry is poison
        table = torch.full((256,), NAN, device=DEV)
        table[0] = 0.5
    w0, grads = _problem(n, gdtype, pdtype)
    out = _run_kernel(w0, grads, pdtype, master, mask, cls, table)
    if size == "second_grid_pass":
        want = _formula64(w0, grads, decay, ecls, table)
    else:
        want = _torch_oracle(w0, [g.float() for g in grads], decay, ecls, table)
    _check(out, want, pdtype, master, f"{size} {gdtype} {pdtype}")
    if size != "one_vector":
        fz = ecls == FROZEN
        assert torch.equal(out["w"][fz], w0[fz]) and bool((out["m"][fz] != 0).all())


# --------------------------------------------------------------------------- #
# 2. the bits of the unscaled kernel
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("gdtype,pdtype,master", DTYPES)
@pytest.mark.parametrize("size", ["all_classes", "second_grid_pass"])
def test_all_ones_table_gives_the_bits_of_adamw_flat_step(gdtype, pdtype, master, size):
    n = _sizes()[size]
    _decay, _ecls, mask, cls = _layout(n)
    w0, grads = _problem(n, gdtype, pdtype, steps=3)
    a = _run_kernel(w0, grads, pdtype, master, mask, cls, None, scaled=False, ema=True)
    b = _run_kernel(w0, grads, pdtype, master, mask, cls, _table("ones"), ema=True)
    for k in ("w", "param", "m", "v", "ema"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("gdtype,pdtype,master", DTYPES)
def test_unit_scale_tensors_in_a_mixed_table_get_the_unscaled_bits(gdtype, pdtype, master):
    n = _sizes()["all_classes"]
    _decay, ecls, mask, cls = _layout(n)
    table = _table()
    unit = table[ecls] == 1
    assert 0 < int(unit.sum()) < n
    w0, grads = _problem(n, gdtype, pdtype, steps=3)
    a = _run_kernel(w0, grads, pdtype, master, mask, cls, None, scaled=False, ema=True)
    b = _run_kernel(w0, grads, pdtype, master, mask, cls, table, ema=True)
    for k in ("w", "param", "m", "v", "ema"):
        assert torch.equal(a[k][unit], b[k][unit]), k
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"])  # the moments do not see the scale
    assert not torch.equal(a["w"][~unit], b["w"][~unit])


# --------------------------------------------------------------------------- #
# 3. frozen tensors
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("pdtype,master", [(BF16, True), (F32, False)])
def test_frozen_tensor_between_two_training_ones_and_slot_padding(pdtype, master):
    """Three adjacent one-vector tensors with scales (1, 0, 0.5); each holds 5
    values and 3 elements of slot padding (weights and gradients zero there)."""
    n = 24
    table = torch.full((256,), NAN, device=DEV)  # unused entries are poison
    table[:3] = torch.tensor([1.0, 0.0, 0.5])
    cls = torch.tensor([0, 1, 2], dtype=torch.uint8, device=DEV)
    mask = torch.ones(3, dtype=torch.uint8, device=DEV)
    pad = (torch.arange(n, device=DEV) % 8) >= 5
    w0, grads = _problem(n, pdtype, pdtype, steps=3, seed=9)
    w0[pad] = 0
    w0[8] = -0.0  # a frozen -0.0 stays -0.0
    for g in grads:
        g[pad] = 0
    out = _run_kernel(w0, grads, pdtype, master, mask, cls, table, ema=True)
    for k in ("w", "param", "m", "v", "ema"):
        assert torch.isfinite(out[k].float()).all(), k
        assert bool((out[k][pad].float() == 0).all()), k  # slot padding stays zero
    mid = slice(8, 16)
    assert torch.equal(out["w"][mid].view(torch.int32), w0[mid].view(torch.int32))
    assert torch.equal(out["param"][mid], w0[mid].to(pdtype))
    assert bool((out["m"][mid][:5] != 0).all()) and bool((out["v"][mid][:5] != 0).all())
    assert torch.equal(out["ema"][mid], w0[mid])  # the EMA's target did not move
    for nb in (slice(0, 5), slice(16, 21)):
        assert bool((out["w"][nb] != w0[nb]).all())


# --------------------------------------------------------------------------- #
# 4. argument checks
# --------------------------------------------------------------------------- #
def test_argument_checks():
    n = 64
    w, m, v, g = (torch.zeros(n, device=DEV) for _ in range(4))
    hyper = torch.tensor([0.1, 0.001, 0.0, 1.0], device=DEV)
    cls, table = torch.zeros(n // 8, dtype=torch.uint8, device=DEV), torch.ones(256, device=DEV)

    def call(cls=cls, table=table, w=w, g=g):
        _C().adamw_flat_step_scaled(None, m, v, g, w, None, hyper, cls, table, LR, B1, B2, EPS, WD)

    call()
    with pytest.raises(RuntimeError, match="lr_class"):
        call(cls=cls.to(torch.int8))
    with pytest.raises(RuntimeError, match="lr_class"):
        call(cls=cls.to(torch.int32))
    for bad in (n // 8 - 1, n // 8 + 1, n):
        with pytest.raises(RuntimeError, match="lr_class"):
            call(cls=torch.zeros(bad, dtype=torch.uint8, device=DEV))
    for bad in (255, 257):
        with pytest.raises(RuntimeError, match="lr_scales"):
            call(table=torch.ones(bad, device=DEV))
    with pytest.raises(RuntimeError, match="lr_scales"):
        call(table=table.double())
    with pytest.raises(RuntimeError, match="lr_scales"):
        call(table=torch.ones(512, device=DEV)[::2])
    with pytest.raises(RuntimeError, match="lr_class"):
        call(cls=cls.cpu())
    with pytest.raises(RuntimeError, match="lr_scales"):
        call(table=table.cpu())
    with pytest.raises(RuntimeError, match="master"):
        call(w=w.bfloat16())
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _C().adamw_flat_step_scaled(None, m[:12], v[:12], g[:12], w[:12], None, hyper, cls[:1], table, LR, B1, B2,
                                    EPS, WD)
    torch.cuda.synchronize()
    assert bool((w == 0).all())


# --------------------------------------------------------------------------- #
# 5 / 6. MasterAdamW: graph capture, clipping
# --------------------------------------------------------------------------- #
def _two_dtype_params(n_bf16, n_f32, seed=4):
    torch.manual_seed(seed)
    a = torch.randn(n_bf16, device=DEV).bfloat16()
    b = torch.randn(40, n_f32 // 40, device=DEV)
    c = torch.randn(n_f32 // 40, device=DEV)  # 1-D: no decay
    return [torch.nn.Parameter(t.clone()) for t in (a.view(8, -1), b, c)]


def _stock(params, scales):
    ref = [p.detach().float().clone().requires_grad_() for p in params]
    opt = torch.optim.AdamW([{"params": [r], "lr": LR * s, "weight_decay": WD if r.dim() > 1 else 0.0}
                             for r, s in zip(ref, scales)], lr=LR, betas=(B1, B2), eps=EPS)
    return ref, opt


def _masters(opt, params):
    out = {}
    for st in opt._groups:
        src = st.get("master", st["param"])
        for p, off in zip(st["params"], st["offs"]):
            out[id(p)] = src.as_strided(p.shape, p.stride(), off).float()
    return [out[id(p)] for p in params]


def test_clipping_composes_with_the_scales():
    params = _two_dtype_params(8 * 300, 40 * 50)
    scales = (0.5, 1.0, 0.25)
    ref, ropt = _stock(params, scales)
    opt = MasterAdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.5,
                      lr_scales=dict(zip(params, scales)))
    for _ in range(4):
        for p, r in zip(params, ref):
            p.grad.copy_(torch.randn_like(p))
            r.grad = p.grad.detach().float().clone()
        want_norm = torch.cat([r.grad.double().flatten() for r in ref]).norm()
        assert float(torch.nn.utils.clip_grad_norm_(ref, 0.5)) > 0.5
        ropt.step()
        opt.step()
        torch.testing.assert_close(opt.last_grad_norm.double(), want_norm, atol=0, rtol=1e-5)
    for got, r in zip(_masters(opt, params), ref):
        print("clipped + scaled: max abs err", float((got - r.detach()).abs().max()))
        torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5)
    for p, r in zip(params, ref):
        if p.dtype == BF16:
            torch.testing.assert_close(p.detach().float(), r.detach(), atol=1e-2, rtol=1e-2)


def test_captured_step_reads_the_scales_of_the_replay():
    """One eager step, then step() captured once: replays follow the eager
    oracle, and after set_lr_scales the NEXT replay uses the new scales (class
    bytes and table are rewritten in place; nothing is captured again)."""
    params = _two_dtype_params(8 * 300, 40 * 50, seed=6)
    scales, later = (0.5, 1.0, 0.0), (1.0, 0.25, 0.75)
    ref, ropt = _stock(params, scales)
    opt = MasterAdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.5,
                      lr_scales=dict(zip(params, scales)))
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

    feed(0)
    opt.step()
    check(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    feed(1)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    frozen0 = _masters(opt, params)[2].clone()
    for t in (1, 2):
        if t > 1:
            feed(t)
        graph.replay()
        torch.cuda.synchronize()
        check(t)
    assert torch.equal(_masters(opt, params)[2], frozen0)  # scale 0 so far
    opt.set_lr_scales(dict(zip(params, later)))
    for grp, s in zip(ropt.param_groups, later):
        grp["lr"] = LR * s
    for t in (3, 4):
        feed(t)
        graph.replay()
        torch.cuda.synchronize()
        check(t)
    assert not torch.equal(_masters(opt, params)[2], frozen0)
    assert opt.state_dict()["steps"] == 5


# --------------------------------------------------------------------------- #
# 7 / 8. model level
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


def test_flat_adamw_with_layer_decay_trains_vit_tiny_under_ddp(_pg):
    from distributed_model_parallel_amd.models import build_model, layer_decay_scales
    from distributed_model_parallel_amd.ops.loss import cross_entropy
    from distributed_model_parallel_amd.ops.optim import FlatAdamW
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    from distributed_model_parallel_amd.utils.precision import cast_model
    torch.manual_seed(0)
    m = build_model("vit_tiny", num_classes=10).to(DEV).to(memory_format=torch.channels_last)
    cast_model(m, BF16)
    scales = layer_decay_scales(m, 0.75)  # on the bare model
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.25, first_bucket_mb=0.05, flat_parameters=True)
    opt = FlatAdamW(ddp, lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, lr_scales=scales)
    L = len(m.blocks)
    assert opt.lr_scale_range() == (0.75 ** (L + 1), 1.0)
    plist = list(ddp._params)
    ref = [p.detach().float().clone().requires_grad_() for p in plist]
    ropt = torch.optim.AdamW([{"params": [r], "lr": 1e-3 * opt.lr_scale_of(p),
                               "weight_decay": WD if r.dim() > 1 else 0.0} for p, r in zip(plist, ref)],
                             lr=1e-3, betas=(B1, B2), eps=EPS)
    x = torch.randn(16, 3, 32, 32, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,), device=DEV)
    for t in range(3):
        cross_entropy(ddp(x), y).backward()
        flats, layout = ddp.flat_groups(), ddp.param_layout()
        for p, r, (g, off) in zip(plist, ref, layout):
            r.grad = flats[g][1].as_strided(p.shape, p.stride(), off).float().contiguous()
        ropt.step()
        opt.step()
        worst = 0.0
        for p, r, (g, off) in zip(plist, ref, ddp.param_layout()):
            st = opt._flat_state[g]
            got = st.get("master", st["param"]).as_strided(p.shape, p.stride(), off)
            worst = max(worst, float((got - r.detach()).abs().max()))
            torch.testing.assert_close(got, r.detach(), atol=1e-5, rtol=1e-5, msg=lambda s: f"step {t}: {s}")
            assert torch.equal(p.detach(), got.to(p.dtype))
            d = opt._lr_dev[g]  # the class bytes follow the (possibly rebuilt) layout
            sc = d["table"][d["cls"][off // 8:(off + p.numel() + 7) // 8].long()]
            assert bool((sc == scales[p]).all())
        print(f"step {t}: max abs err vs grouped AdamW {worst:.3g}")
        opt.zero_grad()
    assert opt.state_dict()["steps"] == 3


def test_train_state_with_layer_decay_runs_a_step():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    cfg = StepConfig(model="vit_tiny", optimizer="adamw", layer_decay=0.75, parallel="none", batch_size=8,
                     lr=1e-3, weight_decay=0.05)
    st = build_train_state(cfg, torch.device(DEV))
    L = len(st.model.blocks)
    assert st.optimizer.lr_scaled and st.optimizer.lr_scale_range() == (0.75 ** (L + 1), 1.0)
    before = st.model.head.weight.detach().clone()
    loss = st.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach()))
    assert st.optimizer._lr_key is not None, "the scaled kernel's tensors were built"
    assert not torch.equal(st.model.head.weight.detach(), before)
