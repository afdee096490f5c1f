"""MasterAdamW / FlatAdamW on the CPU path (``_adamw_reference``): parity with
torch.optim.AdamW built with the usual decay / no-decay param groups, with and
without ``clip_grad_norm_``; fp32 masters for bf16 weights; checkpoint
round-trip; SGD <-> AdamW foreign-state rejection; state and decay mask across
the DDP bucket rebuild; the trainer's StepConfig and CLI flags."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dist_utils import run_world
from distributed_model_parallel_amd.ops.optim import (FlatAdamW, FlatSGD, ForeignOptimizerState,
                                                      MasterAdamW, MasterSGD, _adamw_reference)

LR, WD = 1e-2, 0.1


class _MLP(nn.Module):
    """Registration order (head first) differs from the autograd-ready order,
    so a DDP bucket rebuild really changes the flat layout."""

    def __init__(self):
        super().__init__()
        self.head = nn.Linear(32, 5)
        self.body = nn.Sequential(nn.Linear(12, 32), nn.LayerNorm(32), nn.ReLU(), nn.Linear(32, 32))

    def forward(self, x):
        return self.head(F.relu(self.body(x)))


def _mlp(dtype=torch.float32):
    torch.manual_seed(0)
    return _MLP().to(dtype)


def _two_group_adamw(params, **kw):
    """Stock AdamW the way ViT recipes build it: no decay for ndim <= 1."""
    params = list(params)
    return torch.optim.AdamW([{"params": [p for p in params if p.dim() > 1], "weight_decay": WD},
                              {"params": [p for p in params if p.dim() <= 1], "weight_decay": 0.0}],
                             lr=LR, **kw)


def _batches(n):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(8, 12, generator=g), torch.randint(0, 5, (8,), generator=g)) for _ in range(n)]


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_master_adamw_matches_torch_adamw_fp32(max_norm):
    a, b = _mlp(), _mlp()
    oa = _two_group_adamw(a.parameters())
    ob = MasterAdamW(b.parameters(), lr=LR, weight_decay=WD, max_grad_norm=max_norm)
    norms = []
    for x, y in _batches(5):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            F.cross_entropy(m(x), y).backward()
            if o is oa and max_norm:
                norms.append(torch.nn.utils.clip_grad_norm_(a.parameters(), max_norm))
            o.step()
        if max_norm:
            torch.testing.assert_close(ob.last_grad_norm, norms[-1], atol=0, rtol=1e-5)
    if max_norm:
        assert max(norms) > max_norm, "the test must exercise a clipped step"
    else:
        assert ob.last_grad_norm is None
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        torch.testing.assert_close(va, vb, atol=1e-6, rtol=1e-5, msg=k)
    st = ob._groups[0]
    assert all(p.grad.data_ptr() >= st["grad"].data_ptr() for p in b.parameters())
    assert int(ob._dev_state[torch.device("cpu")]["step"]) == 5


def test_adamw_reference_fp32_close_to_float64_adamw():
    """The GPU kernel test compares fp32 results at atol = rtol = 1e-5; that
    bound is sound only if fp32 arithmetic itself stays well inside it: the
    fp32 reference must stay within a tenth of it of a float64 AdamW."""
    n = 8 * 1024
    g = torch.Generator().manual_seed(2)
    w0 = torch.randn(n, generator=g)
    ref = w0.double().clone().requires_grad_()
    opt = torch.optim.AdamW([ref], lr=LR, weight_decay=WD)
    w, m, v = w0.clone(), torch.zeros(n), torch.zeros(n)
    cfg = {"lr": LR, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": WD}
    for t in range(1, 5):
        gr = torch.randn(n, generator=g)
        gr[:64] = 0.0
        ref.grad = gr.double()
        opt.step()
        hyper = torch.tensor([1 - 0.9 ** t, 1 - 0.999 ** t, 0.0, 1.0])
        _adamw_reference(None, m, v, gr, w, None, hyper, cfg)
    err = (w.double() - ref.detach()).abs()
    assert float((err - 1e-6 * ref.detach().abs()).max()) <= 1e-6, float(err.max())


def test_master_adamw_keeps_sub_ulp_bf16_updates():
    p = nn.Parameter(torch.ones(16, dtype=torch.bfloat16))
    q = nn.Parameter(torch.ones(16, dtype=torch.bfloat16))
    om = MasterAdamW([p], lr=1e-3, weight_decay=0.0)
    ot = torch.optim.AdamW([q], lr=1e-3, weight_decay=0.0)
    for _ in range(10):
        for t, o in ((p, om), (q, ot)):
            o.zero_grad()
            t.float().sum().backward()  # constant gradient: every step moves by lr = 1e-3 < half a bf16 ulp at 1.0
            o.step()
    assert torch.all(q == 1.0), "plain bf16 AdamW drops the update (what the master fixes)"
    torch.testing.assert_close(om._groups[0]["master"][:16], torch.full((16,), 0.99), atol=1e-6, rtol=0)
    assert torch.all(p < 1.0)


def test_no_decay_1d_mask_and_full_decay():
    m = _mlp()
    o = MasterAdamW(m.parameters(), lr=LR, weight_decay=WD)
    for p in m.parameters():
        p.grad.zero_()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    o.step()  # zero gradients: only decay moves anything
    for k, v in m.state_dict().items():
        if v.dim() <= 1:
            assert torch.equal(v, before[k]), k
        else:
            torch.testing.assert_close(v, before[k] * (1 - LR * WD), atol=1e-7, rtol=1e-6, msg=k)
    m2 = _mlp()
    o2 = MasterAdamW(m2.parameters(), lr=LR, weight_decay=WD, no_decay_1d=False)
    o2.step()
    for k, v in m2.state_dict().items():
        torch.testing.assert_close(v, before[k] * (1 - LR * WD), atol=1e-7, rtol=1e-6, msg=k)


def test_master_adamw_checkpoint_roundtrip_resumes(tmp_path):
    from distributed_model_parallel_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    data = _batches(5)

    def run(m, o, batches):
        for x, y in batches:
            o.zero_grad()
            F.cross_entropy(m(x), y).backward()
            o.step()

    a = _mlp()
    oa = MasterAdamW(a.parameters(), lr=LR, weight_decay=WD, max_grad_norm=0.5)
    run(a, oa, data[:3])
    path = save_checkpoint(str(tmp_path / "ck.pth"), a, oa, epoch=1)
    sd = oa.state_dict()
    assert sd["kind"] == "adamw" and sd["steps"] == 3 and "numels" in sd
    assert set(sd["flat_state"][0]) == {"exp_avg", "exp_avg_sq"}  # fp32 model: no separate master
    run(a, oa, data[3:])
    b = _mlp()
    with torch.no_grad():
        for p in b.parameters():
            p.add_(1.0)
    ob = MasterAdamW(b.parameters(), lr=LR, weight_decay=WD, max_grad_norm=0.5)
    load_checkpoint(path, b, ob, restore_rng=False)
    assert ob.state_dict()["steps"] == 3
    torch.testing.assert_close(ob._groups[0]["exp_avg"], torch.load(path, weights_only=False)["optimizer"]
                               ["flat_state"][0]["exp_avg"])
    run(b, ob, data[3:])
    assert ob.state_dict()["steps"] == 5
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        torch.testing.assert_close(va, vb, atol=1e-7, rtol=1e-6, msg=k)


def test_bf16_state_dict_carries_master():
    m = _mlp(torch.bfloat16)
    o = MasterAdamW(m.parameters(), lr=LR)
    assert set(o.state_dict()["flat_state"][0]) == {"exp_avg", "exp_avg_sq", "master"}


def test_foreign_state_rejected_both_ways():
    sgd = MasterSGD(_mlp().parameters(), lr=0.1, momentum=0.9)
    adamw = MasterAdamW(_mlp().parameters(), lr=LR)
    with pytest.raises(ForeignOptimizerState):
        sgd.load_state_dict(adamw.state_dict())  # same keys and numels: only 'kind' tells them apart
    with pytest.raises(ForeignOptimizerState):
        adamw.load_state_dict(sgd.state_dict())
    with pytest.raises(ForeignOptimizerState):
        adamw.load_state_dict(torch.optim.AdamW(_mlp().parameters(), lr=LR).state_dict())
    sgd.load_state_dict(MasterSGD(_mlp().parameters(), lr=0.1, momentum=0.9).state_dict())  # own kind loads


def test_foreign_adamw_state_in_checkpoint_is_tolerated_by_sgd(tmp_path):
    """load_checkpoint keys on ForeignOptimizerState: an AdamW run resumed with
    --optimizer sgd warns and starts the optimizer fresh."""
    import warnings
    from distributed_model_parallel_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    a = _mlp()
    path = save_checkpoint(str(tmp_path / "ck.pth"), a, MasterAdamW(a.parameters(), lr=LR), epoch=0)
    b = _mlp()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        load_checkpoint(path, b, MasterSGD(b.parameters(), lr=0.1, momentum=0.9), restore_rng=False)
    assert any("optimizer state not restored" in str(x.message) for x in w)


def test_unsupported_options_raise():
    with pytest.raises(ValueError, match="amsgrad"):
        MasterAdamW(_mlp().parameters(), lr=LR, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        MasterAdamW(_mlp().parameters(), lr=LR, maximize=True)
    ps = list(_mlp().parameters())
    with pytest.raises(ValueError, match="one param group"):
        MasterAdamW([{"params": ps[:2]}, {"params": ps[2:]}], lr=LR)
    o = MasterAdamW(ps, lr=LR)
    with pytest.raises(ValueError, match="one param group"):
        o.add_param_group({"params": [nn.Parameter(torch.zeros(3))]})


def test_clipping_needs_one_device():
    ps = [nn.Parameter(torch.zeros(8)), nn.Parameter(torch.zeros(8, device="meta"))]
    with pytest.raises(ValueError, match="one device"):
        MasterAdamW(ps, lr=LR, max_grad_norm=1.0)


# --------------------------------------------------------------------------- #
def _flat_worker(rank, world):
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    torch.manual_seed(0)
    m = _MLP()
    ref = _mlp()
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.002, first_bucket_mb=0.0005, flat_parameters=True)
    opt = FlatAdamW(ddp, lr=LR, weight_decay=WD, max_grad_norm=0.5)
    oref = _two_group_adamw(ref.parameters())
    layouts, masks_ok, state_ok = [list(ddp.param_layout())], [], []
    for x, y in _batches(3):
        opt.zero_grad()
        oref.zero_grad()
        F.cross_entropy(ddp(x), y).backward()
        F.cross_entropy(ref(x), y).backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
        opt.step()
        oref.step()
        layouts.append(list(ddp.param_layout()))
        # per parameter, wherever the current layout put it
        ok, mk = True, True
        for p, q, (g, off) in zip(ddp._params, ref.parameters(), ddp.param_layout()):
            st, n = opt._flat_state[g], p.numel()
            s = oref.state[q]
            for key, want in (("exp_avg", s["exp_avg"]), ("exp_avg_sq", s["exp_avg_sq"])):
                ok &= torch.allclose(st[key].narrow(0, off, n), want.flatten(), atol=1e-7, rtol=1e-5)
            ok &= torch.allclose(st["param"].narrow(0, off, n), q.detach().flatten(), atol=1e-6, rtol=1e-5)
            bits = opt._masks[g][off // 8:(off + n + 7) // 8]
            mk &= bool(torch.all(bits == (1 if p.dim() > 1 else 0)))
        state_ok.append(ok)
        masks_ok.append(mk)
    sd = opt.state_dict()
    foreign = []
    for o, state in ((FlatSGD(ddp, lr=0.1, momentum=0.9), sd),
                     (opt, FlatSGD(ddp, lr=0.1, momentum=0.9).state_dict())):
        try:
            o.load_state_dict(state)
            foreign.append(False)
        except ForeignOptimizerState:
            foreign.append(True)
    return {"foreign": foreign, "layouts": layouts, "state_ok": state_ok, "masks_ok": masks_ok, "kind": sd["kind"],
            "steps": sd["steps"], "has_layout": "layout" in sd,
            "norm": float(opt.last_grad_norm)}


def test_flat_adamw_state_and_mask_follow_bucket_rebuild():
    res = run_world(_flat_worker, 1)[0]
    assert res["layouts"][0] != res["layouts"][-1], "test must exercise a layout change"
    assert res["state_ok"] == [True] * 3
    assert res["masks_ok"] == [True] * 3
    assert res["kind"] == "adamw" and res["steps"] == 3 and res["has_layout"]
    assert res["norm"] > 0
    assert res["foreign"] == [True, True]  # FlatSGD <- adamw state, FlatAdamW <- sgd state


def _flat_bf16_worker(rank, world, path):
    """bf16 under DDP: masters and moments resume across save / fresh-layout load."""
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel

    def make():
        torch.manual_seed(0)
        m = _MLP().to(torch.bfloat16)
        ddp = DistributedDataParallel(m, bucket_cap_mb=0.002, first_bucket_mb=0.0005, flat_parameters=True)
        return m, ddp, FlatAdamW(ddp, lr=LR, weight_decay=WD)

    data = [(x.bfloat16(), y) for x, y in _batches(4)]

    def run(ddp, opt, batches):
        for x, y in batches:
            opt.zero_grad()
            F.cross_entropy(ddp(x).float(), y).backward()
            opt.step()

    m, ddp, opt = make()
    run(ddp, opt, data[:2])
    torch.save({"net": m.state_dict(), "opt": opt.state_dict()}, path)
    run(ddp, opt, data[2:])
    m2, ddp2, opt2 = make()
    ck = torch.load(path, weights_only=True)
    m2.load_state_dict(ck["net"])
    opt2.load_state_dict(ck["opt"])
    run(ddp2, opt2, data[2:])
    same = all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    masters = []
    for o, d in ((opt, ddp), (opt2, ddp2)):
        masters.append([o._flat_state[g]["master"].narrow(0, off, p.numel()).clone()
                        for p, (g, off) in zip(d._params, d.param_layout())])
    msame = all(torch.equal(a, b) for a, b in zip(*masters))
    return {"same": same, "masters_same": msame, "steps": opt2.state_dict()["steps"]}


def test_flat_adamw_bf16_resume_across_bucket_rebuild(tmp_path):
    res = run_world(_flat_bf16_worker, 1, str(tmp_path / "ck.pt"))[0]
    assert res["same"] and res["masters_same"] and res["steps"] == 4


# --------------------------------------------------------------------------- #
def test_step_config_builds_adamw_and_trains_vit_tiny():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    cfg = StepConfig(model="vit_tiny", optimizer="adamw", clip_grad_norm=1.0, parallel="none",
                     dtype=torch.float32, batch_size=8, lr=1e-3, weight_decay=0.05, channels_last=False)
    st = build_train_state(cfg, torch.device("cpu"))
    assert isinstance(st.optimizer, MasterAdamW)
    losses = [float(st.step().detach()) for _ in range(3)]
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert losses[0] > losses[1] > losses[2], losses
    assert float(st.optimizer.last_grad_norm) > 0
    sgd = build_train_state(StepConfig(model="vit_tiny", parallel="none", dtype=torch.float32, batch_size=8,
                                       channels_last=False), torch.device("cpu"))
    assert isinstance(sgd.optimizer, MasterSGD)  # the default stays SGD


def test_step_config_rejects_clipping_with_sgd():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    with pytest.raises(ValueError, match="adamw"):
        build_train_state(StepConfig(model="vit_tiny", clip_grad_norm=1.0, parallel="none",
                                     dtype=torch.float32, batch_size=4, channels_last=False),
                          torch.device("cpu"))


def test_cli_flags_and_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert (a.optimizer, a.betas, a.eps, a.clip_grad_norm, a.lr, a.weight_decay) == \
        ("sgd", (0.9, 0.999), 1e-8, 0.0, 0.4, 1e-4)
    a = p.parse_args(["--optimizer", "adamw", "--betas", "0.9,0.95", "--eps", "1e-6", "--clip-grad-norm", "1.0",
                      "--parallel", "pipe"])
    check_args(p, a)  # a one-stage pipeline may clip
    assert a.betas == (0.9, 0.95) and a.eps == 1e-6 and a.clip_grad_norm == 1.0
    for argv, msg in ((["--clip-grad-norm", "1.0"], "--optimizer adamw"),
                      (["--optimizer", "adamw", "--clip-grad-norm", "1.0", "--parallel", "pipe",
                        "--world-size", "2"], "cross-stage"),
                      (["--optimizer", "adamw", "--betas", "0.9"], "B1,B2"),
                      (["--optimizer", "lamb"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_cli_synthetic_data_follows_a_vits_own_shape():
    """The quick-start ViT command (--synthetic, default -type) gets 224-px, 1000-class data."""
    from distributed_model_parallel_amd.train.cli import _num_classes, _synthetic_kind, build_parser
    p = build_parser()
    for arch, kind, ncls in (("vit_b_16", "Synthetic", 1000), ("vit_tiny", "SyntheticCIFAR", 10),
                             ("mobilenetv2", "SyntheticCIFAR", 10), ("resnet50", "SyntheticCIFAR", 10)):
        a = p.parse_args(["--synthetic", "--arch", arch])
        assert (_synthetic_kind(a), _num_classes(a)) == (kind, ncls), arch
