"""MasterLARS / FlatLARS on the CPU path (``_lars_reference``) against an oracle
written here: per tensor the trust ratio in float64 from the definition,
``d = trust (g + wd w)`` handed as the gradient to a stock
``torch.optim.SGD(lr, momentum, weight_decay=0)`` on an fp32 copy, so the
momentum semantics are stock PyTorch's.  Also: fp32 masters for bf16 weights,
``exclude_1d``, the exact-zero norms, state and trust ratios across the DDP
bucket rebuild, checkpoint round trip, foreign-state rejection, the trainer's
StepConfig / CLI flags and one synthetic trainer run.

Hyper-parameters: eta = 1 (not a training value): with eta = 1e-3 every update
would be ~1e-5 and a wrong trust ratio would hide inside the tolerance."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dist_utils import run_world
from distributed_model_parallel_amd.ops.optim import (FlatLARS, FlatSGD, ForeignOptimizerState, MasterAdamW,
                                                      MasterLARS, MasterSGD, build_optimizer)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MU, WD, ETA, EPS = 1e-2, 0.9, 0.1, 1.0, 1e-8
HP = dict(lr=LR, momentum=MU, weight_decay=WD, trust_coefficient=ETA, eps=EPS)


class _MLP(nn.Module):
    """The small MLP of tests/test_adamw.py: registration order (head first)
    differs from the autograd-ready order, so a DDP bucket rebuild really
    changes the flat layout."""

    def __init__(self):
        super().__init__()
        self.head = nn.Linear(32, 5)
        self.body = nn.Sequential(nn.Linear(12, 32), nn.LayerNorm(32), nn.ReLU(), nn.Linear(32, 32))

    def forward(self, x):
        return self.head(F.relu(self.body(x)))


def _mlp(dtype=torch.float32):
    torch.manual_seed(0)
    return _MLP().to(dtype)


def _batches(n):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(8, 12, generator=g), torch.randint(0, 5, (8,), generator=g)) for _ in range(n)]


# --------------------------------------------------------------------------- #
# the oracle
# --------------------------------------------------------------------------- #
def _oracle(params):
    ref = [p.detach().float().clone().requires_grad_() for p in params]
    return ref, torch.optim.SGD(ref, lr=LR, momentum=MU, weight_decay=0.0)


def _oracle_step(ref, ropt, grads, exclude_1d=True):
    """One LARS step of the definition; returns the float64 trust ratios."""
    trusts = []
    for r, g in zip(ref, grads):
        w, g = r.detach().double(), g.detach().double()
        if exclude_1d and r.dim() <= 1:
            trust, d = 1.0, g
        else:
            wn, gn = float(w.norm()), float(g.norm())
            trust = 1.0 if wn == 0.0 or gn == 0.0 else ETA * wn / (gn + WD * wn + EPS)
            d = trust * (g + WD * w)
        r.grad = d.float().reshape(r.shape)
        trusts.append(trust)
    ropt.step()
    return trusts


def _masters(opt, params):
    """fp32 value of every parameter as the optimizer holds it (master where there is one)."""
    out = {}
    for st in opt._groups:
        src = st.get("master", st["param"])
        for p, off in zip(st["params"], st["offs"]):
            out[id(p)] = src.as_strided(p.shape, p.stride(), off).float()
    return [out[id(p)] for p in params]


def _trusts(opt, params):
    """Trust ratio per parameter, from ``last_trust_ratios`` (``_slots`` order per group)."""
    out = {}
    for gi, ratios in enumerate(opt.last_trust_ratios):
        for (p, _off), r in zip(opt._slots(gi), ratios.tolist()):
            out[id(p)] = r
    return [out[id(p)] for p in params]


# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_master_lars_matches_oracle(dtype):
    m = _mlp(dtype)
    params = list(m.parameters())
    ref, ropt = _oracle(params)
    opt = MasterLARS(params, **HP)
    assert opt.last_trust_ratios is None
    for x, y in _batches(5):
        opt.zero_grad()
        F.cross_entropy(m(x.to(dtype)).float(), y).backward()
        want = _oracle_step(ref, ropt, [p.grad.float() for p in params])  # same gradients: optimizers compared
        opt.step()
        torch.testing.assert_close(torch.tensor(_trusts(opt, params), dtype=torch.float64),
                                   torch.tensor(want, dtype=torch.float64), atol=0, rtol=1e-5)
    assert any(abs(t - 1.0) > 0.5 for t in want), "the test must exercise trust ratios away from 1"
    for (k, _v), got, r, p in zip(m.named_parameters(), _masters(opt, params), ref, params):
        torch.testing.assert_close(got, r.detach(), atol=1e-6, rtol=1e-5, msg=lambda s: f"{k}: {s}")
        if dtype == torch.bfloat16:
            assert torch.equal(p.detach(), got.bfloat16()), k
            torch.testing.assert_close(p.detach().float(), r.detach(), atol=1e-2, rtol=1e-2)
    st = opt._groups[0]
    assert ("master" in st) == (dtype == torch.bfloat16)
    assert all(p.grad.data_ptr() >= st["grad"].data_ptr() for p in params)


def test_excluded_tensors_get_plain_momentum_and_no_decay():
    m = _mlp()
    params = list(m.parameters())
    before = [p.detach().clone() for p in params]
    opt = MasterLARS(params, **HP)
    grads = [torch.randn_like(p) for p in params]
    for p, g in zip(params, grads):
        p.grad.copy_(g)
    opt.step()
    for p, b, g, t in zip(params, before, grads, _trusts(opt, params)):
        if p.dim() <= 1:
            assert t == 1.0
            torch.testing.assert_close(p.detach(), b - LR * g, atol=1e-7, rtol=1e-6)  # no decay, trust 1
        else:
            assert t != 1.0


def test_exclude_1d_false_adapts_and_decays_biases_too():
    m = _mlp()
    params = list(m.parameters())
    ref, ropt = _oracle(params)
    opt = MasterLARS(params, exclude_1d=False, **HP)
    for x, y in _batches(3):
        opt.zero_grad()
        F.cross_entropy(m(x), y).backward()
        want = _oracle_step(ref, ropt, [p.grad for p in params], exclude_1d=False)
        opt.step()
    got_t = _trusts(opt, params)
    torch.testing.assert_close(torch.tensor(got_t, dtype=torch.float64), torch.tensor(want, dtype=torch.float64),
                               atol=0, rtol=1e-5)
    assert all(t != 1.0 for p, t in zip(params, got_t) if p.dim() <= 1)
    for got, r in zip(_masters(opt, params), ref):
        torch.testing.assert_close(got, r.detach(), atol=1e-6, rtol=1e-5)


def test_zero_weights_and_zero_gradients_get_trust_one_and_stay_finite():
    torch.manual_seed(1)
    zero_w = nn.Parameter(torch.zeros(6, 10))   # e.g. a ViT's zero-initialised head
    zero_g = nn.Parameter(torch.randn(6, 10))   # e.g. an unused parameter
    plain = nn.Parameter(torch.randn(6, 10))
    params = [zero_w, zero_g, plain]
    ref, ropt = _oracle(params)
    opt = MasterLARS(params, **HP)
    for _ in range(3):
        grads = [torch.randn(6, 10), torch.zeros(6, 10), torch.randn(6, 10)]
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        want = _oracle_step(ref, ropt, grads)
        opt.step()
        got = _trusts(opt, params)
        assert got[1] == 1.0 and want[1] == 1.0
        torch.testing.assert_close(torch.tensor(got, dtype=torch.float64), torch.tensor(want, dtype=torch.float64),
                                   atol=0, rtol=1e-5)
        if _ == 0:
            assert got[0] == 1.0  # |w| = 0 on the first step only
    for p, r in zip(params, ref):
        assert torch.isfinite(p).all()
        torch.testing.assert_close(p.detach(), r.detach(), atol=1e-6, rtol=1e-5)
    assert torch.isfinite(opt._groups[0]["momentum"]).all()


def test_checkpoint_roundtrip_continues_bit_identically(tmp_path):
    from distributed_model_parallel_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    data = _batches(5)

    def run(m, o, batches):
        for x, y in batches:
            o.zero_grad()
            F.cross_entropy(m(x), y).backward()
            o.step()

    a = _mlp()
    oa = MasterLARS(a.parameters(), **HP)
    run(a, oa, data[:3])
    path = save_checkpoint(str(tmp_path / "ck.pth"), a, oa, epoch=1)
    sd = oa.state_dict()
    assert sd["kind"] == "lars" and sd["steps"] == 3 and "numels" in sd
    assert set(sd["flat_state"][0]) == {"momentum"}
    assert sd["param_groups"][0]["trust_coefficient"] == ETA
    run(a, oa, data[3:])
    b = _mlp()
    with torch.no_grad():
        for p in b.parameters():
            p.add_(1.0)
    ob = MasterLARS(b.parameters(), lr=0.5, momentum=0.0, weight_decay=0.0, trust_coefficient=0.5)
    load_checkpoint(path, b, ob, restore_rng=False)
    assert ob.state_dict()["steps"] == 3 and ob.param_groups[0]["trust_coefficient"] == ETA
    run(b, ob, data[3:])
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(va, vb), k
    assert torch.equal(oa._groups[0]["momentum"], ob._groups[0]["momentum"])
    m16 = _mlp(torch.bfloat16)
    assert set(MasterLARS(m16.parameters(), **HP).state_dict()["flat_state"][0]) == {"momentum", "master"}


def test_foreign_state_rejected_both_ways():
    sgd = MasterSGD(_mlp().parameters(), lr=0.1, momentum=0.9)
    adamw = MasterAdamW(_mlp().parameters(), lr=LR)
    lars = MasterLARS(_mlp().parameters(), **HP)
    for dst, src in ((lars, sgd), (sgd, lars), (lars, adamw), (adamw, lars)):
        with pytest.raises(ForeignOptimizerState):
            dst.load_state_dict(src.state_dict())
    with pytest.raises(ForeignOptimizerState):
        lars.load_state_dict(torch.optim.SGD(_mlp().parameters(), lr=LR, momentum=MU).state_dict())
    lars.load_state_dict(MasterLARS(_mlp().parameters(), **HP).state_dict())  # own kind loads


def test_options_are_checked():
    ps = list(_mlp().parameters())
    with pytest.raises(ValueError, match="one param group"):
        MasterLARS([{"params": ps[:2]}, {"params": ps[2:]}], lr=LR)
    o = MasterLARS(ps, lr=LR)
    with pytest.raises(ValueError, match="one param group"):
        o.add_param_group({"params": [nn.Parameter(torch.zeros(3))]})
    with pytest.raises(ValueError, match="trust_coefficient"):
        MasterLARS(_mlp().parameters(), lr=LR, trust_coefficient=0.0)
    assert o.param_groups[0]["trust_coefficient"] == 1e-3 and o.param_groups[0]["eps"] == 1e-8
    assert o.param_groups[0]["momentum"] == 0.9 and o.param_groups[0]["weight_decay"] == 1e-4 and o.exclude_1d


# --------------------------------------------------------------------------- #
def _flat_worker(rank, world):
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    torch.manual_seed(0)
    m = _MLP()
    ref = _mlp()
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.002, first_bucket_mb=0.0005, flat_parameters=True)
    opt = FlatLARS(ddp, **HP)
    rparams = list(ref.parameters())
    oref = MasterLARS(rparams, **HP)
    layouts, state_ok, trust_ok, same = [list(ddp.param_layout())], [], [], []
    for x, y in _batches(3):
        opt.zero_grad()
        oref.zero_grad()
        F.cross_entropy(ddp(x), y).backward()
        F.cross_entropy(ref(x), y).backward()
        opt.step()
        oref.step()
        layouts.append(list(ddp.param_layout()))
        want_t = dict(zip(range(len(rparams)), _trusts(oref, rparams)))
        got_t = _trusts(opt, list(ddp._params))
        ok, tk, sm = True, True, True
        rmom = oref._groups[0]["momentum"]
        for i, (p, q, (g, off)) in enumerate(zip(ddp._params, rparams, ddp.param_layout())):
            st, n = opt._flat_state[g], p.numel()
            ok &= torch.allclose(st["momentum"].narrow(0, off, n), rmom.narrow(0, oref._groups[0]["offs"][i], n),
                                 atol=1e-7, rtol=1e-5)
            sm &= torch.allclose(st["param"].narrow(0, off, n), q.detach().flatten(), atol=1e-6, rtol=1e-5)
            tk &= math.isclose(got_t[i], want_t[i], rel_tol=1e-5)
            tk &= (got_t[i] == 1.0) == (p.dim() <= 1)
        state_ok.append(ok)
        trust_ok.append(tk)
        same.append(sm)
    sd = opt.state_dict()
    foreign = []
    for o, state in ((FlatSGD(ddp, lr=0.1, momentum=0.9), sd),
                     (opt, FlatSGD(ddp, lr=0.1, momentum=0.9).state_dict())):
        try:
            o.load_state_dict(state)
            foreign.append(False)
        except ForeignOptimizerState:
            foreign.append(True)
    return {"foreign": foreign, "layouts": layouts, "state_ok": state_ok, "trust_ok": trust_ok, "same": same,
            "kind": sd["kind"], "steps": sd["steps"], "has_layout": "layout" in sd,
            "range": opt.last_trust_range()}


def test_flat_lars_state_and_trust_follow_bucket_rebuild():
    res = run_world(_flat_worker, 1)[0]
    assert res["layouts"][0] != res["layouts"][-1], "test must exercise a layout change"
    assert res["state_ok"] == [True] * 3
    assert res["trust_ok"] == [True] * 3
    assert res["same"] == [True] * 3  # FlatLARS == MasterLARS on the same model
    assert res["kind"] == "lars" and res["steps"] == 3 and res["has_layout"]
    lo, hi = res["range"]
    assert 0 < lo < hi
    assert res["foreign"] == [True, True]  # FlatSGD <- lars state, FlatLARS <- sgd state


# --------------------------------------------------------------------------- #
def test_build_optimizer_and_step_config():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    o = build_optimizer("lars", _mlp().parameters(), False, lr=0.3, momentum=0.8, weight_decay=5e-5, eps=1e-9,
                        trust_coefficient=0.002)
    assert isinstance(o, MasterLARS)
    g = o.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["eps"], g["trust_coefficient"]) == \
        (0.3, 0.8, 5e-5, 1e-9, 0.002)
    with pytest.raises(ValueError, match="adamw"):
        build_optimizer("lars", _mlp().parameters(), False, lr=0.3, clip_grad_norm=1.0)
    with pytest.raises(ValueError, match=r"sgd \| adamw \| lars"):
        build_optimizer("lamb", _mlp().parameters(), False, lr=0.3)
    assert StepConfig().trust_coefficient == 1e-3
    cfg = StepConfig(model="vit_tiny", optimizer="lars", trust_coefficient=0.01, parallel="none",
                     dtype=torch.float32, batch_size=8, lr=0.5, weight_decay=5e-5, channels_last=False)
    st = build_train_state(cfg, torch.device("cpu"))
    assert isinstance(st.optimizer, MasterLARS)
    assert st.optimizer.param_groups[0]["trust_coefficient"] == 0.01
    losses = [float(st.step().detach()) for _ in range(3)]
    assert all(math.isfinite(v) for v in losses), losses
    lo, hi = st.optimizer.last_trust_range()
    assert 0 < lo <= hi and math.isfinite(hi)


def test_cli_flags_and_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args(["--optimizer", "lars", "--trust-coefficient", "0.002"])
    check_args(p, a)
    assert a.optimizer == "lars" and a.trust_coefficient == 0.002
    a = p.parse_args(["--optimizer", "lars", "--parallel", "pipe", "--world-size", "4"])
    check_args(p, a)  # per-tensor norms: a multi-stage pipeline may use LARS
    assert a.trust_coefficient == 1e-3
    for argv, msg in ((["--trust-coefficient", "0.002"], "--optimizer lars"),
                      (["--optimizer", "adamw", "--trust-coefficient", "0.002"], "--optimizer lars"),
                      (["--optimizer", "lars", "--clip-grad-norm", "1.0"], "--optimizer adamw"),
                      (["--optimizer", "lars", "--trust-coefficient", "0"], "positive")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_cli_trains_with_lars_and_logs_the_trust_range(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29000 + os.getpid() % 1000), PYTHONPATH=ROOT)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "ddp",
                        "--arch", "mobilenetv2", "--synthetic", "-b", "8", "--epochs", "2", "--steps-per-epoch", "2",
                        "--optimizer", "lars", "--lr", "0.5", "--wd", "5e-5", "--warmup-epochs", "1",
                        "--log-dir", str(tmp_path / "log"), "-j", "0", "--checkpoint", str(tmp_path / "ck.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "log" / "ddp_8.txt").read_text().strip().splitlines()
    assert len(lines) == 2
    for ln in lines:
        rec = dict(f.split(":", 1) for f in ln.split("  "))
        assert math.isfinite(float(rec["loss_train"])), ln
        assert 0 < float(rec["trust_min"]) <= float(rec["trust_max"]) < float("inf"), ln
