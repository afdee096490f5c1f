"""The weight EMA of the flat optimizers (ops/optim.py ``ema_decay``) on the
CPU path: the recurrence against float64 over the optimizer's own fp32
masters, that it is a pure side output, the sub-ulp case a bf16 average cannot
follow, warm-up, checkpoints and state loading in every on/off combination,
the DDP bucket rebuild, ``ema_weights()``, the trainer's flags and
checkpoints, and the compile-time resources of the step kernels' EMA
instantiations.

Tolerance of the recurrence: atol = rtol = 5e-6.  One ``fmaf`` and one
subtraction per step, at most 1.5 ulp of ``|e| < 5``: 7.2e-7 per step, 2.9e-6
over 4 steps before the decay contracts it (the 6-step CPU cases stay inside:
at d = 0.9 the errors of earlier steps are contracted by 0.9 per step)."""
import json
import math
import os
import shutil
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dist_utils import run_world
from distributed_model_parallel_amd.ops.optim import (FlatAdamW, MasterAdamW, MasterLARS, MasterSGD,
                                                      _ema_reference, build_optimizer)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-6
BF16, F32 = torch.bfloat16, torch.float32
KINDS = {"sgd": (MasterSGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4)),
         "adamw": (MasterAdamW, dict(lr=1e-2, weight_decay=0.1, max_grad_norm=0.5)),
         "lars": (MasterLARS, dict(lr=0.5, momentum=0.9, weight_decay=1e-4))}


def _params(seed=0):
    """An fp32 group (2-D and 1-D) and a bf16 group; sizes that need slot padding."""
    g = torch.Generator().manual_seed(seed)
    shapes = [((5, 7), F32), ((9,), F32), ((6, 11), BF16), ((13,), BF16)]
    return [nn.Parameter(torch.randn(s, generator=g).to(dt)) for s, dt in shapes]


def _grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g).to(p.dtype) for p in params]


def masters_of(opt):
    """Per parameter (``param_groups`` order) the fp32 weights the optimizer holds: master, or fp32 parameter."""
    views = {}
    for gi, st in enumerate(opt._current_groups()):
        src = st.get("master", st["param"])
        for p, off in opt._slots(gi):
            views[id(p)] = src.as_strided(p.shape, p.stride(), off)
    return [views[id(p)] for grp in opt.param_groups for p in grp["params"]]


class Recurrence:
    """float64 ``e += (1 - d) (w - e)`` over the optimizer's own masters."""

    def __init__(self, opt):
        self.opt = opt
        self.e = [m.detach().double().clone() for m in masters_of(opt)]

    def update(self, d):
        for e, m in zip(self.e, masters_of(self.opt)):
            e += (1.0 - d) * (m.detach().double() - e)

    def check(self, msg=""):
        for i, (e, got) in enumerate(zip(self.e, self.opt.ema_tensors())):
            assert got.dtype == F32
            torch.testing.assert_close(got.double().cpu(), e.cpu(), atol=TOL, rtol=TOL, msg=lambda s: f"{msg} param {i}: {s}")


def _state_flats(opt):
    out = []
    for st in opt._state_groups():
        out += [st[k] for k in sorted(st) if k in opt.STATE_KEYS + ("master", "param")]
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ema_follows_the_recurrence_and_is_a_pure_side_output(kind):
    cls, kw = KINDS[kind]
    pa, pb = _params(), _params()
    oa, ob = cls(pa, ema_decay=0.9, **kw), cls(pb, **kw)
    assert oa.ema_enabled and not ob.ema_enabled
    rec = Recurrence(oa)
    rec.check("start")  # the EMA starts at the weights
    for t in range(6):
        for p, q, g in zip(pa, pb, _grads(pa, 10 + t)):
            p.grad.copy_(g)
            q.grad.copy_(g)
        oa.step()
        ob.step()
        rec.update(0.9)
        rec.check(f"step {t}")
    assert oa.state_dict()["ema_updates"] == 6
    for a, b in zip(_state_flats(oa), _state_flats(ob)):
        assert torch.equal(a, b)
    for st in oa._state_groups():  # zero-padded slot tails stay exactly 0
        used = torch.zeros(st["ema"].numel(), dtype=torch.bool)
        for p, off in zip(st["params"], st["offs"]):
            used[off:off + p.numel()] = True
        assert (~used).any() and torch.all(st["ema"][~used] == 0)


def test_sub_ulp_updates_move_the_fp32_ema_of_the_masters():
    """bf16 parameters at 0.25 (bf16 spacing below it: 2^-10 ~ 9.8e-4), SGD steps
    of 2e-4 each -- less than one bf16 ulp -- and decay 0.9999: the increment
    of the average, 1e-4 * (w - e) <= 1e-6, is far below a bf16 ulp, so a bf16
    average never moves; the fp32 EMA of the fp32 masters follows the float64
    recurrence.  Bound: half an fp32 ulp of 0.25 (7.5e-9) per step, 3.7e-7 over
    50 steps, against a movement of ~2.5e-5."""
    p = nn.Parameter(torch.full((64,), 0.25, dtype=BF16))
    opt = MasterSGD([p], lr=0.1, ema_decay=0.9999)
    rec = Recurrence(opt)
    start = opt.ema_tensors()[0].clone()
    bf16_avg = start.to(BF16)
    for _ in range(50):
        p.grad.fill_(2e-3)
        before = masters_of(opt)[0].clone()
        opt.step()
        assert float((masters_of(opt)[0] - before).abs().max()) < 2 ** -10
        rec.update(0.9999)
        bf16_avg.lerp_(p.detach(), 1e-4)  # the usual deep-copied model's update
    ema = opt.ema_tensors()[0]
    assert ema.dtype == F32
    assert torch.equal(bf16_avg, start.to(BF16))  # a bf16 average does not move
    want = rec.e[0] - start.double()
    assert float(want.abs().min()) > 2e-5
    moved = ema.double() - start.double()
    torch.testing.assert_close(moved, want, atol=5e-7, rtol=0)


def test_warmup_decays():
    opt = MasterSGD(_params(), lr=0.1, ema_decay=0.9999, ema_warmup=True)
    assert opt.ema_decay_of_update(0) == pytest.approx(0.1, abs=1e-15)
    assert opt.ema_decay_of_update(1) == pytest.approx(2 / 11, abs=1e-15)
    assert opt.ema_decay_of_update(10) == pytest.approx(11 / 20, abs=1e-15)
    assert opt.ema_decay_of_update(1000) == pytest.approx(min(0.9999, 1001 / 1010), abs=1e-15)
    low = MasterSGD(_params(), lr=0.1, ema_decay=0.5, ema_warmup=True)
    assert low.ema_decay_of_update(1000) == 0.5
    assert MasterSGD(_params(), lr=0.1, ema_decay=0.9).ema_decay_of_update(0) == 0.9
    # and step() uses them
    params = _params()
    opt = MasterSGD(params, lr=0.1, ema_decay=0.9999, ema_warmup=True)
    rec = Recurrence(opt)
    for t in range(3):
        for p, g in zip(params, _grads(params, t)):
            p.grad.copy_(g)
        opt.step()
        rec.update((1 + t) / (10 + t))
        rec.check(f"step {t}")
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            MasterSGD(_params(), lr=0.1, ema_decay=bad)


class _MLP(nn.Module):
    """Registration order (head first) differs from the autograd-ready order,
    so a DDP bucket rebuild really changes the flat layout."""

    def __init__(self):
        super().__init__()
        self.head = nn.Linear(32, 5)
        self.body = nn.Sequential(nn.Linear(12, 32), nn.LayerNorm(32), nn.ReLU(), nn.Linear(32, 32))

    def forward(self, x):
        return self.head(F.relu(self.body(x)))


def _mlp(dtype=F32):
    torch.manual_seed(0)
    return _MLP().to(dtype)


def _batches(n, dtype=F32):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(8, 12, generator=g).to(dtype), torch.randint(0, 5, (8,), generator=g)) for _ in range(n)]


def _run(m, o, batches):
    for x, y in batches:
        o.zero_grad()
        F.cross_entropy(m(x).float(), y).backward()
        o.step()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_checkpoint_roundtrip_continues_bit_identically(tmp_path, dtype):
    from distributed_model_parallel_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    data = _batches(5, dtype)
    a = _mlp(dtype)
    oa = MasterAdamW(a.parameters(), lr=1e-2, weight_decay=0.1, ema_decay=0.9, ema_warmup=True)
    _run(a, oa, data[:3])
    path = save_checkpoint(str(tmp_path / "ck.pth"), a, oa, epoch=1)
    live = [p.detach().clone() for p in a.parameters()]
    sd = oa.state_dict()
    assert sd["ema_updates"] == 3 and all("ema" in s for s in sd["flat_state"])
    for p, l in zip(a.parameters(), live):  # writing net_ema left the live weights alone
        assert torch.equal(p.detach(), l)
    _run(a, oa, data[3:])
    b = _mlp(dtype)
    with torch.no_grad():
        for p in b.parameters():
            p.add_(1.0)
    ob = MasterAdamW(b.parameters(), lr=1e-2, weight_decay=0.1, ema_decay=0.9, ema_warmup=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the state has an EMA: nothing to warn about
        load_checkpoint(path, b, ob, restore_rng=False)
    assert ob.state_dict()["ema_updates"] == 3
    _run(b, ob, data[3:])
    assert ob.state_dict()["ema_updates"] == 5
    for ea, eb in zip(oa.ema_tensors(), ob.ema_tensors()):
        assert torch.equal(ea, eb)
    for ma, mb in zip(masters_of(oa), masters_of(ob)):
        assert torch.equal(ma, mb)
    # net_ema: the averaged weights at the time of the save, same keys as net
    ck = torch.load(path, weights_only=True)
    assert list(ck["net_ema"]) == list(ck["net"])
    assert any(not torch.equal(ck["net_ema"][k], ck["net"][k]) for k in ck["net"])


def test_state_without_ema_loaded_with_ema_on_seeds_it_and_warns_once():
    a = _mlp(BF16)
    oa = MasterAdamW(a.parameters(), lr=1e-2)
    _run(a, oa, _batches(2, BF16))
    b = _mlp(BF16)
    ob = MasterAdamW(b.parameters(), lr=1e-2, ema_decay=0.99)
    _run(b, ob, _batches(1, BF16))  # the EMA and its count have moved
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ob.load_state_dict(oa.state_dict())
    assert len([x for x in w if "EMA" in str(x.message)]) == 1
    assert ob.state_dict()["ema_updates"] == 0 and ob.state_dict()["steps"] == 2
    for e, m, ma in zip(ob.ema_tensors(), masters_of(ob), masters_of(oa)):
        assert torch.equal(m, ma) and torch.equal(e, m)


def test_state_with_ema_loaded_with_ema_off_ignores_it():
    a = _mlp()
    oa = MasterSGD(a.parameters(), lr=0.1, momentum=0.9, ema_decay=0.9)
    _run(a, oa, _batches(2))
    b = _mlp()
    ob = MasterSGD(b.parameters(), lr=0.1, momentum=0.9)
    ob.load_state_dict(oa.state_dict())
    sd = ob.state_dict()
    assert "ema_updates" not in sd and all("ema" not in s for s in sd["flat_state"])
    assert all("ema" not in st for st in ob._state_groups())
    assert torch.equal(ob._groups[0]["momentum"], oa._groups[0]["momentum"])
    with pytest.raises(RuntimeError, match="ema_decay"):
        ob.ema_tensors()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with ob.ema_weights():
            pass


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_state_dict_without_ema_keeps_the_old_format(kind):
    cls, kw = KINDS[kind]
    for decay in (None, 0, 0.0):
        opt = cls(_params(), ema_decay=decay, **kw)
        assert not opt.ema_enabled
        sd = opt.state_dict()
        want = {"steps", "param_groups", "numels", "flat_state"} | ({"kind"} if kind != "sgd" else set())
        assert set(sd) == want
        for s in sd["flat_state"]:
            assert set(s) <= set(cls.STATE_KEYS) | {"master"}


def test_sync_from_params_reseeds_the_ema():
    params = _params()
    opt = MasterSGD(params, lr=0.1, ema_decay=0.9)
    for t in range(2):
        for p, g in zip(params, _grads(params, t)):
            p.grad.copy_(g)
        opt.step()
    with torch.no_grad():
        for p in params:
            p.copy_(torch.full_like(p, 0.5))  # weights replaced under the optimizer
    opt.sync_from_params()
    assert opt.state_dict()["ema_updates"] == 0
    for e, m in zip(opt.ema_tensors(), masters_of(opt)):
        assert torch.all(m == 0.5) and torch.equal(e, m)


# --------------------------------------------------------------------------- #
def _flat_worker(rank, world):
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    torch.manual_seed(0)
    m = _MLP()
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.002, first_bucket_mb=0.0005, flat_parameters=True)
    opt = FlatAdamW(ddp, lr=1e-2, weight_decay=0.1, ema_decay=0.9)
    rec = Recurrence(opt)
    layouts, errs = [list(ddp.param_layout())], []
    for x, y in _batches(3):
        opt.zero_grad()
        F.cross_entropy(ddp(x), y).backward()
        opt.step()
        layouts.append(list(ddp.param_layout()))
        rec.update(0.9)
        # per parameter, wherever the current layout put it
        err = 0.0
        for p, e, (g, off) in zip(ddp._params, rec.e, ddp.param_layout()):
            got = opt._flat_state[g]["ema"].narrow(0, off, p.numel()).double()
            err = max(err, float(((got - e.flatten()).abs() / (1 + e.flatten().abs())).max()))
        errs.append(err)
    sd = opt.state_dict()
    return {"layouts": layouts, "errs": errs, "ema_updates": sd["ema_updates"],
            "saved": ["ema" in s for s in sd["flat_state"]]}


def test_flat_adamw_ema_follows_bucket_rebuild():
    res = run_world(_flat_worker, 1)[0]
    assert res["layouts"][0] != res["layouts"][-1], "test must exercise a layout change"
    assert max(res["errs"]) <= TOL, res["errs"]
    assert res["ema_updates"] == 3 and all(res["saved"])


# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ema_weights_swaps_in_and_out_bitwise(kind):
    cls, kw = KINDS[kind]
    params = _params()
    opt = cls(params, ema_decay=0.9, **kw)
    for t in range(3):
        for p, g in zip(params, _grads(params, t)):
            p.grad.copy_(g)
        opt.step()
    live = [p.detach().clone() for p in params]
    ema = [e.clone() for e in opt.ema_tensors()]
    masters = [m.clone() for m in masters_of(opt)]
    with opt.ema_weights():
        for p, e, l in zip(params, ema, live):
            assert torch.equal(p.detach(), e.to(p.dtype))
            assert not torch.equal(p.detach(), l)
        with pytest.raises(RuntimeError, match="already entered"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            opt.step()
    for p, l, m in zip(params, live, masters):
        assert torch.equal(p.detach(), l) and torch.equal(p.detach(), m.to(p.dtype))
    for e, e0 in zip(opt.ema_tensors(), ema):
        assert torch.equal(e, e0)
    assert opt.state_dict()["ema_updates"] == 3
    try:  # an exception inside still swaps back
        with opt.ema_weights():
            raise KeyError("x")
    except KeyError:
        pass
    for p, l in zip(params, live):
        assert torch.equal(p.detach(), l)
    with opt.ema_weights():  # and the context can be entered again
        pass


def test_ema_reference_is_an_fp32_lerp():
    e, w = torch.tensor([1.0, -2.0]), torch.tensor([3.0, 2.0])
    _ema_reference(e, w, 0.25)
    assert torch.equal(e, torch.tensor([1.5, -1.0]))
    e = torch.tensor([1.0])
    _ema_reference(e, torch.tensor([3.0], dtype=BF16), 0.5)
    assert e.dtype == F32 and float(e) == 2.0


def test_build_optimizer_and_step_config_build_the_ema():
    from distributed_model_parallel_amd import _native
    from distributed_model_parallel_amd.ops import optim
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    assert "fuse_ema" in _native.FEATURES
    assert optim.fused_ema() is True
    optim.set_fused_ema(False)
    try:
        assert optim.fused_ema() is False
    finally:
        optim.set_fused_ema(True)
    for kind in ("sgd", "adamw", "lars"):
        on = build_optimizer(kind, _params(), flat=False, lr=0.1, ema_decay=0.99, ema_warmup=True)
        assert on.ema_enabled and on.ema_decay == 0.99 and on.ema_warmup
        assert not build_optimizer(kind, _params(), flat=False, lr=0.1).ema_enabled
    cfg = StepConfig(model="vit_tiny", optimizer="adamw", parallel="none", dtype=F32, batch_size=4, lr=1e-3,
                     channels_last=False, ema_decay=0.9)
    st = build_train_state(cfg, torch.device("cpu"))
    assert isinstance(st.optimizer, MasterAdamW) and st.optimizer.ema_enabled
    rec = Recurrence(st.optimizer)
    for _ in range(2):
        st.step()
        rec.update(0.9)
    rec.check()
    assert StepConfig().ema_decay == 0.0
    off = build_train_state(StepConfig(model="vit_tiny", parallel="none", dtype=F32, batch_size=4,
                                       channels_last=False), torch.device("cpu"))
    assert not off.optimizer.ema_enabled


def test_cli_flags_and_parser_errors(tmp_path, capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert (a.model_ema_decay, a.model_ema_warmup, a.init_from_ema) == (0.0, False, False)
    ck = tmp_path / "a.pth"
    ck.write_bytes(b"")
    a = p.parse_args(["--model-ema-decay", "0.9999", "--model-ema-warmup", "--init-from", str(ck), "--init-from-ema"])
    check_args(p, a)
    assert (a.model_ema_decay, a.model_ema_warmup, a.init_from_ema) == (0.9999, True, True)
    for argv, msg in ((["--model-ema-decay", "1.0"], "[0, 1)"),
                      (["--model-ema-decay", "-0.5"], "[0, 1)"),
                      (["--init-from-ema"], "needs --init-from"),
                      (["--model-ema-warmup"], "needs --model-ema-decay"),
                      (["--model-ema-decay", "0.99", "--parallel", "pipe"], "--parallel pipe")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_cli_evaluates_and_saves_the_ema(tmp_path):
    from distributed_model_parallel_amd.models import build_model
    from distributed_model_parallel_amd.utils.checkpoint import load_weights, save_checkpoint
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(33000 + os.getpid() % 1000), PYTHONPATH=ROOT)
    env.pop("RANK", None)
    ckpt = str(tmp_path / "ck.pth")
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "none",
                        "--arch", "vit_tiny", "--synthetic", "-b", "32", "--epochs", "2", "--steps-per-epoch", "3",
                        "--optimizer", "adamw", "--lr", "1e-3", "--wd", "0.05", "--warmup-epochs", "0",
                        "--dtype", "fp32", "--model-ema-decay", "0.9", "-j", "0",
                        "--log-dir", str(tmp_path / "log"), "--checkpoint", ckpt],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(ln) for ln in (tmp_path / "log" / "none_vit_tiny.rank0.jsonl").read_text().splitlines()]
    assert len(recs) == 2
    for rec in recs:
        assert math.isfinite(rec["loss_val_ema"]) and 0.0 <= rec["acc1_val_ema"] <= 100.0
        assert rec["ema_decay"] == 0.9 and "acc1_val" in rec
    lines = (tmp_path / "log" / "none_32.txt").read_text().strip().splitlines()
    assert all("acc1_val_ema:" in ln and "ema_decay:0.9" in ln for ln in lines)
    ck = torch.load(ckpt, weights_only=True)
    assert list(ck["net_ema"]) == list(ck["net"]) and "acc_ema" in ck["extra"]
    assert any(not torch.equal(ck["net_ema"][k], ck["net"][k]) for k in ck["net"])
    assert all("ema" in s for s in ck["optimizer"]["flat_state"]) and ck["optimizer"]["ema_updates"] > 0
    fresh = build_model("vit_tiny", num_classes=10)
    assert not load_weights(ckpt, fresh, ema=True)["pos_embedding_resized"]
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, ck["net_ema"][k]), k
    live = build_model("vit_tiny", num_classes=10)
    load_weights(ckpt, live)
    for k, v in live.state_dict().items():
        assert torch.equal(v, ck["net"][k]), k
    # the position-embedding resize applies to the averaged weights too
    big = build_model("vit_tiny", num_classes=10, image_size=48)
    assert load_weights(ckpt, big, ema=True)["pos_embedding_resized"]
    plain = str(tmp_path / "plain.pth")
    save_checkpoint(plain, build_model("vit_tiny", num_classes=10))
    with pytest.raises(KeyError, match="net_ema"):
        load_weights(plain, fresh, ema=True)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
@pytest.mark.parametrize("src,kernel", [("fused_sgd.hip", "sgd_flat_kernel"), ("fused_adamw.hip", "adamw_flat_kernel"),
                                        ("fused_lars.hip", "lars_flat_kernel")])
def test_step_kernel_instantiations_build_without_scratch(src, kernel):
    """4 dtype combinations x master or not is 4 (a bf16 parameter always has a
    master, an fp32 one never), each with and without the EMA: 8 per kernel."""
    from tools.kernel_resources import resources
    ks = [k for k in resources(os.path.join(ROOT, "csrc/optim", src)) if kernel in k["name"]]
    assert len(ks) == 16, [k["name"] for k in ks]  # (G, P) x MASTER x EMA: the host instantiates all
    for k in ks:
        assert k["scratch"] == "0", k
