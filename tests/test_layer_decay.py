"""Layer-wise lr decay on the CPU path: the layer-id tables of ViT / ConvNeXt,
``MasterAdamW`` / ``FlatAdamW`` with per-parameter lr scales against
``torch.optim.AdamW`` with one param group per tensor, frozen (scale 0) and
unit-scale tensors, in-place ``set_lr_scales``, the class bytes across a DDP
bucket rebuild, checkpoint round trip, ``load_weights(reset_head=True)``, the
trainer's ``--layer-decay`` / ``--reset-head`` flags and a fine-tuning run.

Bounds of the optimizer comparisons: atol = 1e-6, rtol = 1e-5, those of
``tests/test_adamw.py::test_master_adamw_matches_torch_adamw_fp32`` (the same
fp32 arithmetic against the same oracle; a scale only shrinks the step)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dist_utils import run_world
from distributed_model_parallel_amd.models import build_model, classifier_name, layer_decay_scales, layer_ids
from distributed_model_parallel_amd.ops.optim import FlatAdamW, MasterAdamW, _adamw_reference, build_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD = 1e-2, 0.1


# --------------------------------------------------------------------------- #
# layer ids
# --------------------------------------------------------------------------- #
def _meta(name):
    with torch.device("meta"):
        return build_model(name)


def _forward_rank(name: str) -> tuple:
    """Sort key that puts a ConvNeXt's parameters into forward order (the
    registration order lists all down-sampling layers before the stages)."""
    p = name.split(".")
    if p[0] in ("stem", "stem_norm"):
        return (0, 0, 0)
    if p[0] == "stages":
        return (1 + int(p[1]), 1, int(p[2]))
    if p[0] in ("down_norms", "downs"):
        return (2 + int(p[1]), 0, 0)
    if p[0] in ("norm", "head"):
        return (9, 0, 0)
    return (0, 0, 0)  # a ViT: registration order is forward order already


@pytest.mark.parametrize("name", ["vit_tiny", "convnext_test", "convnext_tiny"])
def test_layer_ids_cover_every_parameter_and_follow_the_forward_order(name):
    m = _meta(name)
    ids, n = layer_ids(m)
    names = [k for k, _p in m.named_parameters()]
    assert set(ids) == set(names)
    assert all(0 <= i < n for i in ids.values())
    order = sorted(names, key=_forward_rank) if name.startswith("convnext") else names
    seq = [ids[k] for k in order]
    assert seq == sorted(seq), "ids never decrease in forward order"
    assert seq[0] == 0 and seq[-1] == n - 1
    scales = layer_decay_scales(m, 0.75)
    by_name = dict(m.named_parameters())
    assert len(scales) == len(names)
    for k in names:
        assert scales[by_name[k]] == 0.75 ** (n - 1 - ids[k]), k
    head = classifier_name(m)
    for k in names:
        if k.startswith(head + "."):
            assert scales[by_name[k]] == 1.0, k
    assert all(v == 1.0 for v in layer_decay_scales(m, 1.0).values())


def test_layer_id_spot_names():
    vit = _meta("vit_tiny")
    L = len(vit.blocks)
    ids, n = layer_ids(vit)
    assert n == L + 2
    assert ids["cls_token"] == ids["pos_embedding"] == 0
    assert all(v == 0 for k, v in ids.items() if k.startswith("patch_embed."))
    assert ids["blocks.0.ln1.weight"] == 1 and ids[f"blocks.{L - 1}.mlp.fc2.bias"] == L
    assert ids["ln.weight"] == ids["head.weight"] == ids["head.bias"] == L + 1
    for name, d2 in (("convnext_test", 2), ("convnext_tiny", 9)):
        ids, n = layer_ids(_meta(name))
        assert n == 14
        assert ids["stem_norm.weight"] == 0 and all(v == 0 for k, v in ids.items() if k.startswith("stem."))
        assert ids["stages.0.0.gamma"] == 1
        assert ids["down_norms.0.weight"] == ids["stages.1.0.fc1.weight"] == 2
        assert all(v == 2 for k, v in ids.items() if k.startswith("downs.0."))
        assert ids["down_norms.1.bias"] == 3 and all(v == 3 for k, v in ids.items() if k.startswith("downs.1."))
        for b in range(d2):
            assert ids[f"stages.2.{b}.fc2.weight"] == 3 + (9 * b) // d2
        assert ids["down_norms.2.weight"] == ids["stages.3.0.gamma"] == 12
        assert all(v == 12 for k, v in ids.items() if k.startswith("downs.2."))
        assert ids["norm.weight"] == ids["head.bias"] == 13
    small, _n = layer_ids(_meta("convnext_small"))  # 27 blocks: three per id
    assert [small[f"stages.2.{b}.gamma"] for b in (0, 2, 3, 26)] == [3, 3, 4, 11]


def test_layer_ids_reject_other_models_and_unknown_parameters():
    with pytest.raises(ValueError, match="VisionTransformer.*ConvNeXt"):
        layer_ids(_meta("resnet50"))
    with pytest.raises(ValueError, match="VisionTransformer.*ConvNeXt"):
        layer_decay_scales(_meta("resnet50"), 0.75)
    vit = _meta("vit_tiny")
    vit.register_parameter("extra_token", nn.Parameter(torch.zeros(1, device="meta")))
    with pytest.raises(ValueError, match="extra_token"):
        layer_ids(vit)
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        layer_decay_scales(_meta("vit_tiny"), 0.0)
    assert classifier_name(_meta("resnet50")) == "fc" and classifier_name(_meta("mobilenetv2")) == "linear"
    assert classifier_name(_meta("convnext_test")) == "head"


# --------------------------------------------------------------------------- #
# optimizer
# --------------------------------------------------------------------------- #
class _Toy(nn.Module):
    """Three "blocks"; the head is registered first so a DDP bucket rebuild
    really changes the flat layout (as tests/test_adamw.py's model)."""

    def __init__(self):
        super().__init__()
        self.head = nn.Linear(32, 5)
        self.b0 = nn.Linear(12, 32)
        self.b1 = nn.Sequential(nn.LayerNorm(32), nn.Linear(32, 32))

    def forward(self, x):
        return self.head(F.relu(self.b1(F.relu(self.b0(x)))))


def _toy(dtype=torch.float32):
    torch.manual_seed(0)
    return _Toy().to(dtype)


def _toy_scales(m, s0=0.0, s1=0.5, s2=1.0):
    out = {p: s0 for p in m.b0.parameters()}
    out.update({p: s1 for p in m.b1.parameters()})
    out.update({p: s2 for p in m.head.parameters()})
    return out


def _grouped_adamw(params, scales):
    """The oracle: torch.optim.AdamW, one param group per tensor, lr = lr * s."""
    return torch.optim.AdamW([{"params": [r], "lr": LR * s, "weight_decay": WD if r.dim() > 1 else 0.0}
                              for r, s in zip(params, scales)], lr=LR)


def _batches(n, dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(8, 12, generator=g).to(dtype), torch.randint(0, 5, (8,), generator=g)) for _ in range(n)]


def _masters(opt, params):
    out = {}
    for st in opt._groups:
        src = st.get("master", st["param"])
        for p, off in zip(st["params"], st["offs"]):
            out[id(p)] = src.as_strided(p.shape, p.stride(), off).float()
    return [out[id(p)] for p in params]


@pytest.mark.parametrize("max_norm", [None, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_master_adamw_with_scales_matches_adamw_with_one_group_per_tensor(dtype, max_norm):
    m = _toy(dtype)
    params = list(m.parameters())
    scales = _toy_scales(m)
    ref = [p.detach().float().clone().requires_grad_() for p in params]
    oref = _grouped_adamw(ref, [scales[p] for p in params])
    opt = MasterAdamW(params, lr=LR, weight_decay=WD, max_grad_norm=max_norm, lr_scales=scales)
    assert opt.lr_scaled and opt.lr_scale_range() == (0.0, 1.0)
    norms = []
    for x, y in _batches(5, dtype):
        opt.zero_grad()
        F.cross_entropy(m(x).float(), y).backward()
        for p, r in zip(params, ref):  # the oracle takes the same gradients, upcast
            r.grad = p.grad.detach().float().clone()
        if max_norm:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ref, max_norm)))
        oref.step()
        opt.step()
    if max_norm:
        assert max(norms) > max_norm, "the test must exercise a clipped step"
    worst = 0.0
    for got, r in zip(_masters(opt, params), ref):
        worst = max(worst, float((got - r.detach()).abs().max()))
        torch.testing.assert_close(got, r.detach(), atol=1e-6, rtol=1e-5)
    print(f"max abs err vs grouped AdamW ({dtype}, clip {max_norm}): {worst:.3g} (bound 1e-6 + 1e-5 |w|)")
    if dtype == torch.bfloat16:
        for p, got in zip(params, _masters(opt, params)):
            assert torch.equal(p.detach(), got.bfloat16())


def _run(opt, m, n, dtype=torch.float32):
    for x, y in _batches(n, dtype):
        opt.zero_grad()
        F.cross_entropy(m(x).float(), y).backward()
        opt.step()


def test_all_scales_one_is_bit_identical_to_no_scales_with_ema():
    a, b = _toy(), _toy()
    oa = MasterAdamW(a.parameters(), lr=LR, weight_decay=WD, ema_decay=0.9)
    ob = MasterAdamW(b.parameters(), lr=LR, weight_decay=WD, ema_decay=0.9, lr_scales={p: 1.0 for p in b.parameters()})
    assert not ob.lr_scaled and ob.lr_scale_range() == (1.0, 1.0)
    _run(oa, a, 3)
    _run(ob, b, 3)
    assert ob._lr_key is None, "all-ones scales take the unscaled step: no class bytes are built"
    for key in ("param", "exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(oa._groups[0][key], ob._groups[0][key]), key


def test_reference_unit_scale_vectors_get_the_unscaled_bits_and_zero_freezes():
    """The per-vector rule of _adamw_reference: scale 1 -> the bits of the
    unscaled call; scale 0 -> weights untouched (a -0.0 stays -0.0), moments move."""
    n = 8 * 6
    g = torch.Generator().manual_seed(5)
    w0 = torch.randn(n, generator=g)
    w0[8] = -0.0
    mask = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.uint8)
    scale = torch.tensor([1.0, 0.0, 0.5, 1.0, 0.0, 0.25])
    cfg = {"lr": LR, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": WD}
    wa, ma, va = w0.clone(), torch.zeros(n), torch.zeros(n)
    wb, mb, vb = w0.clone(), torch.zeros(n), torch.zeros(n)
    for t in range(1, 4):
        gr = torch.randn(n, generator=g)
        hyper = torch.tensor([1 - 0.9 ** t, 1 - 0.999 ** t, 0.0, 0.7])
        _adamw_reference(None, ma, va, gr, wa, mask, hyper, cfg)
        _adamw_reference(None, mb, vb, gr, wb, mask, hyper, cfg, scale)
    sv = scale.repeat_interleave(8)
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert torch.equal(wa[sv == 1], wb[sv == 1])
    assert torch.equal(wb[sv == 0].view(torch.int32), w0[sv == 0].view(torch.int32))
    assert not torch.equal(wa[sv == 0.5], wb[sv == 0.5]) and bool(mb[sv == 0].abs().min() > 0)


def test_scale_zero_freezes_the_weights_while_the_moments_move():
    m = _toy()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = MasterAdamW(m.parameters(), lr=LR, weight_decay=WD, lr_scales=_toy_scales(m))
    _run(opt, m, 3)
    st = opt._groups[0]
    for p, off in zip(st["params"], st["offs"]):
        moved = not torch.equal(p.detach(), before[[k for k, v in m.named_parameters() if v is p][0]])
        assert moved == (opt.lr_scale_of(p) != 0.0)
        assert bool(st["exp_avg"].narrow(0, off, p.numel()).abs().max() > 0)


def test_set_lr_scales_rewrites_the_device_tensors_in_place():
    m = _toy()
    opt = MasterAdamW(m.parameters(), lr=LR, weight_decay=WD, lr_scales=_toy_scales(m))
    _run(opt, m, 1)
    d = opt._lr_dev[0]
    ptrs = (d["cls"].data_ptr(), d["table"].data_ptr())
    assert d["cls"].dtype == torch.uint8 and d["cls"].numel() == opt._groups[0]["param"].numel() // 8
    assert d["table"].dtype == torch.float32 and d["table"].numel() == 256
    opt.set_lr_scales(_toy_scales(m, 0.25, 0.125, 0.75))
    assert (opt._lr_dev[0]["cls"].data_ptr(), opt._lr_dev[0]["table"].data_ptr()) == ptrs
    assert opt.lr_scale_range() == (0.125, 0.75) and opt.lr_scale_of(m.b0.weight) == 0.25
    st = opt._groups[0]
    for p, off in zip(st["params"], st["offs"]):
        got = d["table"][d["cls"][off // 8:(off + p.numel() + 7) // 8].long()]
        assert bool(torch.all(got == opt.lr_scale_of(p)))
    opt.set_lr_scales(None)  # back to 1.0 everywhere: same storage, the step keeps reading it
    assert (opt._lr_dev[0]["cls"].data_ptr(), opt._lr_dev[0]["table"].data_ptr()) == ptrs
    assert bool(torch.all(d["table"][d["cls"].long()] == 1.0)) and not opt.lr_scaled
    _run(opt, m, 1)


def test_lr_scale_argument_errors():
    m = _toy()
    params = list(m.parameters())
    with pytest.raises(ValueError, match="not one of the optimizer's parameters"):
        MasterAdamW(params, lr=LR, lr_scales={nn.Parameter(torch.zeros(3)): 0.5})
    for bad in (-0.5, float("nan"), float("inf")):
        mm = _toy()
        with pytest.raises(ValueError, match="finite and not negative"):
            MasterAdamW(mm.parameters(), lr=LR, lr_scales={next(mm.parameters()): bad})
    many = [nn.Parameter(torch.zeros(8)) for _ in range(257)]
    with pytest.raises(ValueError, match="distinct lr scales"):
        MasterAdamW(many, lr=LR, lr_scales={p: (i + 1) / 1000 for i, p in enumerate(many)})
    ok = MasterAdamW(many[:256], lr=LR, lr_scales={p: (i + 1) / 1000 for i, p in enumerate(many[:256])})
    assert len(ok._lr_values()) == 256
    opt = MasterAdamW(_toy().parameters(), lr=LR)
    with pytest.raises(ValueError, match="not one of the optimizer's parameters"):
        opt.set_lr_scales({params[0]: 0.5})
    for kind in ("sgd", "lars"):
        mm = _toy()
        with pytest.raises(ValueError, match="adamw"):
            build_optimizer(kind, mm.parameters(), False, lr=0.1, lr_scales={next(mm.parameters()): 0.5})
    mm = _toy()
    o = build_optimizer("adamw", mm.parameters(), False, lr=0.1, lr_scales=_toy_scales(mm))
    assert isinstance(o, MasterAdamW) and o.lr_scale_range() == (0.0, 1.0)


# --------------------------------------------------------------------------- #
def _flat_worker(rank, world):
    from distributed_model_parallel_amd.parallel.distributed import DistributedDataParallel
    torch.manual_seed(0)
    m = _Toy()
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.002, first_bucket_mb=0.0005, flat_parameters=True)
    scales = _toy_scales(m, 0.0, 0.5, 1.0)  # on the bare model's Parameter objects
    opt = FlatAdamW(ddp, lr=LR, weight_decay=WD, lr_scales=scales)
    plist = list(ddp._params)
    ref = [p.detach().clone().requires_grad_() for p in plist]
    oref = _grouped_adamw(ref, [opt.lr_scale_of(p) for p in plist])
    layouts, cls_ok, same = [list(ddp.param_layout())], [], []
    for x, y in _batches(3):
        opt.zero_grad()
        F.cross_entropy(ddp(x), y).backward()
        flats = ddp.flat_groups()
        for p, r, (g, off) in zip(plist, ref, ddp.param_layout()):
            r.grad = flats[g][1].as_strided(p.shape, p.stride(), off).clone()
        opt.step()
        oref.step()
        layouts.append(list(ddp.param_layout()))
        ck, sm = True, True
        for p, r, (g, off) in zip(plist, ref, ddp.param_layout()):
            d = opt._lr_dev[g]
            got = d["table"][d["cls"][off // 8:(off + p.numel() + 7) // 8].long()]
            ck &= bool(torch.all(got == scales[p]))
            sm &= torch.allclose(opt._flat_state[g]["param"].narrow(0, off, p.numel()), r.detach().flatten(),
                                 atol=1e-6, rtol=1e-5)
        cls_ok.append(ck)
        same.append(sm)
    return {"layouts": layouts, "cls_ok": cls_ok, "same": same, "range": opt.lr_scale_range(),
            "keys": sorted(opt.state_dict().keys())}


def test_flat_adamw_class_bytes_follow_bucket_rebuild():
    res = run_world(_flat_worker, 1)[0]
    assert res["layouts"][0] != res["layouts"][-1], "test must exercise a layout change"
    assert res["cls_ok"] == [True] * 3
    assert res["same"] == [True] * 3
    assert res["range"] == (0.0, 1.0)
    assert not any("scale" in k for k in res["keys"]), "the scales are configuration, not state"


def test_checkpoint_roundtrip_continues_bit_identically_with_the_same_scales(tmp_path):
    a = _toy()
    oa = MasterAdamW(a.parameters(), lr=LR, weight_decay=WD, lr_scales=_toy_scales(a, 0.0, 0.5, 0.75))
    data = _batches(4)

    def run(o, m, batches):
        for x, y in batches:
            o.zero_grad()
            F.cross_entropy(m(x), y).backward()
            o.step()

    run(oa, a, data[:2])
    path = str(tmp_path / "ck.pt")
    plain = MasterAdamW(_toy().parameters(), lr=LR, weight_decay=WD)
    assert sorted(oa.state_dict().keys()) == sorted(plain.state_dict().keys())  # the format is unchanged
    torch.save({"net": a.state_dict(), "opt": oa.state_dict()}, path)
    run(oa, a, data[2:])
    b = _toy()
    ob = MasterAdamW(b.parameters(), lr=LR, weight_decay=WD, lr_scales=_toy_scales(b, 0.0, 0.5, 0.75))
    ck = torch.load(path, weights_only=True)
    b.load_state_dict(ck["net"])
    ob.load_state_dict(ck["opt"])
    run(ob, b, data[2:])
    for key in ("param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(oa._groups[0][key], ob._groups[0][key]), key


# --------------------------------------------------------------------------- #
# load_weights(reset_head=True)
# --------------------------------------------------------------------------- #
def test_load_weights_reset_head(tmp_path):
    from distributed_model_parallel_amd.utils.checkpoint import load_weights, save_checkpoint
    torch.manual_seed(0)
    src = build_model("vit_tiny", num_classes=10)
    path = str(tmp_path / "ten.pth")
    save_checkpoint(path, src)
    torch.manual_seed(1)
    five = build_model("vit_tiny", num_classes=5)
    fresh = {k: v.clone() for k, v in five.state_dict().items()}
    with pytest.raises(RuntimeError):
        load_weights(path, five)
    with pytest.raises(RuntimeError):
        load_weights(path, five, reset_head=False)
    out = load_weights(path, five, reset_head=True)
    assert out["head_reset"] is True and out["pos_embedding_resized"] is False
    want = src.state_dict()
    for k, v in five.state_dict().items():
        if k.startswith("head."):
            assert torch.equal(v, fresh[k]), k  # keeps its initialisation
        else:
            assert torch.equal(v, want[k]), k
    torch.manual_seed(2)
    ten = build_model("vit_tiny", num_classes=10)
    out = load_weights(path, ten, reset_head=True)  # an equal-shape head loads even with the flag
    assert out["head_reset"] is False
    assert torch.equal(ten.head.weight, src.head.weight) and torch.equal(ten.head.bias, src.head.bias)
    assert "head_reset" not in load_weights(path, ten)
    # a mismatch outside the classifier still raises
    wide = build_model("convnext_test", num_classes=5)
    with pytest.raises(RuntimeError):
        load_weights(path, wide, reset_head=True)


# --------------------------------------------------------------------------- #
# trainer
# --------------------------------------------------------------------------- #
def test_cli_layer_decay_and_reset_head_flags(tmp_path, capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert a.layer_decay == 1.0 and a.reset_head is False
    ck = tmp_path / "a.pth"
    ck.write_bytes(b"")
    for arch in ("vit_tiny", "vit_b_16", "convnext_tiny"):
        a = p.parse_args(["--arch", arch, "--optimizer", "adamw", "--layer-decay", "0.75"])
        check_args(p, a)
        assert a.layer_decay == 0.75
    check_args(p, p.parse_args(["--arch", "resnet50", "--layer-decay", "1.0"]))  # 1 = off: any arch, any optimizer
    check_args(p, p.parse_args(["--arch", "mobilenetv2", "--parallel", "pipe", "--layer-decay", "1"]))
    a = p.parse_args(["--arch", "vit_tiny", "--init-from", str(ck), "--reset-head"])
    check_args(p, a)
    assert a.reset_head is True
    for argv, msg in ((["--arch", "vit_tiny", "--layer-decay", "0.75"], "--layer-decay needs --optimizer adamw"),
                      (["--arch", "vit_tiny", "--optimizer", "lars", "--layer-decay", "0.75"],
                       "--layer-decay needs --optimizer adamw"),
                      (["--arch", "resnet50", "--optimizer", "adamw", "--layer-decay", "0.75"],
                       "ViT (vit_*) and ConvNeXt (convnext_*)"),
                      (["--arch", "vit_tiny", "--optimizer", "adamw", "--parallel", "pipe", "--layer-decay", "0.75"],
                       "--layer-decay with --parallel pipe is not supported"),
                      (["--arch", "vit_tiny", "--optimizer", "adamw", "--layer-decay", "0"], "must be in (0, 1]"),
                      (["--arch", "vit_tiny", "--optimizer", "adamw", "--layer-decay", "1.5"], "must be in (0, 1]"),
                      (["--arch", "vit_tiny", "--reset-head"], "--reset-head needs --init-from")):
        with pytest.raises(SystemExit):
            check_args(p, p.parse_args(argv))
        assert msg in capsys.readouterr().err, argv


def test_step_config_layer_decay():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    assert StepConfig().layer_decay == 1.0
    cfg = StepConfig(model="vit_tiny", optimizer="adamw", layer_decay=0.75, parallel="none", dtype=torch.float32,
                     batch_size=8, lr=1e-3, weight_decay=0.05, channels_last=False)
    st = build_train_state(cfg, torch.device("cpu"))
    L = len(st.model.blocks)
    assert st.optimizer.lr_scale_range() == (0.75 ** (L + 1), 1.0)
    assert st.optimizer.lr_scale_of(st.model.head.weight) == 1.0
    assert st.optimizer.lr_scale_of(st.model.blocks[0].ln1.weight) == 0.75 ** L
    assert all(math.isfinite(float(st.step().detach())) for _ in range(2))
    off = build_train_state(StepConfig(model="vit_tiny", optimizer="adamw", parallel="none", dtype=torch.float32,
                                       batch_size=8, channels_last=False), torch.device("cpu"))
    assert not off.optimizer.lr_scaled
    for bad in (dict(optimizer="sgd"), dict(optimizer="adamw", model="resnet50", image_size=32),
                dict(optimizer="adamw", parallel="pipe")):
        kw = dict(model="vit_tiny", layer_decay=0.75, parallel="none", dtype=torch.float32, batch_size=8,
                  channels_last=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            build_train_state(StepConfig(**kw), torch.device("cpu"))


def test_cli_fine_tunes_with_layer_decay_from_a_checkpoint_of_another_class_count(tmp_path):
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    from distributed_model_parallel_amd.utils.checkpoint import save_checkpoint
    pre = build_train_state(StepConfig(model="vit_tiny", num_classes=7, optimizer="adamw", parallel="none",
                                       dtype=torch.float32, batch_size=8, lr=1e-3, weight_decay=0.05,
                                       channels_last=False), torch.device("cpu"))
    for _ in range(3):  # a few synthetic steps of "pre-training" on 7 classes
        pre.step()
    init = str(tmp_path / "pre.pth")
    save_checkpoint(init, pre.model, pre.optimizer)
    L = len(pre.model.blocks)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(32000 + os.getpid() % 1000), PYTHONPATH=ROOT)
    env.pop("RANK", None)
    common = [sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--arch", "vit_tiny", "--synthetic",
              "--parallel", "none", "--epochs", "1", "--steps-per-epoch", "2", "--dtype", "fp32", "-b", "8", "-j", "0",
              "--optimizer", "adamw", "--lr", "1e-3", "--wd", "0.05", "--warmup-epochs", "0", "--init-from", init,
              "--log-dir", str(tmp_path / "log"), "--checkpoint", str(tmp_path / "ck.pth")]
    r = subprocess.run(common + ["--layer-decay", "0.75"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "size mismatch" in r.stderr, r.stderr[-2000:]  # 7 classes into 10, no --reset-head
    r = subprocess.run(common + ["--layer-decay", "0.75", "--reset-head"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(ln) for ln in (tmp_path / "log" / "none_vit_tiny.rank0.jsonl").read_text().splitlines()]
    ev = [x for x in recs if x.get("event") == "layer_decay"]
    assert len(ev) == 1, recs
    assert ev[0]["decay"] == 0.75 and ev[0]["distinct_scales"] == L + 2
    assert (ev[0]["lr_scale_min"], ev[0]["lr_scale_max"]) == (0.75 ** (L + 1), 1.0)
    assert f"lr_scale_min:{0.75 ** (L + 1)}  lr_scale_max:1.0" in r.stdout
    ep = [x for x in recs if "epoch" in x]
    assert len(ep) == 1 and math.isfinite(ep[0]["loss_train"]) and math.isfinite(ep[0]["loss_val"])
