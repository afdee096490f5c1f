"""ConvNeXt (models/convnext.py) on the CPU: parameter counts, the model and
its folded layer scale against the plain-torch mirror, the drop-path rule, the
optimizers' no-decay set and the trainer's flags."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd.models import INPUT_SHAPES, MODELS, build_model
from distributed_model_parallel_amd.models import convnext as CN
from distributed_model_parallel_amd.ops import drop_path as DP
from tests.convnext_mirror import grads, mirror_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("name,count", [("convnext_tiny", 28_589_128), ("convnext_small", 50_223_688),
                                        ("convnext_base", 88_591_464)])
def test_parameter_counts(name, count):
    with torch.device("meta"):
        m = build_model(name)
    assert sum(p.numel() for p in m.parameters()) == count
    assert INPUT_SHAPES[name] == ((3, 224, 224), 1000) and name in MODELS


def test_zoo_entries_and_init():
    assert INPUT_SHAPES["convnext_test"] == ((3, 32, 32), 10)
    m = build_model("convnext_test")
    assert m.depths == (1, 1, 2, 1) and m.dims == (8, 16, 32, 64) and m.head.out_features == 10
    for n, p in m.named_parameters():
        if n.endswith("gamma"):
            assert p.shape == (p.numel(),) and torch.all(p == 1e-6)
        elif n.endswith("bias") and "norm" not in n:
            assert torch.all(p == 0), n
        elif p.dim() > 1:
            assert 0.01 < float(p.detach().std()) < 0.03 and float(p.detach().abs().max()) <= 2.0, n
    m3 = CN.ConvNeXt((1, 2, 1), (8, 16, 24), num_classes=5)  # any number of stages
    assert m3(torch.randn(2, 3, 32, 32)).shape == (2, 5)


def _case(layer_scale, seed=0, **kw):
    torch.manual_seed(seed)
    m = build_model("convnext_test", layer_scale=layer_scale, **kw).train()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1 and float(p.abs().sum()) == 0:
                p.normal_(std=0.05)
    x = torch.randn(6, 3, 32, 32)
    y = torch.randint(0, 10, (6,))
    return m, mirror_of(m).train(), x, y


@pytest.mark.parametrize("layer_scale", [1.0, 1e-6, 0.3])
def test_forward_backward_match_the_mirror(layer_scale):
    """The token layout, the folded layer scale and the GradSlot wiring against
    NCHW modules with the explicit gamma: loss and every gradient, gamma's included."""
    m, ref, x, y = _case(layer_scale)
    torch.testing.assert_close(m(x), ref(x), **TOL)
    l_m, g_m = grads(m, x, y)
    l_r, g_r = grads(ref, x, y)
    assert abs(l_m - l_r) < 1e-5
    assert set(g_m) == set(g_r)
    for n in g_r:
        torch.testing.assert_close(g_m[n], g_r[n], **TOL, msg=lambda s, n=n: f"{n}: {s}")
    assert any(n.endswith("gamma") and float(g_r[n].abs().max()) > 1e-4 for n in g_r)


def test_folded_operands_are_the_explicit_form():
    torch.manual_seed(1)
    blk = CN.ConvNeXtBlock(16, layer_scale=0.5)
    with torch.no_grad():
        blk.gamma.uniform_(0.2, 2.0)
        blk.fc2.bias.normal_()
    w2, b2, w2_t = blk.folded_fc2()
    assert w2_t is None  # CPU: no fused route, no transposed operand
    a = torch.randn(5, 64)
    torch.testing.assert_close(F.linear(a, w2, b2), blk.gamma * blk.fc2(a), **TOL)


def test_drop_path_rates_and_draws(monkeypatch):
    m = build_model("convnext_test", drop_path_rate=0.4)
    rates = [b.drop_path for b in m.blocks]
    assert len(rates) == 5 and rates == pytest.approx([0.4 * i / 4 for i in range(5)])
    with pytest.raises(ValueError):
        build_model("convnext_test", drop_path_rate=1.0)
    x = torch.randn(4, 3, 32, 32)
    d0 = DP._STATS["draws"]
    m.train()
    m(x)
    assert DP._STATS["draws"] == d0 + 4  # block 0 has rate 0
    m.eval()
    m(x)
    assert DP._STATS["draws"] == d0 + 4
    plain = build_model("convnext_test").train()
    plain(x)
    assert DP._STATS["draws"] == d0 + 4
    # fixed scales: the same result as the mirror given the same vectors
    m, ref, x, y = _case(1.0, seed=2, drop_path_rate=0.4)
    g = torch.Generator().manual_seed(5)
    scales = [(torch.rand(6, generator=g) < 0.6).float() / 0.6 for _ in range(4)]
    it = iter(scales)
    monkeypatch.setattr(CN, "sample_scales", lambda n, b, r, d: next(it).view(1, -1))
    l_m, g_m = grads(m, x, y)
    l_r, g_r = grads(ref, x, y, scales=[None] + scales)
    assert abs(l_m - l_r) < 1e-5
    for n in g_r:
        torch.testing.assert_close(g_m[n], g_r[n], **TOL, msg=lambda s, n=n: f"{n}: {s}")


def test_adamw_puts_gamma_in_the_no_decay_set():
    from distributed_model_parallel_amd.ops.optim import FlatAdamW, MasterAdamW
    assert FlatAdamW._decay_masks is MasterAdamW._decay_masks  # one rule for both: ndim <= 1
    torch.manual_seed(3)
    m = build_model("convnext_test", layer_scale=0.5)
    lr, wd = 1e-2, 0.1
    o = MasterAdamW(m.parameters(), lr=lr, weight_decay=wd)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    o.step()  # zero gradients: only decay moves anything
    moved = 0
    for k, v in m.state_dict().items():
        if v.dim() <= 1:
            assert torch.equal(v, before[k]), k
        else:
            torch.testing.assert_close(v, before[k] * (1 - lr * wd), atol=1e-7, rtol=1e-6, msg=k)
            moved += 1
    assert moved > 0 and sum(k.endswith("gamma") for k in before) == 5


def test_cli_flags(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args(["--arch", "convnext_test", "--drop-path", "0.1"])
    check_args(p, a)
    assert a.drop_path == 0.1
    for argv, msg in ((["--arch", "resnet50", "--drop-path", "0.1"], "--drop-path is for ViT archs only"),
                      (["--arch", "convnext_test", "--image-size", "64"], "--image-size is for ViT archs only")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_step_config_passes_the_rate():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    cfg = StepConfig(model="convnext_test", parallel="none", dtype=torch.float32, batch_size=4, lr=0.01,
                     channels_last=False, drop_path_rate=0.4)
    st = build_train_state(cfg, torch.device("cpu"))
    assert [b.drop_path for b in st.model.blocks] == pytest.approx([0.0, 0.1, 0.2, 0.3, 0.4])
    assert torch.isfinite(st.step())
    with pytest.raises(ValueError, match="--drop-path is for ViT archs only"):
        build_train_state(StepConfig(model="resnet18", parallel="none", dtype=torch.float32, batch_size=2,
                                     channels_last=False, drop_path_rate=0.1), torch.device("cpu"))


def test_cli_trains_convnext_with_drop_path(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(32000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "none",
                        "--arch", "convnext_test", "--synthetic", "--optimizer", "adamw", "--drop-path", "0.1",
                        "-b", "8", "--epochs", "1", "--steps-per-epoch", "2", "--lr", "1e-3", "--warmup-epochs", "0",
                        "--log-dir", str(tmp_path / "log"), "-j", "0", "--checkpoint", str(tmp_path / "ck.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()
    assert len(lines) == 1
    rec = dict(f.split(":", 1) for f in lines[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, lines[0]
    import json
    recs = [json.loads(ln) for f in (tmp_path / "log").glob("*.jsonl") for ln in f.read_text().splitlines()]
    epochs = [r_ for r_ in recs if "loss_train" in r_]
    assert len(epochs) == 1 and epochs[0]["drop_path"] == 0.1, recs
