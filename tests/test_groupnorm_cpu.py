"""GroupNorm on the CPU: the torch path of ops/groupnorm.py against
F.group_norm in fp64, nn.GroupNorm state dicts, the GN models' parameter
counts and optimizer groups, the pipeline cut, one CLI step, and the kernels'
resource usage where a compiler is present."""
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.models import INPUT_SHAPES, MODELS, build_model
from distributed_model_parallel_amd.ops import groupnorm as GN
from distributed_model_parallel_amd.ops.fused import conv_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("act", [None, "relu", "relu6"])
@pytest.mark.parametrize("residual", [False, True])
def test_torch_path_against_group_norm(act, residual):
    gen = torch.Generator().manual_seed(3)
    x = (3 * torch.randn(2, 12, 3, 5, dtype=torch.float64, generator=gen) + 2).requires_grad_()
    w = (3 * torch.randn(12, dtype=torch.float64, generator=gen)).requires_grad_()
    b = (torch.randn(12, dtype=torch.float64, generator=gen) + 2).requires_grad_()
    r = (3 * torch.randn(2, 12, 3, 5, dtype=torch.float64, generator=gen)).requires_grad_() if residual else None
    want = F.group_norm(x, 3, w, b, 1e-5) + (r if residual else 0)
    want = F.relu6(want) if act == "relu6" else F.relu(want) if act == "relu" else want
    got = GN.group_norm_act(x, 3, w, b, 1e-5, act, r)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    if act is not None:
        assert 0.05 < float((got == 0).double().mean()) < 0.95
    args = (x, w, b) + ((r,) if residual else ())
    assert torch.autograd.gradcheck(
        lambda x, w, b, r=None: GN.group_norm_act(x, 3, w, b, 1e-5, act, r), args)


def test_state_dict_and_conv_bn_route():
    stock, ours = nn.GroupNorm(4, 16), GN.GroupNormAct2d(4, 16, act="relu")
    with torch.no_grad():
        stock.weight.normal_()
        stock.bias.normal_()
    ours.load_state_dict(stock.state_dict())
    assert set(ours.state_dict()) == set(stock.state_dict())
    conv, x, res = nn.Conv2d(8, 16, 1), torch.randn(2, 8, 4, 4), torch.randn(2, 16, 4, 4)
    want = F.relu(stock(conv(x)) + res)  # the residual goes in before the ReLU
    assert torch.allclose(conv_bn(conv, ours, x, res), want, atol=1e-5)
    assert "groupnorm" in _native.FEATURES and GN.stats()["torch_fwd"] > 0


@pytest.mark.parametrize("gn,bn", [("mobilenetv2_gn", "mobilenetv2"), ("resnet50_gn", "resnet50")])
def test_gn_models(gn, bn):
    m, ref = build_model(gn), build_model(bn)
    assert sum(p.numel() for p in m.parameters()) == sum(p.numel() for p in ref.parameters() if p.requires_grad)
    assert INPUT_SHAPES[gn] == INPUT_SHAPES[bn] and gn in MODELS
    norms = [mod for mod in m.modules() if isinstance(mod, GN.GroupNormAct2d)]
    assert norms and not any(isinstance(mod, nn.BatchNorm2d) for mod in m.modules())
    assert all(mod.num_channels // mod.num_groups == 8 for mod in norms) if gn.startswith("mobilenet") else \
        all(mod.num_groups == 32 for mod in norms)
    assert all(p.dim() == 1 for mod in norms for p in mod.parameters())  # 1-D: the optimizers' no-decay set
    assert len(m.as_sequential()) == len(ref.as_sequential())  # the pipeline partitioner's atoms


def test_zero_init_residual_zeroes_the_last_gn():
    from distributed_model_parallel_amd.models.resnet import Bottleneck
    m = build_model("resnet50_gn", zero_init_residual=True)
    blocks = [b for b in m.modules() if isinstance(b, Bottleneck)]
    assert len(blocks) == 16 and all(float(b.bn3.weight.abs().sum()) == 0 for b in blocks)
    assert all(float(b.bn1.weight.sum()) == b.bn1.num_channels for b in blocks)


def test_cli_trains_mobilenetv2_gn(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(34000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "none",
                        "--arch", "mobilenetv2_gn", "--synthetic", "-b", "8", "--epochs", "1",
                        "--steps-per-epoch", "1", "--lr", "1e-2", "--warmup-epochs", "0",
                        "--log-dir", str(tmp_path / "log"), "-j", "0", "--checkpoint", str(tmp_path / "ck.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = dict(f.split(":", 1) for f in (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_groupnorm_kernel_resources():
    from tools.kernel_resources import resources
    ks = resources(os.path.join(ROOT, "csrc", "norm", "groupnorm.hip"))
    by = {tag: [k for k in ks if tag in k["name"]] for tag in ("gn_fwd_kernel", "gn_bwd_kernel", "finalize_kernel")}
    # (bf16, fp32) x 4 channel splits x (resident small, resident full, stats, apply); colreduce in two dtypes
    assert len(by["gn_fwd_kernel"]) == 32 and len(by["gn_bwd_kernel"]) == 32 and len(by["finalize_kernel"]) == 2
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] != "0"]
    assert not bad, bad
    assert max(int(k["lds"]) for k in by["gn_fwd_kernel"]) <= 163840 // 2   # two forward blocks per CU
    assert max(int(k["lds"]) for k in by["gn_bwd_kernel"]) <= 163840
