"""GRN and ConvNeXt V2 on the CPU: ops/grn.py under gradcheck and against the
closed-form backward (zero columns included), and the V2 model's parameters,
names, layer ids and trainer flags."""
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_model_parallel_amd.models import INPUT_SHAPES, MODELS, build_model, layer_ids
from distributed_model_parallel_amd.ops import grn as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(zero_column):
    torch.manual_seed(0)
    x = torch.randn(2, 5, 8, dtype=torch.float64)
    if zero_column:
        x[0, :, 3] = 0
    gamma, beta = torch.randn(8, dtype=torch.float64), torch.randn(8, dtype=torch.float64)
    return [t.requires_grad_() for t in (x, gamma, beta)]


def test_torch_route_gradcheck():
    assert torch.autograd.gradcheck(G.grn, _inputs(False))


def closed_form_backward(dg, a, gamma, H):
    """GRN's backward in closed form (a zero column gets no gradient through its norm)."""
    gx = a.pow(2).sum(1).sqrt()
    rd = 1 / (gx.mean(-1, keepdim=True) + 1e-6)
    P, S = (dg * a).sum(1), dg.sum(1)
    u = gamma * P
    w = (u * gx).sum(-1, keepdim=True)
    dgx = u * rd - w * rd * rd / H
    cc = torch.where(gx > 0, dgx / gx.clamp_min(1e-300), torch.zeros_like(gx))
    A = 1 + gamma * gx * rd
    return dg * A[:, None] + a * cc[:, None], (gx * rd * P).sum(0), S.sum(0)


@pytest.mark.parametrize("zero_column", [False, True])
def test_closed_form_backward_equals_autograd(zero_column):
    x, gamma, beta = _inputs(zero_column)
    dg = torch.randn_like(x)
    want = torch.autograd.grad(G.grn(x, gamma, beta), (x, gamma, beta), dg)
    assert all(torch.isfinite(t).all() for t in want)
    got = closed_form_backward(dg, x.detach(), gamma.detach(), 8)
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("name,count", [("convnextv2_pico", 9_066_280), ("convnextv2_tiny", 28_635_496),
                                        ("convnextv2_base", 88_717_800)])
def test_parameter_counts(name, count):
    with torch.device("meta"):
        m = build_model(name)
    assert sum(p.numel() for p in m.parameters()) == count
    assert INPUT_SHAPES[name] == ((3, 224, 224), 1000)


def test_state_dict_keys():
    v2, v1 = build_model("convnextv2_test"), build_model("convnext_test")
    k2, k1 = set(v2.state_dict()), set(v1.state_dict())
    blocks = {k.rsplit(".", 2)[0] for k in k1 if k.startswith("stages.") and k.endswith("fc1.weight")}
    assert len(blocks) == 5
    for b in blocks:
        assert f"{b}.grn.gamma" in k2 and f"{b}.grn.beta" in k2 and f"{b}.gamma" not in k2
        assert f"{b}.gamma" in k1 and f"{b}.grn.gamma" not in k1
    assert k2 - k1 == {f"{b}.grn.{p}" for b in blocks for p in ("gamma", "beta")}
    assert k1 - k2 == {f"{b}.gamma" for b in blocks}
    assert all(float(v2.state_dict()[f"{b}.grn.gamma"].abs().sum()) == 0 for b in blocks)  # the published init
    assert {"convnextv2_pico", "convnextv2_nano", "convnextv2_tiny", "convnextv2_base", "convnextv2_large",
            "convnextv2_test"} <= set(MODELS)


def test_layer_ids_cover_the_grn_parameters():
    m = build_model("convnextv2_test")
    ids, n = layer_ids(m)
    assert n == 14 and set(ids) == {k for k, _ in m.named_parameters()}
    names = [k for k in ids if ".grn." in k]
    assert len(names) == 10
    for k in names:
        assert ids[k] == ids[k.rsplit(".", 2)[0] + ".fc1.weight"], k


def test_cli_trains_convnextv2(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(33000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "none",
                        "--arch", "convnextv2_test", "--synthetic", "--optimizer", "adamw", "--drop-path", "0.1",
                        "-b", "8", "--epochs", "1", "--steps-per-epoch", "1", "--lr", "1e-3", "--warmup-epochs", "0",
                        "--log-dir", str(tmp_path / "log"), "-j", "0", "--checkpoint", str(tmp_path / "ck.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = dict(f.split(":", 1) for f in (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0
