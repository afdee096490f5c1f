"""Swin (models/swin.py, ops/window_attention.py) on the CPU: parameter counts,
the torch composition of shifted-window attention against a per-window fp64
loop written from the definition, the no-shift rule, and a training step."""
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_model_parallel_amd.models import INPUT_SHAPES, build_model, classifier_name
from distributed_model_parallel_amd.ops import window_attention as WA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,count", [("swin_tiny", 28_288_354), ("swin_small", 49_606_258),
                                        ("swin_base", 87_768_224)])
def test_parameter_counts(name, count):
    m = build_model(name)
    assert sum(p.numel() for p in m.parameters()) == count
    assert INPUT_SHAPES[name] == ((3, 224, 224), 1000) and classifier_name(m) == "head"
    assert m.blocks[1].attn.relative_position_bias_table.shape == (169, m.blocks[1].attn.heads)
    assert not list(m.buffers())


def _loop_reference(qkv, table, heads, hg, wg, ws, s):
    """Window by window, token by token, from the definition."""
    b, _t, d3 = qkv.shape
    d = d3 // 3
    hd = d // heads
    out = torch.zeros(b, hg * wg, d, dtype=qkv.dtype)

    def region(p, n):
        return 0 if s == 0 or p < n - ws else (1 if p < n - s else 2)

    for bi in range(b):
        for wy in range(hg // ws):
            for wx in range(wg // ws):
                loc = [(iy, ix) for iy in range(ws) for ix in range(ws)]
                tok = [((wy * ws + iy + s) % hg) * wg + (wx * ws + ix + s) % wg for iy, ix in loc]
                reg = [(region(wy * ws + iy, hg), region(wx * ws + ix, wg)) for iy, ix in loc]
                for h in range(heads):
                    q, k, v = (qkv[bi, tok, i * d + h * hd:i * d + (h + 1) * hd] for i in range(3))
                    att = q @ k.T / math.sqrt(hd)
                    for i, (iy, ix) in enumerate(loc):
                        for j, (jy, jx) in enumerate(loc):
                            att[i, j] += table[(iy - jy + ws - 1) * (2 * ws - 1) + ix - jx + ws - 1, h]
                            if reg[i] != reg[j]:
                                att[i, j] = -math.inf
                    out[bi, tok, h * hd:(h + 1) * hd] = att.softmax(-1) @ v
    return out


def test_torch_composition_matches_the_definition():
    torch.manual_seed(0)
    heads, hg, wg, ws, s = 2, 8, 8, 4, 2
    qkv = torch.randn(2, hg * wg, 3 * heads * 8, dtype=torch.float64)
    table = torch.randn((2 * ws - 1) ** 2, heads, dtype=torch.float64)
    got = WA.window_attention_packed(qkv, table, heads, (hg, wg), ws, s)
    torch.testing.assert_close(got, _loop_reference(qkv, table, heads, hg, wg, ws, s), atol=1e-12, rtol=1e-12)
    with pytest.raises(ValueError, match="window side"):
        WA.window_attention_packed(qkv[:, :56], table, heads, (7, 8), ws, s)


def test_no_shift_where_the_grid_equals_the_window(monkeypatch):
    import distributed_model_parallel_amd.models.swin as SW
    seen = []
    real = SW.window_attention_packed
    monkeypatch.setattr(SW, "window_attention_packed", lambda q, t, h, grid, w, shift: (
        seen.append((grid, shift)), real(q, t, h, grid, w, shift))[1])
    build_model("swin_test").eval()(torch.randn(1, 3, 32, 32))
    assert seen == [((8, 8), 0), ((8, 8), 2), ((4, 4), 0), ((4, 4), 0)]


def test_swin_test_trains_a_step():
    torch.manual_seed(1)
    m = build_model("swin_test", drop_path_rate=0.3).train()
    assert [b.drop_path for b in m.blocks] == pytest.approx([0.0, 0.1, 0.2, 0.3])
    x, y = torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    loss = torch.nn.functional.cross_entropy(m(x), y)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert m.blocks[1].attn.relative_position_bias_table.grad.abs().sum() > 0


def test_cli_trains_swin_with_drop_path(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(33000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "none",
                        "--arch", "swin_test", "--synthetic", "--optimizer", "adamw", "--drop-path", "0.1",
                        "-b", "8", "--epochs", "1", "--steps-per-epoch", "1", "--lr", "1e-3", "--warmup-epochs", "0",
                        "--log-dir", str(tmp_path / "log"), "-j", "0", "--checkpoint", str(tmp_path / "ck.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = dict(f.split(":", 1) for f in (tmp_path / "log" / "none_8.txt").read_text().strip().split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, rec
