"""Stochastic depth (drop path) on the CPU: the mask draw, the torch route of
linear_residual / mlp_residual with a per-sample scale, the ViT model's
per-block rates, state_dict and RNG behaviour, activation checkpointing and
the trainer's --drop-path flag."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_model_parallel_amd.models import vit_tiny
from distributed_model_parallel_amd.ops import drop_path as DP
from distributed_model_parallel_amd.ops import linear as L


# ---------------------------------------------------------------- the draw
def test_sample_scales_values_shape_dtype():
    torch.manual_seed(3)
    before = DP._STATS["draws"]
    s = DP.sample_scales(2, 4096, 0.25, "cpu")
    assert DP._STATS["draws"] == before + 1
    assert s.shape == (2, 4096) and s.dtype == torch.float32
    keep = torch.tensor(1.0 / (1.0 - 0.25))
    assert bool(((s == 0) | (s == keep)).all())
    # both outcomes occur, near their odds (4 sigma of a binomial over 8192 draws is 0.02)
    assert abs(float((s == 0).float().mean()) - 0.25) < 0.02
    assert torch.equal(DP.sample_scales(3, 7, 0.0, "cpu"), torch.ones(3, 7))
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            DP.sample_scales(1, 1, bad, "cpu")


def test_sample_scales_follows_the_default_generator():
    torch.manual_seed(11)
    a = DP.sample_scales(2, 64, 0.5, "cpu")
    torch.manual_seed(11)
    b = DP.sample_scales(2, 64, 0.5, "cpu")
    c = DP.sample_scales(2, 64, 0.5, "cpu")
    assert torch.equal(a, b) and not torch.equal(b, c)


# ---------------------------------------------------------------- torch route of the ops
B, T, D, H = 4, 5, 32, 64
SCALES = [0.0, 1.0, 2.0, 0.5]


def _leaf(*shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype).requires_grad_()


def _check_grads(got, want, rtol=1e-4, atol=1e-5):
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w.float(), rtol=rtol, atol=atol)


def test_linear_residual_row_scale_matches_fp64():
    s = torch.tensor(SCALES)
    x, res = _leaf(B, T, D, seed=0), _leaf(B, T, D, seed=1)
    w, b = _leaf(D, D, seed=2, scale=D ** -0.5), _leaf(D, seed=3)
    dy = _leaf(B, T, D, seed=4).detach()
    y = L.linear_residual(x, res, w, b, row_scale=s)
    y.backward(dy)
    x6, r6, w6, b6 = (t.detach().double().requires_grad_() for t in (x, res, w, b))
    y6 = r6 + s.double().view(B, 1, 1) * F.linear(x6, w6, b6)
    y6.backward(dy.double())
    torch.testing.assert_close(y, y6.float(), rtol=1e-4, atol=1e-5)
    _check_grads((x.grad, res.grad, w.grad, b.grad), (x6.grad, r6.grad, w6.grad, b6.grad))
    assert torch.equal(res.grad, dy)  # the residual's gradient is the upstream gradient itself
    assert torch.count_nonzero(x.grad[0]) == 0 and torch.count_nonzero(x.grad[1]) > 0


def test_mlp_residual_row_scale_matches_fp64():
    s = torch.tensor(SCALES)
    fc1, fc2 = nn.Linear(D, H), nn.Linear(H, D)
    x, res = _leaf(B, T, D, seed=5), _leaf(B, T, D, seed=6)
    dy = _leaf(B, T, D, seed=7).detach()
    y = L.mlp_residual(x, res, fc1, fc2, 0.0, True, row_scale=s)
    y.backward(dy)
    params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    x6, r6, w1, b1, w2, b2 = (t.detach().double().requires_grad_() for t in (x, res) + params)
    y6 = r6 + s.double().view(B, 1, 1) * F.linear(F.gelu(F.linear(x6, w1, b1)), w2, b2)
    y6.backward(dy.double())
    torch.testing.assert_close(y, y6.float(), rtol=1e-4, atol=1e-5)
    _check_grads((x.grad, res.grad) + tuple(p.grad for p in params),
                 (x6.grad, r6.grad, w1.grad, b1.grad, w2.grad, b2.grad))
    assert torch.equal(res.grad, dy)
    assert torch.count_nonzero(x.grad[0]) == 0 and torch.count_nonzero(x.grad[3]) > 0


def test_row_scale_none_is_the_plain_call():
    x, res = _leaf(B, T, D, seed=8), _leaf(B, T, D, seed=9)
    w, b = _leaf(D, D, seed=10), _leaf(D, seed=11)
    assert torch.equal(L.linear_residual(x, res, w, b, None), L.linear_residual(x, res, w, b))
    assert torch.equal(L.linear_residual(x, res, w, b, torch.ones(B)), L.linear_residual(x, res, w, b))


# ---------------------------------------------------------------- the model
def _images(n=6):
    return torch.randn(n, 3, 32, 32, generator=torch.Generator().manual_seed(0))


def _nonzero_head(model):
    # the classifier head starts at zero (logits would not depend on the blocks)
    with torch.no_grad():
        model.head.weight.normal_(std=0.1, generator=torch.Generator().manual_seed(1))
    return model


def test_vit_rates_state_dict_and_eval():
    torch.manual_seed(0)
    plain = _nonzero_head(vit_tiny())
    model = vit_tiny(drop_path_rate=0.5)
    assert [blk.drop_path for blk in model.blocks] == [0.0, 0.5]
    assert [blk.drop_path for blk in plain.blocks] == [0.0, 0.0]
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    model.load_state_dict(plain.state_dict())
    x = _images()
    with torch.no_grad():
        assert torch.equal(model.eval()(x), plain.eval()(x))
    with pytest.raises(ValueError):
        vit_tiny(drop_path_rate=1.0)


def test_vit_train_forward_follows_the_seed():
    torch.manual_seed(0)
    model = _nonzero_head(vit_tiny(drop_path_rate=0.5)).train()
    x = _images()
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        outs.append(model(x).detach())
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], outs[2])


def test_rate_zero_makes_no_random_call():
    torch.manual_seed(0)
    model = vit_tiny().train()
    state = torch.get_rng_state()
    before = DP._STATS["draws"]
    model(_images()).sum().backward()
    assert torch.equal(torch.get_rng_state(), state)
    assert DP._STATS["draws"] == before


def test_every_parameter_gets_a_gradient():
    torch.manual_seed(0)
    model = _nonzero_head(vit_tiny(drop_path_rate=0.9)).train()  # block 1 drops nearly every sample
    torch.manual_seed(1)
    model(_images()).square().sum().backward()
    assert all(p.grad is not None for p in model.parameters())


def test_activation_checkpointing_recomputes_the_same_masks():
    from distributed_model_parallel_amd.utils.checkpointing import enable_activation_checkpointing
    torch.manual_seed(0)
    ref = _nonzero_head(vit_tiny(drop_path_rate=0.5)).train()
    torch.manual_seed(0)
    ck = _nonzero_head(vit_tiny(drop_path_rate=0.5)).train()
    ck.load_state_dict(ref.state_dict())
    assert enable_activation_checkpointing(ck, 2) == 1
    x = _images()
    for m in (ref, ck):
        torch.manual_seed(7)
        m(x).square().sum().backward()
    for (name, p), q in zip(ref.named_parameters(), ck.parameters()):
        torch.testing.assert_close(q.grad, p.grad, msg=lambda m, name=name: f"{name}: {m}")


# ---------------------------------------------------------------- trainer
def test_cli_drop_path_flag(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert a.drop_path == 0.0
    a = p.parse_args(["--arch", "vit_tiny", "--drop-path", "0.1"])
    check_args(p, a)
    assert a.drop_path == 0.1
    for argv, msg in ((["--arch", "vit_tiny", "--drop-path", "1.0"], "[0, 1)"),
                      (["--arch", "vit_tiny", "--drop-path", "-0.1"], "[0, 1)"),
                      (["--drop-path", "0.1", "--arch", "resnet50"], "ViT archs only")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_step_config_passes_the_rate_to_vit_only():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    assert StepConfig().drop_path_rate == 0.0
    cfg = StepConfig(model="vit_tiny", parallel="none", dtype=torch.float32, batch_size=4, lr=0.01,
                     channels_last=False, drop_path_rate=0.5)
    st = build_train_state(cfg, torch.device("cpu"))
    assert [blk.drop_path for blk in st.model.blocks] == [0.0, 0.5]
    assert torch.isfinite(st.step())
    with pytest.raises(ValueError):
        build_train_state(StepConfig(model="mobilenetv2", parallel="none", dtype=torch.float32, batch_size=2,
                                     channels_last=False, drop_path_rate=0.1), torch.device("cpu"))
