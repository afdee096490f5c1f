"""Random erasing, the CPU side (data/random_erase.py): the oracle's Philox against the published
known answers, the host-drawn plan, the PyTorch composition of the noise definition (what is
written where, and that the values depend on (key, x, y, c) alone), its moments, the plan check
and the CLI flags."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_model_parallel_amd.data import RandomErasePlanner, random_erase_
from distributed_model_parallel_amd.data import random_erase as RE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1"))


def _hex(words):
    return " ".join(f"{int(v) & 0xFFFFFFFF:08x}" for v in words)


def _boxes(rows, keys=None):
    b = np.zeros((len(rows), 6), dtype=np.int32)
    b[:, :4] = rows
    if keys is None:
        keys = np.random.default_rng(99).integers(0, 1 << 32, size=(len(rows), 2), dtype=np.uint64)
    b[:, 4:] = np.asarray(keys, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return b


def _batch(B, C, H, W, dtype=torch.float32, channels_last=False, seed=0):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dtype)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert _hex(RE.philox4x32(np.array([counter], dtype=np.uint32), np.array(key, dtype=np.uint32))[0]) == want
    # signed words by their bit pattern, as the plan stores the key
    signed = RE.philox4x32(np.array([counter], dtype=np.uint32).view(np.int32), np.array(key, dtype=np.uint32).view(np.int32))
    assert _hex(signed[0]) == want
    # the int64-tensor rounds of the composition
    got = RE._philox_torch(*(torch.tensor([v], dtype=torch.int64) for v in counter), *key)
    assert _hex(v.item() for v in got) == want


def test_torch_rounds_equal_numpy_rounds_on_random_words():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1 << 32, size=(2048, 4), dtype=np.uint64)
    c[:8] = [[0, 0, 0, 0], [1, 1, 0, 0], [32767, 32767, 0, 0], [0xFFFFFFFF] * 4, [0x80000000] * 4, [0xFFFF, 0x10000, 0, 0],
             [0x7FFFFFFF] * 4, [0xFFFF0000, 0x0000FFFF, 1, 2]]
    for key in ((0, 0), (0xFFFFFFFF, 0x80000000), (0x12345678, 0x9ABCDEF0)):
        want = RE.philox4x32(c, np.array(key, dtype=np.uint64))
        got = RE._philox_torch(*(torch.from_numpy(c[:, i].astype(np.int64)) for i in range(4)), *key)
        assert np.array_equal(torch.stack(got, 1).numpy().astype(np.uint32), want)


def test_uniforms_are_exact_in_fp32_and_open():
    r = torch.tensor([0, 511, 512, 0xFFFFFFFF, 0x80000000], dtype=torch.int64)
    m = 2 * (r >> 9) + 1
    u32, u64 = m.to(torch.float32) * 2.0 ** -24, m.to(torch.float64) * 2.0 ** -24
    assert torch.equal(u32.double(), u64) and u64.min() == 2.0 ** -24 and u64.max() == 1 - 2.0 ** -24


# ---------------------------------------------------------------- the planner
def test_planner_is_seeded_by_seed_rank_epoch():
    def draws(seed, rank, epoch, mode="rand"):
        p = RandomErasePlanner(0.5, mode, seed=seed, rank=rank)
        p.set_epoch(epoch)
        return [p.plan(16, 32, 32) for _ in range(3)]

    a, b = draws(3, 1, 2), draws(3, 1, 2)
    for (ba, fa), (bb, fb) in zip(a, b):
        assert np.array_equal(ba, bb) and np.array_equal(fa, fb)
        assert ba.dtype == np.int32 and ba.shape == (16, 6) and fa.dtype == np.float32 and fa.shape == (16, 3)
    for other in (draws(4, 1, 2), draws(3, 0, 2), draws(3, 1, 5)):
        assert not np.array_equal(a[0][0], other[0][0]) and not np.array_equal(a[0][1], other[0][1])
    p = RandomErasePlanner(0.5, seed=3, rank=1)  # set_epoch(e) restarts the epoch's stream
    p.set_epoch(2)
    first = p.plan(16, 32, 32)[0]
    p.plan(16, 32, 32)
    p.set_epoch(2)
    assert np.array_equal(p.plan(16, 32, 32)[0], first)
    assert RandomErasePlanner(0.5, "pixel").plan(4, 8, 8)[1] is None
    assert RandomErasePlanner(0.5, "const").plan(4, 8, 8)[1] is None


def test_planner_draws_fresh_keys():
    p = RandomErasePlanner(0.25, seed=1)
    steps = [p.plan(64, 32, 32)[0] for _ in range(4)]
    keys = np.concatenate([b[:, 4:].copy().view(np.uint32).astype(np.uint64) for b in steps])
    k64 = keys[:, 0] << np.uint64(32) | keys[:, 1]
    assert len(set(k64.tolist())) == 256  # per sample within a step and across steps
    assert (keys[:, 0] >> np.uint64(31)).any() and not (keys[:, 0] >> np.uint64(31)).all()  # all 32 bits are drawn


@pytest.mark.parametrize("hw", [(224, 224), (32, 32), (37, 53), (8, 8), (3, 200)])
def test_planner_boxes_pass_the_host_check(hw):
    H, W = hw
    p = RandomErasePlanner(1.0, seed=7)
    x = torch.zeros(64, 1, H, W)
    for _ in range(20):
        boxes, _ = p.plan(64, H, W)
        RE._check_plan(x, boxes, None, True)
        x0, y0, w, h = (boxes[:, i] for i in range(4))
        assert ((w == 0) == (h == 0)).all() and (w < W).all() and (h < H).all()
        assert (x0 >= 0).all() and (y0 >= 0).all() and (x0 + w <= W).all() and (y0 + h <= H).all()
        e = w > 0
        area, ar = (w[e] * h[e]) / (H * W), h[e] / w[e]
        if H * W >= 224 * 224:  # sides of 17 pixels and more: rounding them moves each by 3 % at the most
            assert area.min() > 0.02 * 0.9 and area.max() < 1 / 3 * 1.1
            assert ar.min() > 0.3 * 0.9 and ar.max() < 1 / 0.3 * 1.1


def test_planner_erases_the_share_it_is_asked_for():
    p = RandomErasePlanner(0.25, seed=11)
    n = sum(int((p.plan(500, 224, 224)[0][:, 2] > 0).sum()) for _ in range(40))
    assert abs(n / 20000 - 0.25) <= 5 * math.sqrt(0.25 * 0.75 / 20000), n


def test_planner_extremes():
    p = RandomErasePlanner(0.0, seed=2)
    assert all((p.plan(100, 32, 32)[0][:, :4] == 0).all() for _ in range(10))
    p = RandomErasePlanner(1.0, seed=2)
    x = torch.zeros(100, 3, 2, 2)
    seen = set()
    for _ in range(20):
        boxes, _ = p.plan(100, 2, 2)
        RE._check_plan(x, boxes, None, True)  # a valid box ...
        seen |= {tuple(r) for r in boxes[:, 2:4].tolist()}
    assert seen <= {(0, 0), (1, 1)}, seen  # ... (1 x 1: the only one with w < 2 and h < 2) or none
    for bad in (dict(prob=1.5), dict(prob=-0.1), dict(prob=0.5, mode="noise"), dict(prob=0.5, min_area=0.5, max_area=0.4),
                dict(prob=0.5, min_aspect=0.0), dict(prob=0.5, channels=5)):
        with pytest.raises(ValueError, match="RandomErasePlanner"):
            RandomErasePlanner(**bad)


# ---------------------------------------------------------------- random_erase_ on CPU tensors
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_outside_the_boxes_every_bit_stays(dtype, channels_last):
    B, C, H, W = 5, 3, 37, 53
    x = _batch(B, C, H, W, dtype, channels_last)
    x[0, 0, 0, 0], x[1, 1, 3, 3] = float("nan"), float("-inf")  # bits, not values
    before = x.clone()
    rows = [(5, 7, 20, 11), (0, 0, 0, 0), (52, 36, 1, 1), (0, 0, 53, 37), (10, 0, 43, 37)]
    boxes = _boxes(rows)
    out = random_erase_(x, boxes)
    assert out is x and x.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    inside = torch.zeros(B, 1, H, W, dtype=torch.bool)
    for i, (x0, y0, w, h) in enumerate(rows):
        inside[i, :, y0:y0 + h, x0:x0 + w] = True
    inside = inside.expand(-1, C, -1, -1)
    assert torch.equal(_bits(x)[~inside], _bits(before)[~inside])
    assert torch.isfinite(x[inside].float()).all() and x[inside].float().abs().max() <= RE.Z_MAX
    assert (_bits(x)[inside] != _bits(before)[inside]).float().mean() > 0.99


def test_values_depend_on_key_and_pixel_alone():
    H, W = 24, 40
    keys = [(0xDEADBEEF, 0x80000001), (7, 9)]
    rows = [(3, 5, 30, 12), (0, 0, 0, 0), (3, 5, 30, 12)]
    ref = random_erase_(_batch(3, 3, H, W), _boxes(rows, [keys[0], keys[1], keys[1]]))
    assert not torch.equal(ref[0], ref[2])  # another key: another field
    # another layout, dtype, channel count and batch position: the same values
    cl = random_erase_(_batch(3, 3, H, W, channels_last=True, seed=1), _boxes(rows, [keys[0], keys[1], keys[1]]))
    assert torch.equal(cl[[0, 2], :, 5:17, 3:33], ref[[0, 2], :, 5:17, 3:33])
    bf = random_erase_(_batch(3, 3, H, W, torch.bfloat16), _boxes(rows, [keys[0], keys[1], keys[1]]))
    assert torch.equal(bf[0, :, 5:17, 3:33], ref[0, :, 5:17, 3:33].bfloat16())
    moved = random_erase_(_batch(2, 4, H, W), _boxes([(0, 0, 0, 0), (3, 5, 30, 12)], [keys[1], keys[0]]))
    assert torch.equal(moved[1, :3, 5:17, 3:33], ref[0, :, 5:17, 3:33])
    one = random_erase_(_batch(1, 1, H, W), _boxes([(3, 5, 30, 12)], [keys[0]]))
    assert torch.equal(one[0, 0, 5:17, 3:33], ref[0, 0, 5:17, 3:33])
    # another box under the same key reads the same field (absolute coordinates), also in a larger image
    other = random_erase_(_batch(1, 3, H + 9, W + 4), _boxes([(10, 8, 29, 20)], [keys[0]]))
    assert torch.equal(other[0, :, 8:17, 10:33], ref[0, :, 8:17, 10:33])
    # and the definition itself, element by element, from the NumPy generator
    r = RE.philox4x32(np.array([[17, 9, 0, 0]]), np.array(keys[0], dtype=np.uint64))[0]
    u = (2.0 * (r >> 9) + 1.0) * 2.0 ** -24
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3])]
    assert np.allclose(ref[0, :, 9, 17].double().numpy(), want, rtol=0, atol=1e-5)
    x64 = random_erase_(torch.zeros(1, 4, H, W, dtype=torch.float64), _boxes([(3, 5, 30, 12)], [keys[0]]))
    assert np.allclose(x64[0, :3, 9, 17].numpy(), want, rtol=0, atol=1e-12)
    assert abs(x64[0, 3, 9, 17].item() - math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])) < 1e-12


@pytest.mark.parametrize("channels_last", [False, True])
def test_const_and_rand_modes(channels_last):
    rows = [(1, 2, 5, 4), (0, 0, 0, 0), (0, 0, 8, 8)]
    x = _batch(3, 3, 8, 8, channels_last=channels_last)
    before = x.clone()
    random_erase_(x, _boxes(rows), noise=False)
    assert (x[0, :, 2:6, 1:6] == 0).all() and (x[2] == 0).all() and torch.equal(x[1], before[1])
    assert torch.equal(x[0, :, :2], before[0, :, :2]) and torch.equal(x[0, :, :, 6:], before[0, :, :, 6:])
    fill = np.random.default_rng(1).standard_normal((3, 3)).astype(np.float32)
    x = before.clone().bfloat16()
    random_erase_(x, _boxes(rows), fill=fill, noise=False)
    want = torch.from_numpy(fill).bfloat16()
    assert torch.equal(x[0, :, 2:6, 1:6], want[0].view(3, 1, 1).expand(3, 4, 5))
    assert torch.equal(x[2], want[2].view(3, 1, 1).expand(3, 8, 8)) and torch.equal(x[1], before[1].bfloat16())
    # the planner's rand plan goes through as drawn
    p = RandomErasePlanner(1.0, "rand", seed=3)
    boxes, fill = p.plan(3, 8, 8)
    assert p.noise is False and RandomErasePlanner(1.0, "pixel").noise is True
    y = random_erase_(before.clone(), boxes, fill, noise=p.noise)
    i = int(np.flatnonzero(boxes[:, 2] > 0)[0])
    x0, y0, w, h = boxes[i, :4]
    assert torch.equal(y[i, :, y0:y0 + h, x0:x0 + w], torch.from_numpy(fill[i]).view(3, 1, 1).expand(3, int(h), int(w)))


def moment_plan():
    """16 samples with a 64 x 64 x 3 box, keys from default_rng([0, 0, 0]): 196 608 values.  The fp64
    evaluation of the definition gives mean 0.00047, var 0.9960, max |z| 4.64 for these keys."""
    keys = np.random.default_rng([0, 0, 0]).integers(0, 1 << 32, size=(16, 2), dtype=np.uint64)
    return _boxes([(0, 0, 64, 64)] * 16, keys)


def check_moments(z):
    z = z.double().flatten()
    n = z.numel()
    assert n == 196608
    mean, var, top = z.mean().item(), z.var(unbiased=False).item(), z.abs().max().item()
    print(f"mean {mean:.5f} var {var:.5f} max {top:.4f}")
    assert abs(mean) < 5 / math.sqrt(n)  # 0.0113
    assert abs(var - 1) < 5 * math.sqrt(2 / n)  # 0.0160
    assert top <= 5.77


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_moments(dtype):
    check_moments(random_erase_(torch.zeros(16, 3, 64, 64, dtype=dtype), moment_plan()))


def test_no_erased_row_takes_no_path():
    before = dict(RE._STATS)
    x = _batch(2, 3, 8, 8)
    keep = x.clone()
    random_erase_(x, _boxes([(0, 0, 0, 0), (0, 0, 0, 0)]))
    assert RE._STATS == before and torch.equal(x, keep)
    random_erase_(x, _boxes([(0, 0, 0, 0), (0, 0, 1, 1)]))
    assert RE._STATS["torch"] == before["torch"] + 1 and RE._STATS["native"] == before["native"]


# ---------------------------------------------------------------- the plan check
def test_plan_check_raises_and_names_the_row():
    x = _batch(3, 3, 8, 10)
    good = [(0, 0, 10, 8), (0, 0, 0, 0), (9, 7, 1, 1)]
    random_erase_(x.clone(), _boxes(good))
    for row, bad in ((0, (-1, 0, 2, 2)), (1, (0, -1, 2, 2)), (2, (9, 0, 2, 2)), (0, (0, 7, 2, 2)), (1, (0, 0, 11, 1)),
                     (2, (0, 0, 1, 9)), (0, (0, 0, 0, 3)), (1, (0, 0, 3, 0)), (2, (0, 0, -2, 2)), (0, (0, 0, 2, -2)),
                     (1, (2 ** 31 - 1, 0, 2, 2))):
        rows = list(good)
        rows[row] = bad
        keep = x.clone()
        with pytest.raises(ValueError, match=f"random_erase_: boxes row {row} "):
            random_erase_(keep, _boxes(rows))
        assert torch.equal(keep, x)  # nothing is written before the check has passed
    b = _boxes(good)
    fill = np.zeros((3, 3), dtype=np.float32)
    for boxes, kw, msg in ((b.astype(np.int64), {}, "int32"), (b[:2], {}, "int32"), (b[:, :5], {}, "int32"),
                           (b, dict(fill=fill), "exclude"), (b, dict(fill=fill.astype(np.float64), noise=False), "float32"),
                           (b, dict(fill=fill[:, :2], noise=False), "float32")):
        with pytest.raises(ValueError, match=msg):
            random_erase_(x.clone(), boxes, **kw)
    for bad_x in (torch.zeros(3, 5, 8, 10), torch.zeros(3, 8, 10), torch.zeros(3, 3, 8, 10, dtype=torch.int32)):
        with pytest.raises(ValueError, match="random_erase_: x must be"):
            random_erase_(bad_x, b)
    random_erase_(x.clone(), torch.from_numpy(b))  # a host tensor is a plan too


def test_feature_is_registered_and_exported():
    from distributed_model_parallel_amd import _native, data
    assert "random_erase" in _native.FEATURES
    assert data.RandomErasePlanner is RandomErasePlanner and data.random_erase_ is random_erase_
    assert "Philox4x32-10" in RE.__doc__ and "0xD2511F53" in RE.__doc__ and "2^-24" in RE.__doc__


# ---------------------------------------------------------------- CLI
def test_cli_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert a.reprob == 0.0 and a.remode == "pixel"
    a = p.parse_args(["--reprob", "0.25", "--remode", "rand"])
    check_args(p, a)
    assert a.reprob == 0.25 and a.remode == "rand"
    check_args(p, p.parse_args(["--reprob", "1.0", "--gpu-augment"]))
    for argv, msg in ((["--remode", "pixel"], "--remode needs --reprob"),
                      (["--reprob", "1.5"], "--reprob must be in [0, 1]"),
                      (["--reprob", "-0.1"], "--reprob must be in [0, 1]"),
                      (["--reprob", "0.25", "--parallel", "pipe"], "--reprob with --parallel pipe is not supported"),
                      (["--reprob", "0.25", "--remode", "noise"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def _train(tmp_path, name, *extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(33000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--arch", "mobilenetv2",
                        "--synthetic", "-b", "8", "--epochs", "1", "--steps-per-epoch", "2", "--lr", "0.05",
                        "--warmup-epochs", "0", "--log-dir", str(tmp_path / name), "-j", "0", "--parallel", "none",
                        "--checkpoint", str(tmp_path / f"{name}.pth"), *extra], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / name / "none_8.txt").read_text().strip().splitlines()
    assert len(lines) == 1
    return dict(f.split(":", 1) for f in lines[0].split("  "))


def test_cli_trains_with_random_erasing(tmp_path):
    plain = _train(tmp_path, "plain")
    erased = _train(tmp_path, "erased", "--reprob", "1.0")
    for rec in (plain, erased):
        assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, rec
        assert math.isfinite(float(rec["loss_val"])), rec
    assert float(erased["loss_train"]) != float(plain["loss_train"]), (plain, erased)
