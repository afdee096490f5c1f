"""GPU-side augmentation, the CPU side (data/gpu_augment.py): the PyTorch
composition against the existing CPU transforms bit for bit, the host-drawn
plans, the plan checks, the uint8 synthetic set, the CLI flag and a CIFAR-10
loader end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_model_parallel_amd.data import (CIFAR10, AugmentPlanner, SyntheticImages, gpu_augment,
                                                 transforms as T)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(n=64, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pad_crop_case():
    """64 images, a hand-made pad_crop row each, and the existing CPU transforms applied by hand."""
    imgs = _images()
    rng = np.random.default_rng(1)
    plan = np.zeros((64, 5), dtype=np.int32)
    plan[:, :2] = rng.integers(-4, 5, size=(64, 2))
    plan[:4, :2] = [(-4, -4), (4, 4), (-4, 4), (0, 0)]
    plan[:, 2:4] = 32
    plan[:, 4] = np.arange(64) % 2
    to_t, norm = T.ToTensor(), T.Normalize(T.CIFAR_MEAN, T.CIFAR_STD)
    want = []
    for img, (x0, y0, _cw, _ch, flip) in zip(imgs, plan):
        a = np.pad(img, ((4, 4), (4, 4), (0, 0)))[y0 + 4:y0 + 36, x0 + 4:x0 + 36]
        if flip:
            a = a[:, ::-1]
        want.append(norm(to_t(a)))
    return torch.from_numpy(imgs), plan, torch.stack(want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("channels_last", [False, True])
def test_fallback_equals_the_cpu_transforms_bit_for_bit(pad_crop_case, dtype, channels_last):
    src, plan, want = pad_crop_case
    out = gpu_augment(src, plan, 32, T.CIFAR_MEAN, T.CIFAR_STD, dtype=dtype, channels_last=channels_last)
    assert out.shape == (64, 3, 32, 32) and out.dtype == dtype
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert out.is_contiguous(memory_format=fmt)
    assert torch.equal(out, want.to(dtype))


def test_identity_plan_equals_the_test_transform():
    imgs = _images(8, seed=3)
    tf = T.cifar_test_transform()
    want = torch.stack([tf(a) for a in imgs])
    plan = AugmentPlanner("identity", 32, 32).plan(8)
    assert (plan == np.array([0, 0, 32, 32, 0], dtype=np.int32)).all()
    out = gpu_augment(torch.from_numpy(imgs), plan, 32, T.CIFAR_MEAN, T.CIFAR_STD, dtype=torch.float32,
                      channels_last=False)
    assert torch.equal(out, want)
    with pytest.raises(ValueError):
        AugmentPlanner("identity", 224, 256)


def test_resize_follows_the_definition():
    """The composition's resize path against the formula of the definition, tap by tap, in fp64."""
    src = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(1, 9, 7, 3), dtype=np.uint8))
    x0, y0, cw, ch, H, W = -2, 3, 8, 9, 5, 6  # hangs over the left and the bottom edge
    mean, std = T.CIFAR_MEAN, T.CIFAR_STD
    m, s = torch.tensor(mean).double(), torch.tensor(std).double()
    for flip in (0, 1):
        plan = np.array([[x0, y0, cw, ch, flip]], dtype=np.int32)
        out = gpu_augment(src, plan, (H, W), mean, std, dtype=torch.float64, channels_last=False)[0]

        def px(y, x, c):
            return float(src[0, y, x, c]) if 0 <= y < 9 and 0 <= x < 7 else 0.0
        for dy in range(H):
            for dx in range(W):
                dxp = W - 1 - dx if flip else dx
                sx, sy = max(0.0, (dxp + 0.5) * cw / W - 0.5), max(0.0, (dy + 0.5) * ch / H - 0.5)
                xl, yl = int(math.floor(sx)), int(math.floor(sy))
                xh, yh, lx, ly = min(xl + 1, cw - 1), min(yl + 1, ch - 1), sx - xl, sy - yl
                for c in range(3):
                    v = ((1 - ly) * ((1 - lx) * px(y0 + yl, x0 + xl, c) + lx * px(y0 + yl, x0 + xh, c))
                         + ly * ((1 - lx) * px(y0 + yh, x0 + xl, c) + lx * px(y0 + yh, x0 + xh, c)))
                    want = (v / 255 - float(m[c])) / float(s[c])
                    assert abs(float(out[c, dy, dx]) - want) < 1e-12, (flip, dy, dx, c)


# ---------------------------------------------------------------- planner
def test_planner_is_seeded_by_seed_rank_epoch():
    def draws(seed=3, rank=0, epoch=0, mode="rrc"):
        p = AugmentPlanner(mode, 224, 256, seed=seed, rank=rank)
        p.set_epoch(epoch)
        return np.concatenate([p.plan(16), p.plan(16)])
    for mode in ("rrc", "pad_crop"):
        a = draws(mode=mode)
        assert a.dtype == np.int32 and a.shape == (32, 5)
        assert (a == draws(mode=mode)).all()
        assert not (a == draws(rank=1, mode=mode)).all()
        assert not (a == draws(epoch=1, mode=mode)).all()
        assert not (a == draws(seed=4, mode=mode)).all()
    p = AugmentPlanner("rrc", 224, 256, seed=3)
    p.set_epoch(2)
    first = p.plan(8)
    p.set_epoch(2)  # a resumed run
    assert (p.plan(8) == first).all()


def test_pad_crop_plans():
    p = AugmentPlanner("pad_crop", 32, 32, padding=4, seed=1).plan(10_000)
    assert (p[:, 2:4] == 32).all()
    for k in (0, 1):
        assert p[:, k].min() == -4 and p[:, k].max() == 4
    assert set(np.unique(p[:, 4])) == {0, 1}
    assert abs(p[:, 4].mean() - 0.5) <= 0.025  # five binomial sigmas of 10 000 draws
    q = AugmentPlanner("pad_crop", 24, 32, padding=2, seed=1).plan(10_000)  # a crop smaller than the image
    assert q[:, :2].min() == -2 and q[:, :2].max() == 32 - 24 + 2 and (q[:, 2:4] == 24).all()


def test_rrc_plans():
    S = 256
    p = AugmentPlanner("rrc", 224, S, seed=2).plan(10_000).astype(np.int64)
    x0, y0, cw, ch, flip = p.T
    assert (cw >= 1).all() and (ch >= 1).all()
    assert (x0 >= 0).all() and (y0 >= 0).all() and (x0 + cw <= S).all() and (y0 + ch <= S).all()
    # the integer sides are the real ones rounded: each within half a pixel
    area_lo, area_hi = (cw - 0.5) * (ch - 0.5) / S ** 2, (cw + 0.5) * (ch + 0.5) / S ** 2
    assert (area_hi >= 0.08).all() and (area_lo <= 1.0).all()
    assert ((cw + 0.5) / (ch - 0.5) >= 3 / 4).all() and ((cw - 0.5) / (ch + 0.5) <= 4 / 3).all()
    assert cw.min() < 100 and cw.max() > 200 and len(np.unique(x0)) > 100  # the draws spread
    assert abs(flip.mean() - 0.5) <= 0.025
    # no try fits (a scale above 1 never does): the centre square
    q = AugmentPlanner("rrc", 224, S, scale=(4.0, 5.0), seed=2).plan(4)
    assert (q[:, :4] == np.array([0, 0, S, S])).all()


def test_bad_plans_raise():
    src = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    good = np.array([[0, 0, 8, 8, 0], [1, -1, 4, 5, 1]], dtype=np.int32)
    gpu_augment(src, good, 8, T.CIFAR_MEAN, T.CIFAR_STD, dtype=torch.float32)
    gpu_augment(src, torch.from_numpy(good), 8, T.CIFAR_MEAN, T.CIFAR_STD, dtype=torch.float32)

    def bad(row, col, val):
        p = good.copy()
        p[row, col] = val
        return p
    for plan, msg in ((bad(1, 2, 0), "row 1"), (bad(0, 3, 0), "row 0"), (bad(1, 4, 2), "row 1"),
                      (bad(0, 0, 40_000), "row 0"), (bad(1, 2, 40_000), "row 1"),
                      (good[:1], "[2, 5]"), (good[:, :4], "[2, 5]"), (good.astype(np.int64), "int32")):
        with pytest.raises(ValueError, match=msg.replace("[", r"\[").replace("]", r"\]")):
            gpu_augment(src, plan, 8, T.CIFAR_MEAN, T.CIFAR_STD, dtype=torch.float32)
    with pytest.raises(ValueError):
        gpu_augment(src.float(), good, 8, T.CIFAR_MEAN, T.CIFAR_STD)
    with pytest.raises(ValueError):
        gpu_augment(src, good, 8, T.CIFAR_MEAN, (0.2, 0.0, 0.2))


def test_feature_is_registered_and_documented():
    from distributed_model_parallel_amd import _native
    assert "gpu_augment" in _native.FEATURES
    assert "gpu_augment.gpu_augment" in T.__doc__


# ---------------------------------------------------------------- data
def test_synthetic_uint8_images():
    ds = SyntheticImages(10, (3, 40, 24), 7, seed=2, uint8=True)
    x, y = ds[3]
    assert x.dtype == torch.uint8 and x.shape == (40, 24, 3) and 0 <= y < 7
    x2, y2 = SyntheticImages(10, (3, 40, 24), 7, seed=2, uint8=True)[3]
    assert torch.equal(x, x2) and y == y2
    assert not torch.equal(x, ds[4][0])
    assert len(torch.unique(x)) > 100  # the whole byte range, not a cast of randn
    f, _ = SyntheticImages(10, (3, 40, 24), 7, seed=2)[3]  # the default is untouched
    assert f.dtype == torch.float32 and f.shape == (3, 40, 24)


def test_staging_transforms():
    img = np.random.default_rng(0).integers(0, 256, size=(60, 90, 3), dtype=np.uint8)
    a = T.cifar_staging_transform()(img[:32, :32])
    assert a.dtype == torch.uint8 and a.shape == (32, 32, 3) and np.array_equal(a.numpy(), img[:32, :32])
    b = T.imagenet_train_staging_transform(48)(img)
    assert b.dtype == torch.uint8 and b.shape == (48, 48, 3)
    c = T.imagenet_val_staging_transform(28)(img)
    assert c.dtype == torch.uint8 and c.shape == (28, 28, 3)
    # the validation staging holds the very pixels the CPU validation transform normalises
    want = T.Compose([T.Resize(32), T.CenterCrop(28), T.ToTensor(), T.Normalize(T.IMAGENET_MEAN, T.IMAGENET_STD)])(img)
    got = gpu_augment(c[None], AugmentPlanner("identity", 28, 28).plan(1), 28, T.IMAGENET_MEAN, T.IMAGENET_STD,
                      dtype=torch.float32, channels_last=False)[0]
    assert torch.equal(got, want)


def test_cifar_loader_end_to_end(tmp_path):
    """A 16-image cifar-10-batches-bin: the staging loader + gpu_augment(identity) = the test-transform loader."""
    rng = np.random.default_rng(7)
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    raw = np.concatenate([rng.integers(0, 10, size=(16, 1), dtype=np.uint8),
                          rng.integers(0, 256, size=(16, 3072), dtype=np.uint8)], axis=1)
    raw.tofile(d / "test_batch.bin")
    from torch.utils.data import DataLoader
    staged = DataLoader(CIFAR10(str(tmp_path), False, T.cifar_staging_transform()), batch_size=8)
    plain = DataLoader(CIFAR10(str(tmp_path), False, T.cifar_test_transform()), batch_size=8)
    planner = AugmentPlanner("identity", 32, 32)
    n = 0
    for (xb, yb), (xr, yr) in zip(staged, plain):
        assert xb.dtype == torch.uint8 and xb.shape == (8, 32, 32, 3)
        out = gpu_augment(xb, planner.plan(xb.shape[0]), 32, T.CIFAR_MEAN, T.CIFAR_STD, dtype=torch.float32,
                          channels_last=False)
        assert torch.equal(out, xr) and torch.equal(yb, yr)
        n += xb.shape[0]
    assert n == 16


# ---------------------------------------------------------------- CLI
def test_cli_flag_and_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import _augment_geometry, build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert a.gpu_augment is False and a.augment_staging is None
    a = p.parse_args(["--gpu-augment", "--arch", "resnet50", "-type", "Imagenet", "--synthetic"])
    check_args(p, a)
    assert _augment_geometry(a) == (False, 224, 256)
    a = p.parse_args(["--gpu-augment", "--arch", "vit_b_16", "--image-size", "384", "--synthetic"])
    check_args(p, a)
    assert _augment_geometry(a) == (False, 384, 439)
    a = p.parse_args(["--gpu-augment", "--arch", "resnet50", "-type", "Imagenet", "--synthetic", "--augment-staging", "300"])
    check_args(p, a)
    assert _augment_geometry(a) == (False, 224, 300)
    a = p.parse_args(["--gpu-augment", "--arch", "mobilenetv2", "--synthetic"])
    check_args(p, a)
    assert _augment_geometry(a) == (True, 32, 32)
    for argv, msg in ((["--gpu-augment", "--parallel", "pipe"], "--gpu-augment with --parallel pipe"),
                      (["--augment-staging", "256"], "needs --gpu-augment"),
                      (["--gpu-augment", "--augment-staging", "0"], "[1, 16384]")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def _cli(tmp_path, *extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(31000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    return subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--arch", "mobilenetv2",
                           "--synthetic", "-b", "8", "--epochs", "1", "--steps-per-epoch", "2", "--lr", "0.05",
                           "--warmup-epochs", "0", "--log-dir", str(tmp_path / "log"), "-j", "0",
                           "--checkpoint", str(tmp_path / "ck.pth"), "--gpu-augment", *extra],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def test_cli_trains_with_gpu_augment(tmp_path):
    r = _cli(tmp_path, "--parallel", "none")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()
    assert len(lines) == 1
    rec = dict(f.split(":", 1) for f in lines[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, lines[0]
    assert math.isfinite(float(rec["loss_val"])), lines[0]


def test_cli_refuses_gpu_augment_with_pipe(tmp_path):
    r = _cli(tmp_path, "--parallel", "pipe")
    assert r.returncode != 0
    assert "--gpu-augment with --parallel pipe is not supported" in r.stderr
