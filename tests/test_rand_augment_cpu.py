"""RandAugment, the CPU side (data/rand_augment.py): the PyTorch composition of every op against
PIL (the colour ops bit for bit, the affine ops up to PIL's fixed-point coordinates), the level
functions, the host-drawn plan, the spec parser, the byte crop's oracle and the CLI flag."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd.data import AugmentPlanner, gpu_augment, transforms as T
from distributed_model_parallel_amd.data import rand_augment as RA
from distributed_model_parallel_amd.data.gpu_augment import norm_table

try:
    from PIL import Image, ImageEnhance, ImageOps
except ImportError:  # pragma: no cover
    Image = None
needs_pil = pytest.mark.skipif(Image is None, reason="PIL is not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (124, 116, 104)
FACTORS = (0.1, 0.19, 0.55, 1.0, 1.37, 1.81, 1.9)
C = RA.CODE


def _images():
    rng = np.random.default_rng(0)
    const_chan = rng.integers(0, 256, size=(13, 17, 3), dtype=np.uint8)
    const_chan[..., 1] = 77
    return {"random 13 x 17": rng.integers(0, 256, size=(13, 17, 3), dtype=np.uint8),
            "values 100..103": rng.integers(100, 104, size=(13, 17, 3), dtype=np.uint8),
            "constant channel": const_chan,
            "constant": np.full((13, 17, 3), 93, dtype=np.uint8),
            "5 x 7": rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)}


IMAGES = _images()


def _op(a: np.ndarray, name: str, *arg) -> np.ndarray:
    row = list(arg) + [0.0] * (6 - len(arg))
    return RA.apply_op(torch.from_numpy(a), C[name], row, FILL).numpy()


def _solarize_add(img, add):
    lut = [min(255, i + add) if i < 128 else i for i in range(256)]
    return img.point(lut * 3)


@needs_pil
@pytest.mark.parametrize("case", list(IMAGES))
def test_colour_ops_equal_pil_bit_for_bit(case):
    a = IMAGES[case]
    img = Image.fromarray(a)
    assert np.array_equal(_op(a, "AutoContrast"), np.asarray(ImageOps.autocontrast(img)))
    assert np.array_equal(_op(a, "Equalize"), np.asarray(ImageOps.equalize(img)))
    assert np.array_equal(_op(a, "Invert"), np.asarray(ImageOps.invert(img)))
    for bits in range(5):
        assert np.array_equal(_op(a, "PosterizeIncreasing", bits), np.asarray(ImageOps.posterize(img, bits))), bits
    for t in (0, 26, 128, 256):
        assert np.array_equal(_op(a, "SolarizeIncreasing", t), np.asarray(ImageOps.solarize(img, t))), t
    for add in (0, 99, 110):
        assert np.array_equal(_op(a, "SolarizeAdd", add), np.asarray(_solarize_add(img, add))), add
    for f in FACTORS:
        for name, enh in (("BrightnessIncreasing", ImageEnhance.Brightness), ("ContrastIncreasing", ImageEnhance.Contrast),
                          ("ColorIncreasing", ImageEnhance.Color), ("SharpnessIncreasing", ImageEnhance.Sharpness)):
            assert np.array_equal(_op(a, name, f), np.asarray(enh(img).enhance(f))), (name, f)
    if case in ("constant", "5 x 7"):  # one level per channel / Equalize's step == 0: the identity
        assert np.array_equal(_op(a, "Equalize"), a)
    if case == "constant":
        assert np.array_equal(_op(a, "AutoContrast"), a)


def test_autocontrast_table_for_every_pair():
    """PIL's ImageOps.autocontrast formula, int(ix * scale + offset) clipped, for every (lo, hi)."""
    v = np.arange(256, dtype=np.float64)
    assert RA.autocontrast_table(7, 7).tolist() == list(range(256))
    for lo in range(255):
        for hi in range(lo + 1, 256):
            scale = 255.0 / (hi - lo)
            want = np.clip(np.trunc(v * scale + (-lo * scale)), 0, 255).astype(np.uint8)
            assert np.array_equal(RA.autocontrast_table(lo, hi).numpy(), want), (lo, hi)


@needs_pil
@pytest.mark.parametrize("hw", [(33, 47), (224, 224)])
def test_affine_ops_against_pil_nearest(hw):
    """At most 0.5 % of the pixels differ (PIL's 16.16 fixed-point coordinates; the definition alone
    measured at most 0.12 %): the cap catches a wrong matrix or an off-by-half."""
    H, W = hw
    rng = np.random.default_rng(H)
    a = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    img = Image.fromarray(a)
    kw = dict(resample=Image.NEAREST, fillcolor=FILL)
    for trial in range(6):
        mag, sign = float(rng.uniform(1.0, 10.0)), float(rng.choice([-1.0, 1.0]))
        for name in ("ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "Rotate"):
            m = RA.op_argument(C[name], mag, sign, H, W)
            got = _op(a, name, *m)
            if name == "Rotate":
                want = img.rotate(sign * mag / 10 * 30.0, **kw)
            else:
                want = img.transform(img.size, Image.AFFINE, m, **kw)
            differ = (got != np.asarray(want)).any(-1).mean()
            print(f"{name} {H}x{W} magnitude {mag:.2f} sign {sign:+.0f}: {100 * differ:.3f} % differ")
            assert differ <= 0.005, (name, mag, sign, differ)
            assert (got != a).any()  # the op did something


def test_level_functions():
    H, W = 200, 300
    arg = lambda name, m, s=1.0: RA.op_argument(C[name], m, s, H, W)  # noqa: E731
    # magnitude 0: every op is (nearly) the identity
    assert arg("Rotate", 0.0) == pytest.approx((1, 0, 0, 0, 1, 0))
    assert arg("ShearX", 0.0) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0) and arg("TranslateYRel", 0.0)[5] == 0.0
    assert arg("PosterizeIncreasing", 0.0)[0] == 4 and arg("SolarizeIncreasing", 0.0)[0] == 256
    assert arg("SolarizeAdd", 0.0)[0] == 0 and arg("ColorIncreasing", 0.0)[0] == 1.0
    # magnitude 9
    rad = math.radians(27.0)
    m = arg("Rotate", 9.0)
    assert (m[0], m[1], m[3], m[4]) == pytest.approx((math.cos(rad), -math.sin(rad), math.sin(rad), math.cos(rad)))
    assert arg("Rotate", 9.0, -1.0)[1] == pytest.approx(math.sin(rad))
    # the centre maps to itself
    assert m[0] * 150 + m[1] * 100 + m[2] == pytest.approx(150) and m[3] * 150 + m[4] * 100 + m[5] == pytest.approx(100)
    assert arg("ShearX", 9.0)[1] == pytest.approx(0.27) and arg("ShearY", 9.0, -1.0)[3] == pytest.approx(-0.27)
    assert arg("TranslateXRel", 9.0)[2] == pytest.approx(0.405 * W)
    assert arg("TranslateYRel", 9.0, -1.0)[5] == pytest.approx(-0.405 * H)
    assert arg("PosterizeIncreasing", 9.0)[0] == 1 and arg("PosterizeIncreasing", 10.0)[0] == 0
    assert arg("SolarizeIncreasing", 9.0)[0] == 26 and arg("SolarizeIncreasing", 10.0)[0] == 0
    assert arg("SolarizeAdd", 9.0)[0] == 99
    for name in ("BrightnessIncreasing", "ContrastIncreasing", "ColorIncreasing", "SharpnessIncreasing"):
        assert arg(name, 9.0)[0] == pytest.approx(1.81) and arg(name, 9.0, -1.0)[0] == pytest.approx(0.19)
        assert arg(name, 10.0, -1.0)[0] == 0.1 and arg(name, 10.0)[0] == pytest.approx(1.9)
    assert RA.fill_from_mean(T.IMAGENET_MEAN) == FILL


# ---------------------------------------------------------------- planner
def _plans(seed=3, rank=0, epoch=0):
    p = RA.RandAugmentPlanner(seed=seed, rank=rank)
    p.set_epoch(epoch)
    a, b = p.plan(16, 32, 32), p.plan(16, 32, 32)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def test_planner_is_seeded_by_seed_rank_epoch():
    codes, args = _plans()
    assert codes.dtype == np.int32 and codes.shape == (32, 2)
    assert args.dtype == np.float64 and args.shape == (32, 2, 6)
    again = _plans()
    assert np.array_equal(codes, again[0]) and np.array_equal(args, again[1])
    for other in (_plans(rank=1), _plans(epoch=1), _plans(seed=4)):
        assert not np.array_equal(codes, other[0])
    assert ((codes >= 0) & (codes <= RA.NOT_APPLIED)).all() and np.isfinite(args).all()
    assert (args[codes == RA.NOT_APPLIED] == 0).all()
    RA._check_ops((codes, args), 32)  # every drawn plan passes the host check


def test_augment_planner_draws_do_not_change():
    """RandAugment draws from a stream of its own: the crop plans of a seed are what they were."""
    plain = AugmentPlanner("rrc", 224, 256, seed=5, rank=1)
    mixed = AugmentPlanner("rrc", 224, 256, seed=5, rank=1)
    rand = RA.RandAugmentPlanner(seed=5, rank=1)
    for epoch in (0, 3):
        for p in (plain, mixed, rand):
            p.set_epoch(epoch)
        for _ in range(3):
            want = plain.plan(8)
            rand.plan(8, 224, 224)
            assert np.array_equal(mixed.plan(8), want)
    # and its stream is no copy of the crop planner's
    crop_stream = np.random.default_rng([5, 1, 0]).integers(0, 15, size=(8, 2))
    rand.set_epoch(0)
    assert not np.array_equal(rand.rng.integers(0, 15, size=(8, 2)), crop_stream)


def test_planner_statistics():
    """30000 draws: each op's frequency and the applied share within 6 binomial standard deviations."""
    n = 30000
    codes, _ = RA.RandAugmentPlanner(prob=1.0, seed=1).plan(n // 2, 32, 32)
    sd = math.sqrt((1 / 15) * (14 / 15) / n)
    for k in range(15):
        assert abs((codes == k).mean() - 1 / 15) <= 6 * sd, k
    codes, args = RA.RandAugmentPlanner(seed=2).plan(n // 2, 32, 32)
    applied = codes != RA.NOT_APPLIED
    assert abs(applied.mean() - 0.5) <= 6 * math.sqrt(0.25 / n)
    q = 0.5 / 15
    for k in range(15):
        assert abs((codes == k).mean() - q) <= 6 * math.sqrt(q * (1 - q) / n), k
    # the magnitude spreads (mstd 0.5 about 9, clipped at 10) and both signs occur
    f = args[codes == C["BrightnessIncreasing"]][:, 0]
    assert len(np.unique(f)) > 50 and (f < 1).any() and (f > 1).any() and f.max() <= 1.9 and f.min() >= 0.1
    fixed = RA.RandAugmentPlanner(magnitude_std=0.0, prob=1.0, seed=2).plan(2000, 32, 32)
    assert set(np.unique(fixed[1][fixed[0] == C["SolarizeAdd"]][:, 0])) == {99.0}


# ---------------------------------------------------------------- spec parser
def test_parse_rand_augment():
    assert RA.parse_rand_augment("rand-m9-mstd0.5-inc1") == dict(num_ops=2, magnitude=9.0, magnitude_std=0.5, prob=0.5)
    assert RA.parse_rand_augment("rand-m7-n3-mstd0-p0.7-inc1") == dict(num_ops=3, magnitude=7.0, magnitude_std=0.0,
                                                                      prob=0.7)
    assert RA.parse_rand_augment("rand-inc1-m9.5")["magnitude"] == 9.5
    RA.RandAugmentPlanner(**RA.parse_rand_augment("rand-m9-mstd0.5-inc1"))
    for spec, word in (("rand-m9-mstd0.5", "inc1"), ("rand-m9-inc0", "'inc'"), ("rand-m9-mstd100-inc1", "'mstd'"),
                       ("rand-m9-mmax10-inc1", "'mmax'"), ("rand-m9-w0-inc1", "'w'"), ("rand-m9-t0.3-inc1", "'t'"),
                       ("rand-m9-zz3-inc1", "'zz'"), ("rand-m11-inc1", "'m'"), ("rand-m9-n0-inc1", "'n'"),
                       ("rand-m9-p2-inc1", "'p'"), ("rand-m9-inc", "'inc'"), ("augmix-m9-inc1", "rand-"),
                       ("rand", "rand-")):
        with pytest.raises(ValueError, match=word):
            RA.parse_rand_augment(spec)


# ---------------------------------------------------------------- byte crop and the chain
def test_byte_crop_oracle_against_interpolate():
    src = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(6, 37, 53, 3), dtype=np.uint8))
    plan = np.array([[0, 0, 53, 37, 0], [0, 0, 53, 37, 1], [-3, -3, 59, 43, 0], [48, 30, 5, 7, 1],
                     [20, 10, 1, 1, 0], [2, 3, 24, 16, 1]], dtype=np.int32)
    H, W = 16, 24
    got = RA.crop_bytes(src, plan, (H, W))
    assert got.dtype == torch.uint8 and got.shape == (6, H, W, 3)
    for i, (x0, y0, cw, ch, flip) in enumerate(plan.tolist()):
        padded = F.pad(src[i].permute(2, 0, 1), (64, 64, 64, 64))[:, y0 + 64:y0 + 64 + ch, x0 + 64:x0 + 64 + cw]
        if (cw, ch) == (W, H):
            want = padded.flip(2) if flip else padded
            assert torch.equal(got[i].permute(2, 0, 1), want)  # no resize: a copy
            continue
        ref = F.interpolate(padded[None].float(), size=(H, W), mode="bilinear", align_corners=False, antialias=False)[0]
        if flip:
            ref = ref.flip(2)
        err = float((got[i].permute(2, 0, 1).float() - ref).abs().max())
        print(f"row {i}: max |bytes - F.interpolate| = {err:.4f}")
        assert err <= 0.501, (i, err)


def test_gpu_augment_with_ops_is_crop_then_ops_then_table():
    rng = np.random.default_rng(9)
    src = torch.from_numpy(rng.integers(0, 256, size=(4, 20, 20, 3), dtype=np.uint8))
    plan = np.array([[0, 0, 20, 20, 0], [2, 1, 16, 16, 1], [-2, -2, 16, 16, 0], [3, 3, 9, 11, 1]], dtype=np.int32)
    codes = np.array([[C["Rotate"], C["Equalize"]], [C["ColorIncreasing"], RA.NOT_APPLIED],
                      [C["AutoContrast"], C["ShearX"]], [RA.NOT_APPLIED, C["SharpnessIncreasing"]]], dtype=np.int32)
    args = np.zeros((4, 2, 6))
    for i in range(4):
        for k in range(2):
            if codes[i, k] != RA.NOT_APPLIED:
                args[i, k] = RA.op_argument(int(codes[i, k]), 9.0, -1.0 if i % 2 else 1.0, 16, 16)
    mean, std = T.IMAGENET_MEAN, T.IMAGENET_STD
    out = gpu_augment(src, plan, 16, mean, std, dtype=torch.float32, channels_last=False, ops=(codes, args))
    crop = RA.crop_bytes(src, plan, 16)
    tab = norm_table(mean, std)
    for i in range(4):
        img = RA.apply_op(RA.apply_op(crop[i], codes[i, 0], args[i, 0], FILL), codes[i, 1], args[i, 1], FILL)
        want = torch.stack([tab[c][img[..., c].long()] for c in range(3)])
        assert torch.equal(out[i], want), i
    norm = T.Normalize(mean, std)
    assert torch.equal(out[1], norm(T.ToTensor()(RA.apply_op(crop[1], codes[1, 0], args[1, 0], FILL).numpy())))
    cl = gpu_augment(src, plan, 16, mean, std, dtype=torch.bfloat16, ops=(codes, args))
    assert cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl, out.to(torch.bfloat16))
    with pytest.raises(ValueError, match="C == 3"):
        gpu_augment(src[..., :1].contiguous(), plan, 16, mean[:1], std[:1], ops=(codes, args))
    for bad_codes, bad_args in ((codes + 20, args), (codes, np.full_like(args, np.nan)), (codes.astype(np.int64), args),
                                (codes, args[:, :1])):
        with pytest.raises(ValueError, match="rand_augment"):
            gpu_augment(src, plan, 16, mean, std, ops=(bad_codes, bad_args))


def test_feature_is_registered():
    from distributed_model_parallel_amd import _native
    assert "rand_augment" in _native.FEATURES
    assert "PosterizeIncreasing" in RA.__doc__ and "blend(d, v, f)" in RA.__doc__


# ---------------------------------------------------------------- CLI
def test_cli_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args(["--gpu-augment", "--rand-augment", "rand-m9-mstd0.5-inc1"])
    check_args(p, a)
    assert a.rand_augment == "rand-m9-mstd0.5-inc1" and p.parse_args([]).rand_augment is None
    for argv, msg in ((["--rand-augment", "rand-m9-mstd0.5-inc1"], "--rand-augment needs --gpu-augment"),
                      (["--gpu-augment", "--rand-augment", "rand-m9-mstd0.5"], "inc1"),
                      (["--gpu-augment", "--rand-augment", "rand-m9-w0-inc1"], "'w'")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_cli_trains_with_rand_augment(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(32000 + os.getpid() % 1000), PYTHONPATH=ROOT,
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--arch", "mobilenetv2",
                        "--synthetic", "-b", "8", "--epochs", "1", "--steps-per-epoch", "2", "--lr", "0.05",
                        "--warmup-epochs", "0", "--log-dir", str(tmp_path / "log"), "-j", "0", "--parallel", "none",
                        "--checkpoint", str(tmp_path / "ck.pth"), "--gpu-augment", "--rand-augment",
                        "rand-m9-mstd0.5-inc1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()
    assert len(lines) == 1
    rec = dict(f.split(":", 1) for f in lines[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, lines[0]
    assert math.isfinite(float(rec["loss_val"])), lines[0]
