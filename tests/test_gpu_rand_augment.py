"""RandAugment kernels (csrc/data/rand_augment.hip) against the PyTorch composition of
data/rand_augment.py on CPU copies, bit for bit (torch.equal), bf16 and fp32, both layouts."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.data import AugmentPlanner, gpu_augment, transforms as T

pytestmark = pytest.mark.gpu

RA = importlib.import_module("distributed_model_parallel_amd.data.rand_augment")
MEAN, STD = T.IMAGENET_MEAN, T.IMAGENET_STD
C = RA.CODE
VARIANTS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)]


def _u8(shape, seed, lo=0, hi=256):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, size=shape, dtype=np.uint8))


def _check(u8, codes, args):
    """One fp32 oracle on the CPU; every dtype / layout of the kernels equals it (rounded once to the dtype)."""
    codes, args = np.ascontiguousarray(codes, dtype=np.int32), np.ascontiguousarray(args, dtype=np.float64)
    want = RA.rand_augment_bytes(u8, (codes, args), MEAN, STD, dtype=torch.float32, channels_last=False)
    dev = u8.cuda()
    before = dict(RA._STATS)
    for dtype, cl in VARIANTS:
        got = RA.rand_augment_bytes(dev, (codes, args), MEAN, STD, dtype=dtype, channels_last=cl)
        assert got.dtype == dtype and got.shape == want.shape
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        same = got.cpu() == want.to(dtype)
        if not bool(same.all()):
            bad = (~same).flatten(1).any(1).nonzero().flatten().tolist()
            raise AssertionError(f"{dtype} channels_last={cl}: samples {bad[:10]} differ; ops {codes[bad[:10]].tolist()}")
    assert RA._STATS["native"] == before["native"] + len(VARIANTS)
    assert torch.equal(dev.cpu(), u8)  # the input is never written
    return want


def _every_op(H, W, magnitudes=(9.0, 3.3)):
    """One sample per (op, sign, magnitude), a single slot."""
    rows = [(k, RA.op_argument(k, m, s, H, W)) for k in range(15) for s in (1.0, -1.0) for m in magnitudes]
    rows.append((RA.NOT_APPLIED, (0.0,) * 6))
    return np.array([[r[0]] for r in rows], dtype=np.int32), np.array([[r[1]] for r in rows], dtype=np.float64)


@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (3, 3), (1, 1), (1, 9)])
def test_every_op_alone(hw):
    """5 x 7: 105 elements, scalar stores; 8 x 8: vector stores; 3 x 3: one interior pixel; 1 x 1 and
    1 x 9: Sharpness all border, affine mostly fill."""
    H, W = hw
    codes, args = _every_op(H, W)
    u8 = _u8((len(codes), H, W, 3), seed=H * 16 + W)
    want = _check(u8, codes, args)
    ident = RA.rand_augment_bytes(u8, (np.full_like(codes, RA.NOT_APPLIED), np.zeros_like(args)), MEAN, STD,
                                  dtype=torch.float32, channels_last=False)
    assert torch.equal(want[-1], ident[-1])
    if (H, W) == (8, 8):
        assert sum(not torch.equal(want[i], ident[i]) for i in range(len(codes))) >= len(codes) // 2  # ops do something


def test_all_ordered_pairs():
    """225 samples at 8 x 8, one per ordered op pair: the second op's statistic sees the first one's fill or table."""
    pairs = [(a, b) for a in range(15) for b in range(15)]
    rng = np.random.default_rng(2)
    codes = np.array(pairs, dtype=np.int32)
    args = np.array([[RA.op_argument(k, float(rng.uniform(5, 10)), float(rng.choice([-1.0, 1.0])), 8, 8) for k in p]
                     for p in pairs])
    _check(_u8((225, 8, 8, 3), seed=3, lo=20, hi=230), codes, args)


def test_several_blocks_feed_one_histogram():
    H = W = 224
    codes = np.array([[C["Rotate"], C["Equalize"]], [C["AutoContrast"], C["ContrastIncreasing"]]], dtype=np.int32)
    args = np.array([[RA.op_argument(int(k), 9.0, s, H, W) for k in row] for row, s in zip(codes, (1.0, -1.0))])
    _check(_u8((2, H, W, 3), seed=4, lo=30, hi=200), codes, args)
    codes = np.array([[C["Equalize"], C["SharpnessIncreasing"], C["ColorIncreasing"]],
                      [C["ShearX"], C["AutoContrast"], C["TranslateYRel"]]], dtype=np.int32)  # three slots: both stagings
    args = np.array([[RA.op_argument(int(k), 8.0, s, H, W) for k in row] for row, s in zip(codes, (-1.0, 1.0))])
    _check(_u8((2, H, W, 3), seed=5, lo=30, hi=200), codes, args)


def test_autocontrast_every_span():
    """255 samples of 16 x 16, one per span hi - lo = 1..255, each holding every level of its range."""
    rng = np.random.default_rng(6)
    u8 = np.empty((255, 256, 3), dtype=np.uint8)
    for d in range(1, 256):
        for c in range(3):
            lo = int(rng.integers(0, 256 - d))
            u8[d - 1, :, c] = rng.permutation(lo + np.arange(256) % (d + 1))
    codes = np.full((255, 1), C["AutoContrast"], dtype=np.int32)
    _check(torch.from_numpy(u8.reshape(255, 16, 16, 3)), codes, np.zeros((255, 1, 6)))


def test_equalize_and_a_constant_image():
    eq = np.full((3, 1), C["Equalize"], dtype=np.int32)
    _check(_u8((3, 16, 16, 3), seed=7), eq, np.zeros((3, 1, 6)))          # step >= 1
    _check(_u8((3, 16, 16, 3), seed=8, lo=100, hi=104), eq, np.zeros((3, 1, 6)))
    _check(_u8((3, 5, 7, 3), seed=9), eq, np.zeros((3, 1, 6)))            # step == 0: identity
    codes, args = _every_op(8, 8, magnitudes=(9.0,))
    _check(torch.full((len(codes), 8, 8, 3), 93, dtype=torch.uint8), codes, args)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_applied_and_not_applied_rows(n):
    codes, args = RA.RandAugmentPlanner(num_ops=n, seed=n).plan(96, 8, 8)
    assert (codes == RA.NOT_APPLIED).any() and (codes != RA.NOT_APPLIED).any()
    _check(_u8((96, 8, 8, 3), seed=10 + n), codes, args)


def test_batch_grid_stride_wraps():
    """2049 samples against at most 2048 blocks in y: the batch loop of every kernel takes a second lap."""
    codes, args = RA.RandAugmentPlanner(prob=0.9, seed=11).plan(2049, 4, 4)
    codes[-1], args[-1] = (C["Equalize"], C["AutoContrast"]), 0.0  # the wrapped sample needs its histograms
    _check(_u8((2049, 4, 4, 3), seed=12), codes, args)


def test_byte_crop():
    src = _u8((8, 37, 53, 3), seed=13)
    resize = np.array([[0, 0, 53, 37, 0], [0, 0, 53, 37, 1], [-3, -3, 59, 43, 0], [-3, -3, 59, 43, 1], [48, 30, 5, 7, 1],
                       [20, 10, 1, 1, 0], [2, 3, 24, 16, 1], [-30, -20, 24, 16, 0]], dtype=np.int32)  # last two: copies
    copy = np.array([[x0, y0, 24, 16, i % 2] for i, (x0, y0) in enumerate(
        [(0, 0), (29, 21), (-5, -4), (40, 30), (-24, 0), (53, 37), (10, -15), (30, 36)])], dtype=np.int32)
    for plan in (resize, copy):
        want = RA.crop_bytes(src, plan, (16, 24))
        got = RA.crop_bytes(src.cuda(), plan, (16, 24))
        assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got.cpu(), want)
    rrc = AugmentPlanner("rrc", 224, 256, seed=3).plan(2)
    big = _u8((2, 256, 256, 3), seed=14)
    assert torch.equal(RA.crop_bytes(big.cuda(), rrc, 224).cpu(), RA.crop_bytes(big, rrc, 224))


def test_gpu_augment_with_ops_end_to_end():
    src = _u8((6, 40, 40, 3), seed=15)
    plan = AugmentPlanner("rrc", 32, 40, seed=4).plan(6)
    ops = RA.RandAugmentPlanner(prob=1.0, seed=5).plan(6, 32, 32)
    want = gpu_augment(src, plan, 32, MEAN, STD, dtype=torch.float32, channels_last=False, ops=ops)
    for dtype, cl in VARIANTS:
        got = gpu_augment(src.cuda(), plan, 32, MEAN, STD, dtype=dtype, channels_last=cl, ops=ops)
        assert torch.equal(got.cpu(), want.to(dtype))


@pytest.mark.parametrize("dtype,channels_last", VARIANTS)
def test_raw_entry_point_marks_a_bad_sample(dtype, channels_last):
    """An op code outside the table or a NaN matrix: that sample reads nothing and comes out NaN; the
    others are exact."""
    N = _native.require("test")
    H, W = 8, 8
    u8 = _u8((5, H, W, 3), seed=16)
    codes = np.array([[C["Rotate"], C["Equalize"]]] * 5, dtype=np.int32)
    args = np.array([[RA.op_argument(int(k), 9.0, 1.0, H, W) for k in row] for row in codes])
    want = RA.rand_augment_bytes(u8, (codes, args), MEAN, STD, dtype=dtype, channels_last=False)
    codes[1, 0], codes[3, 1] = 99, -1
    args[2, 0, 4] = np.nan
    args[4, 1, 5] = np.inf  # an argument the op does not use counts too
    table = RA._device_table(MEAN, STD, torch.device("cuda", torch.cuda.current_device()))
    got = N.rand_augment_apply(u8.cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(args).cuda(), [0, 1],
                               [124, 116, 104], table, dtype, channels_last).cpu()
    assert torch.equal(got[0], want[0])
    for i in (1, 2, 3, 4):
        assert bool(torch.isnan(got[i]).all()), i


def test_host_checks():
    N = _native.require("test")
    u8 = _u8((2, 4, 4, 3), seed=17).cuda()
    codes = torch.zeros(2, 1, dtype=torch.int32, device="cuda")
    args = torch.zeros(2, 1, 6, dtype=torch.float64, device="cuda")
    table = RA._device_table(MEAN, STD, u8.device)
    N.rand_augment_apply(u8, codes, args, [1], [0, 0, 0], table, torch.float32, True)
    for bad in (lambda: N.rand_augment_apply(u8.cpu(), codes, args, [1], [0, 0, 0], table, torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes.long(), args, [1], [0, 0, 0], table, torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes, args.float(), [1], [0, 0, 0], table, torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes, args[:, :, :5].contiguous(), [1], [0, 0, 0], table, torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes, args, [1, 0], [0, 0, 0], table, torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes, args, [1], [0, 0, 256], table, torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes, args, [1], [0, 0, 0], table[:2].contiguous(), torch.float32, True),
                lambda: N.rand_augment_apply(u8, codes, args, [1], [0, 0, 0], table, torch.float16, True),
                lambda: N.crop_bytes(u8, torch.zeros(2, 4, dtype=torch.int32, device="cuda"), 4, 4),
                lambda: N.crop_bytes(u8[..., :2].contiguous(), torch.zeros(2, 5, dtype=torch.int32, device="cuda"), 4, 4)):
        with pytest.raises(RuntimeError):
            bad()


_CHILD = r"""
import importlib, numpy as np, torch
from distributed_model_parallel_amd.data import AugmentPlanner, gpu_augment, transforms as T
RA = importlib.import_module("distributed_model_parallel_amd.data.rand_augment")
src = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(4, 20, 20, 3), dtype=np.uint8))
plan = AugmentPlanner("rrc", 16, 20, seed=1).plan(4)
ops = RA.RandAugmentPlanner(prob=1.0, seed=2).plan(4, 16, 16)
want = gpu_augment(src, plan, 16, T.IMAGENET_MEAN, T.IMAGENET_STD, dtype=torch.float32, ops=ops)
before = dict(RA._STATS)
got = gpu_augment(src.cuda(), plan, 16, T.IMAGENET_MEAN, T.IMAGENET_STD, dtype=torch.float32, ops=ops)
assert got.is_cuda and torch.equal(got.cpu(), want)
print("ROUTE", RA._STATS["native"] - before["native"], RA._STATS["torch"] - before["torch"])
"""


def test_disable_feature_in_child_process():
    """DMP_DISABLE=rand_augment: the PyTorch composition, the same bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DMP_DISABLE="rand_augment")
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROUTE")][-1].split()
    assert line == ["ROUTE", "0", "2"], line  # the byte crop and the chain, both on the torch path
