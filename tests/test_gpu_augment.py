"""The augmentation kernel (csrc/data/augment.hip) against the PyTorch composition of
data/gpu_augment.py run on CPU copies: bit for bit without a resize, within twice
the fp32 composition's own error against fp64 with one."""
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

GA = importlib.import_module("distributed_model_parallel_amd.data.gpu_augment")  # the module (its _STATS)
MEANS = {1: ((0.45,), (0.225,)), 3: (T.IMAGENET_MEAN, T.IMAGENET_STD), 4: ((0.485, 0.456, 0.406, 0.5),
                                                                          (0.229, 0.224, 0.225, 0.25))}
DTYPES = [torch.bfloat16, torch.float32]
LAYOUTS = [True, False]


def _src(shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8))


def _plan(B, H, W, seed=0, reach=4):
    """No-resize rows: offsets in [-reach, reach], both flip values."""
    rng = np.random.default_rng(seed)
    p = np.zeros((B, 5), dtype=np.int32)
    p[:, :2] = rng.integers(-reach, reach + 1, size=(B, 2))
    p[:, 2], p[:, 3] = W, H
    p[:, 4] = np.arange(B) % 2
    return p


def _check_exact(src, plan, size, dtype, channels_last, dev_src=None):
    C = src.shape[3]
    mean, std = MEANS[C]
    want = gpu_augment(src, plan, size, mean, std, dtype=dtype, channels_last=channels_last)  # CPU composition
    before = dict(GA._STATS)
    out = gpu_augment(src.cuda() if dev_src is None else dev_src, plan, size, mean, std, dtype=dtype,
                      channels_last=channels_last)
    assert GA._STATS["native"] == before["native"] + 1 and GA._STATS["torch"] == before["torch"]
    assert out.is_cuda and out.dtype == dtype and out.shape == want.shape
    assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert torch.equal(out.cpu(), want)
    if bool(((plan[:, 2] == out.shape[3]) & (plan[:, 3] == out.shape[2])).all()):
        # the wrapper took the crop-only instantiation: the same rows through the one that can resize too
        N = _native.require("test")
        dev = src.cuda() if dev_src is None else dev_src
        both = N.augment_batch(dev, torch.from_numpy(plan).cuda(), out.shape[2], out.shape[3], list(mean), list(std),
                               dtype, channels_last, False)
        assert torch.equal(both.cpu(), want)


# ---------------------------------------------------------------- no resize: bit for bit
@pytest.mark.parametrize("channels_last", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 11, 13, 3),   # 429 elements: no multiple of the vector, the scalar kernel
                                   (3, 8, 8, 3),     # the vector kernel
                                   (2, 8, 8, 1), (2, 8, 8, 4),
                                   (2, 6, 20, 3)],   # rows shorter than a vector lap, H != W
                         ids=lambda s: "x".join(map(str, s)))
def test_crop_is_bit_exact(shape, dtype, channels_last):
    B, H, W, _ = shape
    _check_exact(_src(shape, seed=H), _plan(B, H, W, seed=W, reach=2), (H, W), dtype, channels_last)


@pytest.mark.parametrize("channels_last", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pad_crop_offsets_and_flips(dtype, channels_last):
    src = _src((4, 32, 32, 3), seed=1)
    for flip in (0, 1):
        plan = np.array([[-4, -4, 32, 32, flip], [4, 4, 32, 32, flip], [-4, 4, 32, 32, flip], [0, 0, 32, 32, flip]],
                        dtype=np.int32)
        _check_exact(src, plan, 32, dtype, channels_last)


def test_crop_smaller_than_the_source_and_identity():
    src = _src((3, 40, 36, 3), seed=2)
    plan = np.array([[0, 0, 24, 16, 0], [12, 24, 24, 16, 1], [20, 30, 24, 16, 0]], dtype=np.int32)  # last: hangs over
    _check_exact(src, plan, (16, 24), torch.bfloat16, True)
    sq = _src((2, 36, 36, 3), seed=3)
    _check_exact(sq, AugmentPlanner("identity", 36, 36).plan(2), 36, torch.bfloat16, True)


@pytest.mark.parametrize("channels_last", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_grid_stride_wraps(dtype, channels_last):
    """2100 samples against at most 2048 blocks in y: the batch loop of every instantiation takes a second lap."""
    _check_exact(_src((2100, 8, 8, 3), seed=4), _plan(2100, 8, 8, seed=4, reach=3), 8, dtype, channels_last)


@pytest.mark.parametrize("channels_last", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_source_offset_by_one_byte(dtype, channels_last):
    src = _src((3, 8, 8, 3), seed=5)
    buf = torch.empty(src.numel() + 1, dtype=torch.uint8, device="cuda")
    dev = buf[1:].view(src.shape)
    dev.copy_(src)
    assert dev.data_ptr() % 2 == 1 and dev.is_contiguous()
    _check_exact(src, _plan(3, 8, 8, seed=5, reach=2), 8, dtype, channels_last, dev_src=dev)


# ---------------------------------------------------------------- resize: within the fp32 composition's own error
BOXES = {"whole": (0, 0, 53, 37), "1x1": (20, 10, 1, 1), "far corner 5x7": (48, 30, 5, 7),
         "3 over each edge": (-3, -3, 59, 43)}


def _resize_small():
    src = _src((2, 37, 53, 3), seed=11)
    return [(name, src, np.array([[*b, 0], [*b, 1]], dtype=np.int32), (16, 24)) for name, b in BOXES.items()]


def _resize_rrc():
    plan = AugmentPlanner("rrc", 224, 256, seed=5).plan(2)
    assert ((plan[:, 2] != 224) | (plan[:, 3] != 224)).all()  # both rows resize
    return [("rrc 256 -> 224", _src((2, 256, 256, 3), seed=12), plan, 224)]


def _half_bf16_ulp(ref):
    """Half a bf16 ulp of each reference value: bf16 keeps 8 significant bits, so for
    2^e <= |ref| < 2^(e+1) the ulp is 2^(e-7) and half of it 2^(e-8) -- between 2^-9 |ref|
    (top of the binade) and 2^-8 |ref| (its bottom, where even the correctly rounded
    reference is that far off: 2^-9 |ref| would fail it)."""
    _m, e = torch.frexp(ref.abs())  # |ref| = m 2^e with m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


@pytest.fixture(scope="module", params=["37x53 -> 16x24", "256 -> 224"])
def resize_case(request):
    """(name, [(call, src, plan, size, fp64 reference, the fp32 CPU composition's max error against it)])."""
    calls = _resize_small() if request.param.startswith("37") else _resize_rrc()
    mean, std = MEANS[3]
    out = []
    for name, src, plan, size in calls:
        ref = gpu_augment(src, plan, size, mean, std, dtype=torch.float64, channels_last=False)
        f32 = gpu_augment(src, plan, size, mean, std, dtype=torch.float32, channels_last=False)
        measured = float((f32.double() - ref).abs().max())
        print(f"[gpu_augment] {request.param} / {name}: fp32 CPU composition vs fp64 max abs err {measured:.3e}")
        out.append((name, src, plan, size, ref, measured))
    return request.param, out


@pytest.mark.parametrize("channels_last", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_within_twice_the_fp32_error(resize_case, dtype, channels_last):
    """Each call (one box, unflipped and flipped) against its own measured error, the tightest
    reading of the bound: fp32 within twice the fp32 CPU composition's max error against fp64 on
    that very input, bf16 with half a bf16 ulp of the reference value on top."""
    case, calls = resize_case
    mean, std = MEANS[3]
    for name, src, plan, size, ref, measured in calls:
        assert measured > 0
        out = gpu_augment(src.cuda(), plan, size, mean, std, dtype=dtype, channels_last=channels_last)
        assert out.dtype == dtype and out.shape == ref.shape
        err = (out.cpu().double() - ref).abs()
        bound = torch.full_like(ref, 2 * measured)
        if dtype == torch.bfloat16:
            bound = bound + _half_bf16_ulp(ref)
        print(f"[gpu_augment] {case} / {name} {dtype} cl={channels_last}: max abs err {float(err.max()):.3e}, "
              f"2 x measured {2 * measured:.3e}, worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (name, float(err.max()), 2 * measured)


# ---------------------------------------------------------------- defined behaviour of odd rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_and_outside_boxes(dtype):
    N = _native.require("test")
    mean, std = MEANS[3]
    src = _src((5, 8, 8, 3), seed=6)
    rows = [[1, -1, 8, 8, 1], [0, 0, 0, 8, 0], [2, 2, 8, 8, 0], [0, 0, 8, -3, 1], [100, -200, 8, 8, 0]]
    plan = np.array(rows, dtype=np.int32)
    out = N.augment_batch(src.cuda(), torch.from_numpy(plan).cuda(), 8, 8, list(mean), list(std), dtype, True).cpu()
    assert torch.isnan(out[1]).all() and torch.isnan(out[3]).all()  # cw = 0, ch = -3
    good = [0, 2, 4]
    want = gpu_augment(src[good], plan[good], 8, mean, std, dtype=dtype, channels_last=True)
    assert torch.equal(out[good], want)  # the neighbours are untouched
    pad = ((torch.zeros(3) - torch.tensor(mean)) / torch.tensor(std)).to(dtype)  # wholly outside: the padding value
    assert torch.equal(out[4], pad.view(3, 1, 1).expand(3, 8, 8))
    # wholly outside with a resize; degenerate rows of the scalar kernel
    src2 = _src((2, 5, 7, 3), seed=7)
    plan2 = torch.tensor([[-50, 60, 9, 4, 1], [0, 0, -1, 0, 0]], dtype=torch.int32)
    out2 = N.augment_batch(src2.cuda(), plan2.cuda(), 5, 7, list(mean), list(std), dtype, False).cpu()
    assert torch.isnan(out2[1]).all()
    torch.testing.assert_close(out2[0].float(), pad.float().view(3, 1, 1).expand(3, 5, 7), atol=1e-6, rtol=2.0 ** -8)


@pytest.mark.parametrize("channels_last", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(8, 8), (5, 7)], ids=["vector", "scalar"])
def test_crop_only_kernel_refuses_a_resize_row(hw, dtype, channels_last):
    """no_resize=True is the caller's word; a row that breaks it is written as NaN, the others are exact."""
    N = _native.require("test")
    H, W = hw
    mean, std = MEANS[3]
    src = _src((3, 9, 9, 3), seed=9)
    plan = np.array([[1, 0, W, H, 1], [0, 0, W + 1, H, 0], [-2, 2, W, H, 0]], dtype=np.int32)
    out = N.augment_batch(src.cuda(), torch.from_numpy(plan).cuda(), H, W, list(mean), list(std), dtype,
                          channels_last, True).cpu()
    assert torch.isnan(out[1]).all()
    want = gpu_augment(src[[0, 2]], plan[[0, 2]], (H, W), mean, std, dtype=dtype, channels_last=channels_last)
    assert torch.equal(out[[0, 2]], want)


def test_host_checks():
    N = _native.require("test")
    mean, std = list(MEANS[3][0]), list(MEANS[3][1])
    src = _src((2, 8, 8, 3)).cuda()
    plan = torch.from_numpy(_plan(2, 8, 8)).cuda()
    N.augment_batch(src, plan, 8, 8, mean, std, torch.float32, True)
    for args in ((src.float(), plan, 8, 8, mean, std, torch.float32, True),
                 (src, plan.long(), 8, 8, mean, std, torch.float32, True),
                 (src, plan.cpu(), 8, 8, mean, std, torch.float32, True),
                 (src, plan[:1], 8, 8, mean, std, torch.float32, True),
                 (src, plan, 0, 8, mean, std, torch.float32, True),
                 (src, plan, 8, 16385, mean, std, torch.float32, True),
                 (src, plan, 8, 8, mean[:2], std, torch.float32, True),
                 (src, plan, 8, 8, mean, [0.2, 0.0, 0.2], torch.float32, True),
                 (src, plan, 8, 8, mean, std, torch.float16, True),
                 (src.permute(0, 2, 1, 3), plan, 8, 8, mean, std, torch.float32, True),
                 (_src((2, 8, 8, 5)).cuda(), plan, 8, 8, mean + [0.5, 0.5], std + [0.2, 0.2], torch.float32, True)):
        with pytest.raises(RuntimeError, match="augment_batch"):
            N.augment_batch(*args)


_CHILD = r"""
import importlib, numpy as np, torch
from distributed_model_parallel_amd.data import gpu_augment, transforms as T
GA = importlib.import_module("distributed_model_parallel_amd.data.gpu_augment")
src = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(4, 32, 32, 3), dtype=np.uint8))
plan = np.array([[-4, -4, 32, 32, 1], [4, 4, 32, 32, 0], [-4, 4, 32, 32, 1], [0, 0, 32, 32, 0]], dtype=np.int32)
want = gpu_augment(src, plan, 32, T.CIFAR_MEAN, T.CIFAR_STD)
before = dict(GA._STATS)
out = gpu_augment(src.cuda(), plan, 32, T.CIFAR_MEAN, T.CIFAR_STD)
print("ROUTE", GA._STATS["native"] - before["native"], GA._STATS["torch"] - before["torch"],
      int(out.is_cuda), int(torch.equal(out.cpu(), want)))
"""


def test_disable_feature_in_child_process():
    """DMP_DISABLE=gpu_augment: the torch composition on the device, the same bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DMP_DISABLE="gpu_augment")
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROUTE")][-1].split()
    assert line[1:] == ["0", "1", "1", "1"], r.stdout
    # and the kernel gives those bits too (this process has the feature on)
    src = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(4, 32, 32, 3), dtype=np.uint8))
    plan = np.array([[-4, -4, 32, 32, 1], [4, 4, 32, 32, 0], [-4, 4, 32, 32, 1], [0, 0, 32, 32, 0]], dtype=np.int32)
    _check_exact(src, plan, 32, torch.bfloat16, True)
