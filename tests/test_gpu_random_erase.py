"""Random-erasing kernels (csrc/data/random_erase.hip) against the definition of data/random_erase.py:
the device generator bit for bit against the NumPy Philox, the fp32 noise within 1e-5 of the fp64
evaluation of the definition (u is exact; the fp32 angle, logf, sqrtf and sincospif contribute a few
ulp of a value <= 5.77, about 2e-6; an indexing, shift or key mistake is off by order 1), bf16 as the
rounded fp32 output, and every bit outside the boxes unchanged."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.data import RandomErasePlanner, random_erase_
from distributed_model_parallel_amd.data import random_erase as RE

pytestmark = pytest.mark.gpu

TOL = 1e-5
TILE_W, TILE_H = 64, 4  # csrc/data/random_erase.hip: a block is 4 waves, each a 64-pixel row segment
VARIANTS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)]


def _boxes(rows, seed=99):
    b = np.zeros((len(rows), 6), dtype=np.int32)
    b[:, :4] = rows
    keys = np.random.default_rng(seed).integers(0, 1 << 32, size=(len(rows), 2), dtype=np.uint64)
    keys[0] |= np.uint64(0x80000000)  # a key with both top bits set
    b[:, 4:] = keys.astype(np.uint32).view(np.int32)
    return b


def _batch(B, C, H, W, seed=0):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
    x[0, 0, 0, 0], x[-1, -1, -1, -1] = float("nan"), float("-inf")  # bits, not values
    return x


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _inside(rows, C, H, W):
    m = torch.zeros(len(rows), 1, H, W, dtype=torch.bool)
    for i, (x0, y0, w, h) in enumerate(rows):
        m[i, :, y0:y0 + h, x0:x0 + w] = True
    return m.expand(-1, C, -1, -1)


def _check(rows, C, H, W, fill=None, noise=True, seed=0):
    """One fp64 oracle on the CPU; every dtype / layout of the kernel against it."""
    boxes, src = _boxes(rows, seed + 99), _batch(len(rows), C, H, W, seed)
    want = random_erase_(src.double(), boxes, fill, noise)
    inside = _inside(rows, C, H, W)
    got32 = {}
    for dtype, cl in VARIANTS:
        x = src.to(dtype).cuda()
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        before, stats = x.clone(), dict(RE._STATS)
        out = random_erase_(x, boxes, fill, noise)
        assert out is x and x.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        erased = bool(inside.any())
        assert RE._STATS["native"] == stats["native"] + erased and RE._STATS["torch"] == stats["torch"]
        got = x.cpu()
        assert torch.equal(_bits(got)[~inside], _bits(before.cpu())[~inside]), f"{dtype} cl={cl}: written outside"
        if dtype == torch.float32:
            got32[cl] = got
            if erased:
                err = (got.double() - want)[inside].abs().max().item()
                if noise:
                    print(f"C={C} {H}x{W} cl={cl}: max |kernel - fp64 oracle| = {err:.3g}")
                    assert err <= TOL, (dtype, cl, err)
                else:  # const / rand: exact
                    assert torch.equal(got[inside], want.float()[inside])
        else:  # the fp32 output of the same plan, rounded once
            assert torch.equal(_bits(got)[inside], _bits(got32[cl].bfloat16())[inside]), f"bf16 cl={cl}"
    assert torch.equal(_bits(got32[False]), _bits(got32[True]))  # NCHW and channels-last: the same bits
    return got32[False]


# ---------------------------------------------------------------- the generator
KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1"))


def _device_bits(counters, key):
    N = _native.require("philox_bits")
    c = torch.from_numpy(np.ascontiguousarray(counters, dtype=np.uint32).view(np.int32)).cuda()
    k = torch.from_numpy(np.asarray(key, dtype=np.uint32).view(np.int32)).cuda()
    return N.philox_bits(c, k).cpu().numpy().view(np.uint32)


def test_philox_bits_known_answers():
    for counter, key, want in KNOWN:
        got = _device_bits(np.array([counter], dtype=np.uint32), key)
        assert " ".join(f"{v:08x}" for v in got[0]) == want


def test_philox_bits_equal_the_numpy_generator():
    rng = np.random.default_rng(4)
    c = rng.integers(0, 1 << 32, size=(4096, 4), dtype=np.uint64).astype(np.uint32)
    edge = [0, 1, 32767]
    c[:9, 0], c[:9, 1] = np.repeat(edge, 3), np.tile(edge, 3)  # x and y at 0, 1 and 32767 ...
    c[:9, 2:] = 0  # ... as the eraser forms its counters
    c[9:13] = [[0xFFFFFFFF] * 4, [0x80000000] * 4, [0x7FFFFFFF] * 4, [0xFFFF0000, 0x0000FFFF, 0x80000001, 1]]
    for key in ((0, 0), (0xFFFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (0x9E3779B9, 0xBB67AE85)):
        assert np.array_equal(_device_bits(c, key), RE.philox4x32(c, np.array(key, dtype=np.uint32))), key
    assert _device_bits(np.zeros((0, 4), dtype=np.uint32), (1, 2)).shape == (0, 4)


# ---------------------------------------------------------------- the eraser
@pytest.mark.parametrize("C", [1, 3, 4])
def test_small_image_corners_edges_and_whole(C):
    rows = [(0, 0, 1, 1), (7, 0, 1, 1), (0, 7, 1, 1), (7, 7, 1, 1),  # a 1 x 1 box at each corner
            (0, 0, 3, 2), (5, 0, 3, 4), (0, 5, 2, 3), (4, 6, 4, 2),  # a box at each corner
            (3, 2, 5, 6),  # reaching the right and the bottom edge
            (0, 0, 8, 8),  # the whole image
            (0, 0, 0, 0), (1, 1, 5, 3)]
    _check(rows, C, 8, 8)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_odd_sizes_and_odd_offsets(C):
    H, W = 37, 53
    rows = [(1, 1, 51, 35), (0, 0, 53, 37), (52, 36, 1, 1), (0, 0, 0, 0),
            (17, 5, 33, 9),  # odd x0 with odd w: at C = 3 bf16 the 2-byte-aligned stores
            (11, 3, 7, 31), (50, 0, 3, 37), (0, 34, 53, 3)]
    _check(rows, C, H, W, seed=1)


def test_tile_and_wave_edges():
    """Widths and heights one below, at and one above the tile (64 x 4: the width is the wave)."""
    H, W = 64, 70
    rows = [(x0, y0, w, h) for (w, x0) in ((TILE_W - 1, 1), (TILE_W, 0), (TILE_W + 1, 5), (TILE_W, 6))
            for (h, y0) in ((TILE_H - 1, 0), (TILE_H, 60), (TILE_H + 1, 3), (2 * TILE_H, 1), (2 * TILE_H + 1, 55))]
    _check(rows[:16], 3, H, W, seed=2)
    _check(rows[16:] + [(0, 0, 1, H), (0, 0, W, 1), (0, 0, W, H)], 3, H, W, seed=3)


def test_only_the_last_sample_is_erased():
    _check([(0, 0, 0, 0)] * 15 + [(20, 10, 40, 50)], 3, 64, 64, seed=4)


def test_no_erased_sample_launches_nothing():
    x = _batch(4, 3, 8, 8).cuda()
    keep, stats = x.clone(), dict(RE._STATS)
    assert random_erase_(x, _boxes([(0, 0, 0, 0)] * 4)) is x
    assert RE._STATS == stats  # neither the kernel nor the composition
    assert torch.equal(_bits(x), _bits(keep))
    _check([(0, 0, 0, 0)] * 4, 3, 8, 8)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_const_and_rand_are_exact(C):
    rows = [(17, 5, 33, 9), (0, 0, 0, 0), (0, 0, 53, 37), (52, 36, 1, 1)]
    _check(rows, C, 37, 53, noise=False)
    got = _check(rows, C, 37, 53, fill=np.random.default_rng(3).standard_normal((4, C)).astype(np.float32), noise=False)
    assert got[2].abs().max() > 0


def test_same_key_same_field_anywhere():
    """The values depend on (key, x, y, c) alone: batch position, box, image size and channel count."""
    H, W = 64, 64
    a = _check([(3, 5, 50, 40), (0, 0, 0, 0)], 3, H, W, seed=5)
    boxes = _boxes([(3, 5, 50, 40), (0, 0, 0, 0)], 5 + 99)
    moved = np.zeros((3, 6), dtype=np.int32)
    moved[2] = (10, 8, 30, 29, boxes[0, 4], boxes[0, 5])
    x = torch.zeros(3, 4, 37, 53, device="cuda")
    random_erase_(x, moved)
    assert torch.equal(x[2, :3, 8:37, 10:40].cpu(), a[0, :, 8:37, 10:40])


def test_planner_plans_run():
    p = RandomErasePlanner(0.5, seed=6)
    for _ in range(3):
        boxes, _fill = p.plan(16, 37, 53)
        _check([tuple(r) for r in boxes[:, :4].tolist()], 3, 37, 53, seed=6)


def test_moments_of_the_kernel_output():
    """16 samples with a 64 x 64 x 3 box, keys from default_rng([0, 0, 0]): 196 608 values, the bounds of
    tests/test_random_erase_cpu.py (the fp64 definition gives mean 0.00047, var 0.9960, max |z| 4.64)."""
    boxes = np.zeros((16, 6), dtype=np.int32)
    boxes[:, 2:4] = 64
    keys = np.random.default_rng([0, 0, 0]).integers(0, 1 << 32, size=(16, 2), dtype=np.uint64)
    boxes[:, 4:] = keys.astype(np.uint32).view(np.int32)
    for cl in (False, True):
        x = torch.zeros(16, 3, 64, 64, device="cuda")
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        z = random_erase_(x, boxes).cpu().double().flatten()
        n = z.numel()
        mean, var, top = z.mean().item(), z.var(unbiased=False).item(), z.abs().max().item()
        print(f"cl={cl}: mean {mean:.5f} var {var:.5f} max {top:.4f}")
        assert n == 196608
        assert abs(mean) < 5 / math.sqrt(n)  # 0.0113
        assert abs(var - 1) < 5 * math.sqrt(2 / n)  # 0.0160
        assert top <= 5.77


def test_host_checks():
    N = _native.require("random_erase")
    x = torch.zeros(2, 3, 8, 8, device="cuda")
    good = _boxes([(0, 0, 2, 2), (0, 0, 0, 0)])
    bad = good.copy()
    bad[1, :4] = (7, 0, 2, 2)
    with pytest.raises(ValueError, match="boxes row 1 "):
        random_erase_(x, bad)
    with pytest.raises(ValueError, match="dense"):
        random_erase_(torch.zeros(2, 3, 8, 16, device="cuda")[..., ::2], good)
    for call in (lambda: N.random_erase(x, torch.from_numpy(bad), None, True),  # the entry point checks the rows again
                 lambda: N.random_erase(x, torch.from_numpy(good).cuda(), None, True),
                 lambda: N.random_erase(x, torch.from_numpy(good[:1]), None, True),
                 lambda: N.random_erase(x, torch.from_numpy(good), torch.zeros(2, 3), True),
                 lambda: N.random_erase(x, torch.from_numpy(good), torch.zeros(2, 2), False),
                 lambda: N.random_erase(x.cpu(), torch.from_numpy(good), None, True),
                 lambda: N.random_erase(x.half(), torch.from_numpy(good), None, True),
                 lambda: N.random_erase(torch.zeros(2, 5, 8, 8, device="cuda"), torch.from_numpy(good), None, True),
                 lambda: N.philox_bits(torch.zeros(4, 3, dtype=torch.int32, device="cuda"),
                                       torch.zeros(2, dtype=torch.int32, device="cuda")),
                 lambda: N.philox_bits(torch.zeros(4, 4, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(RuntimeError):
            call()
    assert not x.any()  # a refused call has written nothing


_CHILD = r"""
import numpy as np, torch
from distributed_model_parallel_amd.data import random_erase as RE
boxes = np.zeros((4, 6), dtype=np.int32)
boxes[:, :4] = [(17, 5, 33, 9), (0, 0, 0, 0), (0, 0, 53, 37), (52, 36, 1, 1)]
boxes[:, 4:] = np.random.default_rng(8).integers(0, 1 << 32, size=(4, 2), dtype=np.uint64).astype(np.uint32).view(np.int32)
src = torch.randn(4, 3, 37, 53, generator=torch.Generator().manual_seed(8))
want = RE.random_erase_(src.double(), boxes)
before = dict(RE._STATS)
got = RE.random_erase_(src.cuda().contiguous(memory_format=torch.channels_last), boxes)
assert got.is_cuda
err = (got.cpu().double() - want).abs().max().item()
print("ROUTE", RE._STATS["native"] - before["native"], RE._STATS["torch"] - before["torch"], err)
"""


def test_disable_feature_in_child_process():
    """DMP_DISABLE=random_erase: the PyTorch composition on the device, within the same 1e-5."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DMP_DISABLE="random_erase")
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROUTE")][-1].split()
    assert line[:3] == ["ROUTE", "0", "1"], line
    assert float(line[3]) <= TOL, line
