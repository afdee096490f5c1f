"""Soft-target cross-entropy kernels (label smoothing, a second label weighted
1 - lam) against F.cross_entropy in fp32, and the batch-mixing kernel
(csrc/data/batch_mix.hip) against the indexed paste / the fp32 formula."""
import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd.ops import mix as M
from distributed_model_parallel_amd.ops.loss import _STATS, cross_entropy, cross_entropy_with_stats
from distributed_model_parallel_amd.ops.mix import BatchMixer, batch_mix

pytestmark = pytest.mark.gpu

# rows shorter than a wave, one partial lap, a batch not divisible by the four rows of a block,
# the real class count
SHAPES = [(7, 10), (5, 70), (33, 365), (64, 1000)]
MODES = [(0.1, False, 1.0), (0.0, True, 0.3), (0.1, True, 0.3)]  # (e, with target_b, lam)


def _case(B, C, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + B + C)
    x = (torch.randn(B, C, generator=g) * 3).to(dtype).cuda()
    a = torch.randint(0, C, (B,), generator=g)
    b = torch.randint(0, C, (B,), generator=g)
    a[1], b[1] = 0, C - 1          # class 0 and class C-1
    a[2], b[2] = C - 1, 0
    a[3] = b[3] = C // 2           # both labels on one class
    b[4] = a[4]
    a[0] = -100                    # ignored row (its second label is a valid class)
    return x, a.cuda(), b.cuda()


def _reference(xr, a, b, e, lam):
    """lam * CE(a) + (1 - lam) * CE(b) with torch in fp32; a row is ignored iff its first label is."""
    if b is None:
        return F.cross_entropy(xr, a, label_smoothing=e)
    b = torch.where(a == -100, a, b)
    return lam * F.cross_entropy(xr, a, label_smoothing=e) + (1 - lam) * F.cross_entropy(xr, b, label_smoothing=e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", SHAPES)
@pytest.mark.parametrize("e,paired,lam", MODES)
def test_soft_cross_entropy_matches_torch(dtype, B, C, e, paired, lam):
    """Tolerances of tests/test_gpu_loss.py for the plain loss.  Gradient rows sum
    to zero up to their rounding: the softmax is exp(x - lse) with lse (|lse| < 32)
    rounded to fp32, half an ulp = 1e-6, which scales the whole row, plus the fast
    exp / log (about 1e-6 each): 1e-5 of the row scale in all; then each element is
    rounded to the gradient's dtype (2^-24 / 2^-9 of its magnitude)."""
    x, a, b = _case(B, C, dtype)
    tb = b if paired else None
    xa = x.detach().requires_grad_()
    xr = x.detach().float().requires_grad_()
    n0 = _STATS["native"]
    la = cross_entropy(xa, a, label_smoothing=e, target_b=tb, lam=lam)
    assert _STATS["native"] == n0 + 1
    lr = _reference(xr, a, tb, e, lam)
    torch.testing.assert_close(la, lr, atol=1e-5, rtol=1e-5)
    (la * 2.0).backward()
    (lr * 2.0).backward()
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    torch.testing.assert_close(xa.grad.float(), xr.grad, atol=tol, rtol=1e-2)
    assert xa.grad.dtype == dtype
    g = xa.grad.float()
    assert torch.equal(g[0], torch.zeros_like(g[0]))  # the ignored row
    scale = 2.0 / (B - 1)
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -9
    bound = 1e-5 * scale + g[1:].abs().sum(1) * eps
    assert (g[1:].sum(1).abs() <= bound).all(), (g[1:].sum(1).abs() / bound).max()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_second_label_equal_to_the_first_is_the_plain_loss(dtype):
    x, a, _ = _case(33, 365, dtype)
    xa, xp = x.detach().requires_grad_(), x.detach().requires_grad_()
    la = cross_entropy(xa, a, label_smoothing=0.0, target_b=a.clone(), lam=0.3)
    lp = cross_entropy(xp, a)
    torch.testing.assert_close(la, lp, atol=1e-6, rtol=1e-6)
    la.backward()
    lp.backward()
    torch.testing.assert_close(xa.grad.float(), xp.grad.float(), atol=1e-6 if dtype == torch.float32 else 2e-3,
                               rtol=1e-2)


def test_defaults_run_the_plain_kernels_bit_for_bit():
    x, a, _ = _case(64, 1000, torch.bfloat16)
    x1, x2 = x.detach().requires_grad_(), x.detach().requires_grad_()
    l1 = cross_entropy(x1, a)
    l2 = cross_entropy(x2, a, label_smoothing=0.0, target_b=None, lam=1.0)
    assert torch.equal(l1, l2)
    l1.backward()
    l2.backward()
    assert torch.equal(x1.grad, x2.grad)


@pytest.mark.parametrize("bad", [10, -3, -100])
def test_second_label_out_of_range_is_nan_not_oob(bad):
    """A second label outside [0, C) on a valid row (ignore_index counts as outside:
    only the first label ignores a row) reads nothing: NaN loss, NaN gradient row;
    the other rows stay finite."""
    torch.manual_seed(1)
    x = torch.randn(8, 10, device="cuda", requires_grad=True)
    a = torch.randint(0, 10, (8,), device="cuda")
    b = torch.randint(0, 10, (8,), device="cuda")
    a[5] = -100
    b[5] = bad  # on the ignored row: no effect
    b[3] = bad
    loss = cross_entropy(x, a, label_smoothing=0.1, target_b=b, lam=0.4)
    assert torch.isnan(loss).item()
    loss.backward()
    assert torch.isnan(x.grad[3]).all().item()
    keep = [i for i in range(8) if i != 3]
    assert torch.isfinite(x.grad[keep]).all().item()
    assert torch.equal(x.grad[5], torch.zeros_like(x.grad[5]))


def test_native_argument_checks():
    from distributed_model_parallel_amd import _native
    C = _native.require("test")
    x = torch.randn(4, 10, device="cuda")
    t = torch.zeros(4, dtype=torch.int64, device="cuda")
    for kw in (dict(label_smoothing=1.0), dict(lam=1.5), dict(target_b=t[:3]), dict(target_b=t.int()),
               dict(target_b=t.cpu())):
        with pytest.raises(RuntimeError):
            C.cross_entropy_fwd(x, t, **kw)
    with pytest.raises(ValueError):
        cross_entropy(x, t, target_b=t.cpu())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_with_stats_mixed_loss_and_first_label_counts(dtype):
    B, C = 64, 1000
    x, a, b = _case(B, C, dtype, seed=3)
    a[0] = 7  # cross_entropy_with_stats has no ignored rows
    stats = torch.full((3,), 1.5, dtype=torch.float64, device="cuda")
    xa = x.clone().requires_grad_()
    n0 = _STATS["native"]
    loss = cross_entropy_with_stats(xa, a, 0.25, stats, label_smoothing=0.1, target_b=b, lam=0.3)
    assert _STATS["native"] == n0 + 1
    loss.backward()
    xr = x.float().clone().requires_grad_()
    ref = _reference(xr, a, b, 0.1, 0.3) * 0.25
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-5 * max(1.0, abs(float(ref.detach())))
    torch.testing.assert_close(xa.grad.float(), xr.grad, atol=2e-3 if dtype == torch.bfloat16 else 1e-6, rtol=1e-2)
    assert abs(float(stats[0]) - 1.5 - float(ref.detach())) < 1e-5 * max(1.0, abs(float(ref.detach())))
    xf = x.float()
    xt = xf.gather(1, a[:, None])
    idx = torch.arange(C, device="cuda")[None, :]
    rank = ((xf > xt) | ((xf == xt) & (idx < a[:, None]))).sum(1)
    assert float(stats[1]) - 1.5 == float((rank < 1).sum())
    assert float(stats[2]) - 1.5 == float((rank < 5).sum())


# ---------------------------------------------------------------- batch_mix
# (3, 3, 5, 7): an odd per-sample element count -- the scalar path, unaligned sample bases
MIX_SHAPES = [(3, 3, 5, 7), (4, 3, 32, 32), (2, 16, 8, 8)]


def _batch(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    B = shape[0]
    k = min(B, 3)  # a cycle over the first rows (not its own inverse at B >= 3), the rest fixed points
    perm = torch.tensor([(i + 1) % k for i in range(k)] + list(range(k, B)))
    return x, perm.cuda()


def _boxes(H, W):
    return {"interior": (1, H - 1, 2, W - 2), "two_edges": (H // 2, H, W // 2, W), "pixel": (2, 3, 3, 4),
            "empty": (2, 2, 0, W), "whole": (0, H, 0, W)}


def _paste(x, perm, box):
    y0, y1, x0, x1 = box
    ref = x.clone()
    ref[:, :, y0:y1, x0:x1] = x[perm][:, :, y0:y1, x0:x1]
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", MIX_SHAPES)
def test_cutmix_is_the_indexed_paste(dtype, shape):
    x, perm = _batch(shape, dtype)
    x0 = x.clone()
    ident = torch.arange(shape[0], device="cuda")
    n0 = M._STATS["native"]
    for name, box in _boxes(shape[2], shape[3]).items():
        out = batch_mix(x, perm, 0.5, box)
        assert torch.equal(out, _paste(x, perm, box)), name
        assert out.stride() == x.stride() and out.dtype == dtype
        assert torch.equal(batch_mix(x, ident, 0.5, box), x), name
    assert M._STATS["native"] == n0 + 10
    assert torch.equal(batch_mix(x, perm, 0.5, (2, 2, 0, shape[3])), x)
    assert torch.equal(batch_mix(x, perm, 0.5, (0, shape[2], 0, shape[3])), x[perm])
    assert torch.equal(x, x0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", MIX_SHAPES)
def test_mixup_is_the_fp32_formula(dtype, shape):
    x, perm = _batch(shape, dtype)
    x0 = x.clone()
    assert torch.equal(batch_mix(x, perm, 1.0), x)
    for lam in (0.25, 0.7):
        out = batch_mix(x, perm, lam)
        ref = (lam * x.float() + (1 - lam) * x[perm].float()).to(dtype)
        if dtype == torch.float32:
            torch.testing.assert_close(out, ref, atol=1e-6, rtol=0)
        else:  # one bf16 ulp: a fused multiply-add may round the other way
            torch.testing.assert_close(out.float(), ref.float(), atol=0, rtol=2.0 ** -7)
        assert out.stride() == x.stride() and out.dtype == dtype
    ident = torch.arange(shape[0], device="cuda")
    torch.testing.assert_close(batch_mix(x, ident, 0.25).float(), x.float(), atol=1e-6, rtol=2.0 ** -7)
    assert torch.equal(x, x0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_vector_sized_samples_on_an_unaligned_base_take_the_scalar_path(dtype):
    """n is a multiple of the 16-byte vector but the tensor starts one element into
    its allocation: 16-byte accesses would be misaligned, so the scalar kernel runs."""
    B, C, H, W = 3, 3, 8, 8
    flat = torch.randn(B * C * H * W + 1, device="cuda").to(dtype)
    x = flat[1:].view(B, H, W, C).permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 != 0
    perm = torch.tensor([2, 0, 1], device="cuda")
    assert torch.equal(batch_mix(x, perm, 0.5, (1, 6, 2, 8)), _paste(x, perm, (1, 6, 2, 8)))
    ref = (0.7 * x.float() + (1 - 0.7) * x[perm].float()).to(dtype)
    torch.testing.assert_close(batch_mix(x, perm, 0.7).float(), ref.float(), atol=1e-6, rtol=2.0 ** -7)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", MIX_SHAPES)
@pytest.mark.parametrize("box", [None, "interior"])
def test_hostile_perm_rows_are_nan(dtype, shape, box):
    """A perm entry outside [0, B) reads nothing: exactly that output row is NaN."""
    x, perm = _batch(shape, dtype)
    B = shape[0]
    bx = _boxes(shape[2], shape[3])[box] if box else None
    good = batch_mix(x, perm, 0.25, bx)
    for row, bad in ((0, B), (B - 1, -1)):
        p = perm.clone()
        p[row] = bad
        out = batch_mix(x, p, 0.25, bx)
        assert torch.isnan(out[row]).all().item()
        keep = [i for i in range(B) if i != row]
        assert torch.equal(out[keep], good[keep])


def test_batch_mixer_on_the_gpu():
    twin = BatchMixer(0.8, 1.0, seed=11)
    m = BatchMixer(0.8, 1.0, seed=11)
    x, _ = _batch((4, 3, 32, 32), torch.bfloat16)
    y = torch.tensor([3, 1, 4, 1], device="cuda")
    kinds = set()
    for _ in range(8):
        p = twin.plan(4, 32, 32)
        xm, ya, yb, lam = m(x, y)
        perm = torch.from_numpy(p.perm).cuda()
        assert torch.equal(xm, batch_mix(x, perm, p.lam, p.box))
        assert ya is y and torch.equal(yb, y[perm]) and lam == p.lam
        kinds.add(p.kind)
    assert kinds == {"mixup", "cutmix"}
