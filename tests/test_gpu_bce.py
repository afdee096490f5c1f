"""csrc/loss/bce.hip against timm's dense target in float64 (timm_bce) and autograd's gradient of it.  Bounds:
the loss within atol = rtol = 1e-5 (the cross-entropy's; fp32 sums of <= 1000 softplus terms stay inside).  A
gradient element is at most s = |g| * scale / norm: 2e-6 * s for the fast exp / reciprocal in the sigmoid, plus
one rounding to the gradient's dtype, eps * |ref| (eps = 2^-24 / 2^-8).  With e = 0.1, lam = 0.3 the dense
values are <= 0.01, 0.27..0.28 and 0.63..0.64: none near the 0.2 threshold."""
import pytest
import torch

from distributed_model_parallel_amd.ops.loss import _STATS, binary_cross_entropy, binary_cross_entropy_with_stats
from tests.test_bce_cpu import MODES, timm_bce
from tests.test_gpu_loss_mix import SHAPES, _case  # an ignored first row, class 0 / C-1, both labels on one class

pytestmark = pytest.mark.gpu
MIXED = dict(label_smoothing=0.1, lam=0.3, target_thresh=0.2)
DTYPES = [torch.float32, torch.bfloat16]


def _check(x, a, b, g=2.0, scale=1.0, stats=None, **kw):
    """One native forward + backward inside the bounds; returns (loss, gradient)."""
    xa = x.detach().requires_grad_()
    n0 = _STATS["native"]
    loss = (binary_cross_entropy(xa, a, target_b=b, **kw) if stats is None else
            binary_cross_entropy_with_stats(xa, a, scale, stats, target_b=b, **kw))
    assert _STATS["native"] == n0 + 1
    (loss * g).backward()
    xd = x.detach().double().requires_grad_()
    ref = timm_bce(xd, a, target_b=b, **kw)
    (ref * g * scale).backward()
    gref, norm = xd.grad, float((a != -100).sum()) * (1 if kw.get("sum_classes") else x.shape[1])
    torch.testing.assert_close(loss.double(), ref.detach() * scale, atol=1e-5, rtol=1e-5)
    assert xa.grad.dtype == x.dtype and xa.grad.shape == x.shape
    eps = 2.0 ** -24 if x.dtype == torch.float32 else 2.0 ** -8
    err, bound = (xa.grad.double() - gref).abs(), 2e-6 * g * scale / norm + eps * gref.abs()
    print(f"loss {float(loss.detach()):.8g} (ref {float(ref.detach()) * scale:.8g}), gradient error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert not xa.grad[a == -100].any()  # ignored rows: exactly zero
    return loss.detach(), xa.grad


@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("e,paired,lam,thresh", MODES)
@pytest.mark.parametrize("B,C", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_matches_the_dense_target_reference(dtype, B, C, e, paired, lam, thresh, sum_classes):
    x, a, b = _case(B, C, dtype)
    _check(x, a, b if paired else None, label_smoothing=e, lam=lam, target_thresh=thresh, sum_classes=sum_classes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_extreme_logits(dtype):
    """+-100 and +-30 on labelled and unlabelled classes: a naive log(1 + exp(x)) overflows here."""
    x, a, b = _case(33, 365, dtype)
    big, r = torch.tensor([100.0, -100.0, 30.0, -30.0], device="cuda").to(dtype), torch.arange(5, 9, device="cuda")
    x[r, a[r]], x[r + 4, b[r + 4]], x[r + 8, a[r + 8]], x[20:24, 17] = big, big, big.flip(0), big
    assert torch.isfinite(_check(x, a, b, **MIXED)[0]).item()
    _check(x, a, None)


@pytest.mark.parametrize("c0", [0, 1, 3])
def test_row_stride_and_alignment(c0):
    """A column slice (row stride != C) starting 0, 1 or 3 elements into an allocation full of 50s."""
    x, a, b = _case(64, 1000, torch.bfloat16)
    xv = torch.full((64, 1024), 50.0, dtype=x.dtype, device="cuda")[:, c0:c0 + 1000]
    xv.copy_(x)
    assert not xv.is_contiguous() and (xv.data_ptr() % 16 == 0) == (c0 == 0)
    _check(xv, a, b, **MIXED)  # inside the bounds of the contiguous call's reference: nothing off the row was read


@pytest.mark.parametrize("which,bad", [("a", 10), ("a", -3), ("b", 10), ("b", -100)])
def test_label_out_of_range_is_nan_not_oob(which, bad):
    torch.manual_seed(1)
    x = torch.randn(8, 10, device="cuda", requires_grad=True)
    a, b = torch.randint(0, 10, (8,), device="cuda"), torch.randint(0, 10, (8,), device="cuda")
    a[5], b[5] = -100, bad  # on the ignored row: no effect
    (a if which == "a" else b)[3] = bad
    loss = binary_cross_entropy(x, a, label_smoothing=0.1, target_b=b, lam=0.4)
    assert torch.isnan(loss).item()
    loss.backward()
    assert torch.isnan(x.grad[3]).all().item()
    assert torch.isfinite(x.grad[[i for i in range(8) if i != 3]]).all().item()
    assert not x.grad[5].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_stats_scaled_loss_and_first_label_counts(dtype):
    x, a, b = _case(64, 1000, dtype, seed=3)
    a[0] = 7  # binary_cross_entropy_with_stats has no ignored rows
    stats = torch.full((3,), 1.5, dtype=torch.float64, device="cuda")
    loss, _ = _check(x, a, b, scale=0.25, stats=stats, **MIXED)
    assert float(stats[0]) - 1.5 == pytest.approx(float(loss), rel=1e-6)
    xf = x.float()
    xt = xf.gather(1, a[:, None])
    rank = ((xf > xt) | ((xf == xt) & (torch.arange(1000, device="cuda")[None, :] < a[:, None]))).sum(1)
    assert (float(stats[1]) - 1.5, float(stats[2]) - 1.5) == (float((rank < 1).sum()), float((rank < 5).sum()))


def _run(x, a, **kw):
    loss = binary_cross_entropy(x, a, **kw)
    return loss, torch.autograd.grad(loss, x)[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_labels_and_defaults_give_the_same_bits(dtype):
    x, a, _ = _case(33, 365, dtype)
    x.requires_grad_()
    explicit = dict(ignore_index=-100, label_smoothing=0.0, target_b=None, lam=1.0, target_thresh=None, sum_classes=False)
    for kw, twin in ((dict(label_smoothing=0.1, target_b=a.clone(), lam=0.3), dict(label_smoothing=0.1)), (explicit, {})):
        (l1, g1), (l2, g2) = _run(x, a, **kw), _run(x, a, **twin)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_graph_replay_equals_eager_bit_for_bit():
    x, a, b = _case(64, 1000, torch.bfloat16)
    x.requires_grad_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(x, a, target_b=b, **MIXED)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = _run(x, a, target_b=b, **MIXED)
    for seed in (1, 2):  # new logits in the static input
        x.data.copy_(_case(64, 1000, torch.bfloat16, seed=seed)[0])
        graph.replay()
        le, ge = _run(x, a, target_b=b, **MIXED)
        assert torch.equal(loss, le) and torch.equal(grad, ge)
