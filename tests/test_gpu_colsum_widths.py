"""The column-sum side passes (csrc/linear/bias_act.hip) at widths that are
multiples of 64 but not of 256 -- ConvNeXt's 128-wide first stage, and the
64 / 192 / 384 / 448 around it.  These run the 4-column-per-lane kernels with
lanes past the last column idle.

Integer data: every sum is an exact integer below 2^24, so fp32 partials and
the column reduce are exact, and "the sum equals the stored tensor's column
sum" (what the kernels promise for the tensors they write) is asserted
bitwise."""
import pytest
import torch

from distributed_model_parallel_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = [64, 128, 192, 384, 448]
ROWS = [1, 31, 4100]


def _ints(m, n, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, (m, n), device=DEV).bfloat16()


def _once(t64, dtype):
    return t64.float().to(dtype)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", WIDTHS)
def test_bias_grad(n, m):
    C = _native.require("colsum")
    assert C.colsum_supported(n)
    torch.manual_seed(0)
    dy = _ints(m, n)
    ref = dy.double().sum(0)
    for od in (torch.float32, torch.bfloat16):
        db = C.bias_grad(dy, od)
        assert db.shape == (n,) and db.dtype == od
        assert torch.equal(db, _once(ref, od))


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", WIDTHS)
def test_gelu_bwd_bias_grad(n, m):
    """dh = bf16(dy * gelu'(h)) within one bf16 rounding of the fp64 value, and
    db the exact column sum of the STORED dh (randn h: dh is not integer, so the
    fp32 sum is compared under m * U * sum|dh|)."""
    C = _native.require("colsum")
    torch.manual_seed(1)
    dy = _ints(m, n)
    h = torch.randn(m, n, device=DEV).bfloat16()
    dh, db = C.gelu_bwd_bias_grad(dy, h, torch.float32)
    assert dh.shape == (m, n) and dh.dtype == torch.bfloat16 and db.shape == (n,)
    h64 = h.double()
    g = 0.5 * (1 + torch.erf(h64 / 2 ** 0.5)) + h64 * torch.exp(-0.5 * h64 * h64) / (2 * torch.pi) ** 0.5
    ref = dy.double() * g
    assert bool(((dh.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-5 * dy.double().abs()).all())
    s = dh.double().sum(0)
    assert bool(((db.double() - s).abs() <= (m + 16) * 2.0 ** -24 * dh.double().abs().sum(0)).all())
    # h = 0: gelu'(0) = 1/2 exactly, dh = dy / 2 is exact in bf16 and the sums are exact
    dh0, db0 = C.gelu_bwd_bias_grad(dy, torch.zeros_like(h), torch.float32)
    assert torch.equal(dh0, (dy.float() * 0.5).bfloat16())
    assert torch.equal(db0, dh0.double().sum(0).float())


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", WIDTHS)
def test_rowscale_bias_grad(n, m):
    """Scales in {0, 1, 2}: g = dy * s[row / rows_per_sample] and its column sums are exact.
    M = 4100 is 100 samples of 41 rows."""
    C = _native.require("colsum")
    torch.manual_seed(2)
    rps = 41 if m == 4100 else m
    dy = _ints(m, n)
    s = torch.randint(0, 3, (m // rps,), device=DEV).float()
    g, db = C.rowscale_bias_grad(dy, s, rps, torch.float32)
    gr = dy.double() * s.double().repeat_interleave(rps).view(-1, 1)
    assert torch.equal(g.double(), gr)
    assert torch.equal(db, g.double().sum(0).float())
    gb, dbb = C.rowscale_bias_grad(dy, s, rps, torch.bfloat16)
    assert torch.equal(gb, g) and torch.equal(dbb, _once(gr.sum(0), torch.bfloat16))


def test_width_768_route_is_untouched():
    """A multiple of 256: the same result as before the gate widened, the exact
    column sum rounded once."""
    C = _native.require("colsum")
    torch.manual_seed(3)
    dy = _ints(4100, 768)
    for od in (torch.float32, torch.bfloat16):
        assert torch.equal(C.bias_grad(dy, od), dy.float().sum(0).to(od))


def test_widths_below_the_gate_are_refused():
    C = _native.require("colsum")
    assert not C.colsum_supported(32) and not C.colsum_supported(96) and not C.colsum_supported(0)
    with pytest.raises(RuntimeError):
        C.bias_grad(torch.zeros(8, 96, device=DEV, dtype=torch.bfloat16), torch.float32)
