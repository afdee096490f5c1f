"""BN apply + ReLU that also forms the Gram matrix of its output
(csrc/bn/bn_apply_gram.hip) on MI355X.

1. the kernel against the two launches it replaces: `a`, mean, invstd, the
   running statistics and the step counter bit-identical to
   bn_forward_apply(out_moments); the column moments and G against fp64 sums
   of that reference `a` (G within the TN GEMM's bound of
   tests/test_gpu_gemm_tn_xl.py, the moments within the bound of
   tests/test_gpu_bn_fold.py::test_bn_apply_out_moments);
2. rows past a slab's end must enter G as zeros, not as relu(shift);
3. exact small-integer products through the BN coefficients;
4. a Bottleneck forward + backward with the feature on and off."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import batchnorm as bnops
from distributed_model_parallel_amd.ops import bn_fold

pytestmark = pytest.mark.gpu
DEV = "cuda"
CS = (64, 128, 256)
MS = (1, 63, 64, 65, 129, 1000, 4099, 70001)


@functools.lru_cache(maxsize=None)
def _case(C, M):
    """Inputs and the two-pass reference of one (C, M), computed once."""
    K = _native.require("bn apply gram")
    g = torch.Generator(device=DEV).manual_seed(1000 * C + M)
    x = (torch.randn(M, C, device=DEV, generator=g) * 2 + 0.5).bfloat16()
    w = torch.randn(C, device=DEV, generator=g)          # negative weights included
    b = torch.randn(C, device=DEV, generator=g) * 0.5
    rm = torch.randn(C, device=DEV, generator=g)
    rv = torch.rand(C, device=DEV, generator=g) + 0.5
    sums = K.bn_local_moments(x, C)
    rm0, rv0 = rm.clone(), rv.clone()
    nbt0 = torch.tensor(7, device=DEV, dtype=torch.int64)
    a, mean, inv, osums = K.bn_forward_apply(x, sums, w, b, rm0, rv0, 0.1, 1e-5, None, True, C, nbt0, True)
    ad = a.double()
    return dict(x=x, w=w, b=b, rm=rm, rv=rv, sums=sums, a=a, mean=mean, inv=inv, rm0=rm0, rv0=rv0, nbt0=nbt0,
                s1=ad.sum(0), s2=(ad * ad).sum(0), G=ad.t() @ ad)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("C", CS)
def test_apply_gram_matches_two_pass(C, M):
    K = _native.require("bn apply gram")
    r = _case(C, M)
    rm, rv = r["rm"].clone(), r["rv"].clone()
    nbt = torch.tensor(7, device=DEV, dtype=torch.int64)
    a, mean, inv, osums, G = K.bn_forward_apply_gram(r["x"], r["sums"], r["w"], r["b"], rm, rv, 0.1, 1e-5, C, nbt)
    # bit-identical to the unfused apply
    assert torch.equal(a, r["a"])
    assert torch.equal(mean, r["mean"]) and torch.equal(inv, r["inv"])
    assert torch.equal(rm, r["rm0"]) and torch.equal(rv, r["rv0"])
    assert int(nbt) == 8 and int(r["nbt0"]) == 8       # one step per call
    # moments: the bound of test_bn_apply_out_moments
    assert osums.dtype == torch.float64 and osums.shape == (2 * C + 1,)
    torch.testing.assert_close(osums[:C], r["s1"], rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(osums[C:2 * C], r["s2"], rtol=1e-5, atol=1e-3)
    assert osums[2 * C].item() == M
    # G: the TN GEMM's bound
    atol = 1e-3 * M ** 0.5
    assert G.dtype == torch.float32 and G.shape == (C, C)
    torch.testing.assert_close(G.double(), r["G"], atol=atol, rtol=1e-2)
    torch.testing.assert_close(G, G.t().contiguous(), atol=atol, rtol=1e-2)
    torch.testing.assert_close(G.diagonal().double(), osums[C:2 * C], atol=atol, rtol=1e-2)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("C", CS)
def test_long_slabs_run_the_main_loop(C, blocks):
    """Few blocks over M = 4099: 65 / 22 steps per block, so the peeled pair,
    several iterations of the two-step loop and the checked tail all run (the
    default grids give a block at most 5 steps at the sizes above)."""
    K = _native.require("bn apply gram")
    M = 4099
    r = _case(C, M)
    K.set_bn_gram_blocks(blocks)
    try:
        a, mean, inv, osums, G = K.bn_forward_apply_gram(r["x"], r["sums"], r["w"], r["b"], None, None, 0.1, 1e-5, C)
    finally:
        K.set_bn_gram_blocks(0)
    assert torch.equal(a, r["a"]) and torch.equal(mean, r["mean"]) and torch.equal(inv, r["inv"])
    torch.testing.assert_close(osums[:C], r["s1"], rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(osums[C:2 * C], r["s2"], rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(G.double(), r["G"], atol=1e-3 * M ** 0.5, rtol=1e-2)
    # integers: exact whatever the number of steps
    x = torch.randint(-3, 4, (M, C), device=DEV, generator=torch.Generator(device=DEV).manual_seed(C)).bfloat16()
    sums = torch.zeros(2 * C + 1, device=DEV, dtype=torch.float64)
    sums[C:] = M
    w = torch.full((C,), 2.0, device=DEV)
    b = torch.ones(C, device=DEV)
    K.set_bn_gram_blocks(blocks)
    try:
        a, _, _, _, G = K.bn_forward_apply_gram(x, sums, w, b, None, None, 0.1, 0.0, C)
    finally:
        K.set_bn_gram_blocks(0)
    ref = torch.relu(x.float() * 2 + 1)
    assert torch.equal(a.float(), ref) and torch.equal(G.double(), ref.double().t() @ ref.double())


@pytest.mark.parametrize("C", CS)
def test_padding_rows_enter_as_zeros(C):
    """M = 65: one whole step and one row; with relu(shift) > 0 in every
    channel, 63 tail rows entering the tile as relu(shift) would show in G."""
    K = _native.require("bn apply gram")
    M = 65
    g = torch.Generator(device=DEV).manual_seed(C)
    x = (torch.randn(M, C, device=DEV, generator=g) * 2 + 0.5).bfloat16()
    w = torch.randn(C, device=DEV, generator=g)
    b = torch.rand(C, device=DEV, generator=g) + 20.0
    sums = K.bn_local_moments(x, C)
    a, _, _, osums, G = K.bn_forward_apply_gram(x, sums, w, b, None, None, 0.1, 1e-5, C)
    assert float(a.min()) > 0
    ad = a.double()
    torch.testing.assert_close(G.double(), ad.t() @ ad, atol=1e-3 * M ** 0.5, rtol=1e-2)
    torch.testing.assert_close(osums[:C], ad.sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("M", [64, 65, 640, 1000])
@pytest.mark.parametrize("C", CS)
def test_apply_gram_exact_pattern(C, M):
    """Integer x in [-3, 3]; hand-built moments give mean 0, var 1 (eps 0), so
    scale = weight (a power of two) and shift = bias (an integer): every value
    of `a` and every product and partial sum of G is exact in fp32."""
    K = _native.require("bn apply gram")
    g = torch.Generator(device=DEV).manual_seed(7 * C + M)
    x = torch.randint(-3, 4, (M, C), device=DEV, generator=g).bfloat16()
    w = torch.tensor([0.5, 1.0, 2.0, -1.0, -2.0], device=DEV)[torch.randint(0, 5, (C,), device=DEV, generator=g)]
    b = torch.randint(-2, 3, (C,), device=DEV, generator=g).float()
    sums = torch.zeros(2 * C + 1, device=DEV, dtype=torch.float64)
    sums[C:2 * C] = M
    sums[2 * C] = M
    a, mean, inv, osums, G = K.bn_forward_apply_gram(x, sums, w, b, None, None, 0.1, 0.0, C)
    ref = torch.relu(x.float() * w + b)
    assert torch.equal(a.float(), ref)
    assert torch.equal(mean, torch.zeros_like(mean)) and torch.equal(inv, torch.ones_like(inv))
    assert torch.equal(G, ref.t() @ ref)
    assert torch.equal(G.double(), ref.double().t() @ ref.double())
    assert torch.equal(osums[:C], ref.double().sum(0)) and torch.equal(osums[C:2 * C], (ref.double() ** 2).sum(0))


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@pytest.mark.parametrize("n,cin,hw,planes", [(8, 64, 56, 64), (4, 512, 28, 128)])
def test_bottleneck_fused_gram_on_off(n, cin, hw, planes, monkeypatch):
    """One Bottleneck, forward + backward, with the Gram formed inside bn2's
    apply pass and by the TN GEMM: both against the fp32 stock block, within
    the bounds tests/test_gpu_bn_fold.py uses for fold vs. no fold."""
    import copy
    from distributed_model_parallel_amd.models.resnet import Bottleneck
    from distributed_model_parallel_amd.ops.batchnorm import BatchNormAct2d
    from distributed_model_parallel_amd.ops.conv1x1 import Conv1x1
    from distributed_model_parallel_amd.utils.precision import cast_model
    torch.manual_seed(5)
    cout = planes * 4
    down = torch.nn.Sequential(Conv1x1(cin, cout, 1), BatchNormAct2d(cout)) if cin != cout else None
    base = Bottleneck(cin, planes, 1, down).to(DEV)
    net = cast_model(copy.deepcopy(base).to(memory_format=torch.channels_last))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, BatchNormAct2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    off = copy.deepcopy(net)
    f32 = copy.deepcopy(net).float()
    for m in (net, off, f32):
        m.train()
    x = torch.relu(torch.randn(n, cin, hw, hw, device=DEV)).bfloat16().contiguous(memory_format=torch.channels_last)
    g = torch.randn(n, cout, hw, hw, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)

    def run(model, dtype):
        xi = x.to(dtype).clone().requires_grad_(True)
        y = model(xi)
        y.backward(g.to(dtype))
        return [y.float(), xi.grad.float()] + [p.grad.float() for p in model.parameters()]

    monkeypatch.setattr(bnops, "_FUSE_GRAM", True)
    c0, f0, t0 = bnops.stats()["fused_gram"], bn_fold.stats()["fold_gram_given"], bnops.stats()["torch_fwd"]
    got = run(net, torch.bfloat16)
    assert bnops.stats()["fused_gram"] == c0 + 1, "one fused Gram per block"
    assert bn_fold.stats()["fold_gram_given"] == f0 + 1
    assert bnops.stats()["torch_fwd"] == t0, "torch fallback on the GPU"
    monkeypatch.setattr(bnops, "_FUSE_GRAM", False)
    unf = run(off, torch.bfloat16)
    assert bnops.stats()["fused_gram"] == c0 + 1 and bn_fold.stats()["fold_gram_given"] == f0 + 1
    with _native.reference_mode():
        gold = run(f32, torch.float32)
    names = ["out", "x.grad"] + [k for k, _ in net.named_parameters()]
    for k, a, b, r in zip(names, got, unf, gold):
        e_on, e_off = _rel(a, r), _rel(b, r)
        assert e_on < max(1.3 * e_off, 1e-2), f"{k}: fused Gram {e_on:.4f} vs two launches {e_off:.4f} (fp32 reference)"
    for (k, b1), (_, b2) in zip(net.named_buffers(), off.named_buffers()):
        if b1.dtype.is_floating_point:
            assert _rel(b1, b2) < 2e-2, k
        else:
            assert torch.equal(b1, b2), k


_CHILD = """
import torch
from distributed_model_parallel_amd.models.resnet import Bottleneck
from distributed_model_parallel_amd.ops import batchnorm as bnops, bn_fold
from distributed_model_parallel_amd.utils.precision import cast_model
net = cast_model(Bottleneck(256, 64).to("cuda").to(memory_format=torch.channels_last)).train()
x = torch.randn(2, 256, 16, 16, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
net(x.requires_grad_(True)).float().sum().backward()
torch.cuda.synchronize()
print("COUNTS", bn_fold.stats()["fold"], bnops.stats()["fused_gram"], bn_fold.stats()["fold_gram_given"])
"""


def test_disable_feature_in_child_process():
    """DMP_DISABLE=fuse_bn_gram: the fold still runs, no fused Gram."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DMP_DISABLE="fuse_bn_gram")
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("COUNTS")][-1].split()
    assert int(line[1]) == 1 and int(line[2]) == 0 and int(line[3]) == 0, r.stdout
