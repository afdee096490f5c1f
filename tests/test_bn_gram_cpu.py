"""The torch path of BatchNormAct2d(..., out_gram=True) and the bn3 fold with a
precomputed Gram (ops/bn_fold.py a_gram), on the CPU in fp64."""
import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd import _native
from distributed_model_parallel_amd.ops import batchnorm as bnops
from distributed_model_parallel_amd.ops.batchnorm import BatchNormAct2d, batch_norm_act
from distributed_model_parallel_amd.ops.bn_fold import conv1x1_bn_fold
from distributed_model_parallel_amd.ops.conv1x1 import Conv1x1


def _bn(c, seed):
    g = torch.Generator().manual_seed(seed)
    bn = BatchNormAct2d(c, act="relu").double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.3)
    return bn, g


def _rows(t):
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("training", [True, False])
def test_out_gram_torch_path_is_ata(training):
    bn, g = _bn(8, 1)
    bn.train(training)
    x = torch.randn(3, 8, 5, 4, generator=g, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    out, osums, G = bn(x, out_gram=True)
    a2 = _rows(out)
    torch.testing.assert_close(G, a2.t() @ a2)
    torch.testing.assert_close(osums, torch.cat([a2.sum(0), (a2 * a2).sum(0), a2.new_tensor([float(a2.shape[0])])]))
    assert not G.requires_grad and not osums.requires_grad
    torch.testing.assert_close(G.diagonal(), osums[8:16])
    if training:
        assert int(bn.num_batches_tracked) == 1
    # the output and its gradient are those of the plain call
    bn2, _ = _bn(8, 1)
    bn2.train(training)
    x2 = x.detach().clone().requires_grad_(True)
    ref = bn2(x2)
    torch.testing.assert_close(out, ref, rtol=0, atol=0)
    (out * out).sum().backward()
    (ref * ref).sum().backward()
    torch.testing.assert_close(x.grad, x2.grad, rtol=0, atol=0)
    torch.testing.assert_close(bn.weight.grad, bn2.weight.grad, rtol=0, atol=0)


def test_out_gram_functional_2d_rows():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(37, 16, generator=g, dtype=torch.float64)
    out, osums, G = batch_norm_act(x, None, None, None, None, True, 0.1, 1e-5, relu=True, out_gram=True)
    torch.testing.assert_close(G, out.t() @ out)
    assert osums[-1].item() == 37


@pytest.mark.parametrize("downsample", [False, True])
def test_fold_with_and_without_a_gram_identical(downsample):
    def run(give):
        bn2, g = _bn(8, 3)
        conv = Conv1x1(8, 32).double()
        bn3 = BatchNormAct2d(32, act="relu").double()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(32, 8, 1, 1, generator=g, dtype=torch.float64) * 0.5)
        for b in (bn3,):
            b.running_mean = b.running_mean.float()
            b.running_var = b.running_var.float()
        raw = torch.randn(2, 8, 4, 4, generator=g, dtype=torch.float64).contiguous(
            memory_format=torch.channels_last).requires_grad_(True)
        up = torch.randn(2, 32, 4, 4, generator=g, dtype=torch.float64)
        a2, asums, G = bn2(raw, out_gram=True)
        kw = {}
        if downsample:
            cd = Conv1x1(16, 32, 1).double()
            bd = BatchNormAct2d(32).double()
            bd.running_mean, bd.running_var = bd.running_mean.float(), bd.running_var.float()
            with torch.no_grad():
                cd.weight.copy_(torch.randn(32, 16, 1, 1, generator=g, dtype=torch.float64) * 0.5)
            xs = torch.randn(2, 16, 4, 4, generator=g, dtype=torch.float64).contiguous(
                memory_format=torch.channels_last).requires_grad_(True)
            kw = dict(downsample=torch.nn.Sequential(cd, bd), x=xs)
            out = conv1x1_bn_fold(conv, bn3, a2, asums, force=True, a_gram=G if give else None, **kw)
        else:
            res = torch.randn(2, 32, 4, 4, generator=g, dtype=torch.float64).contiguous(
                memory_format=torch.channels_last).requires_grad_(True)
            out = conv1x1_bn_fold(conv, bn3, a2, asums, res, force=True, a_gram=G if give else None)
        (out * up).sum().backward()
        return [out.detach(), raw.grad, conv.weight.grad, bn3.weight.grad, bn3.bias.grad, bn2.weight.grad,
                bn3.running_mean, bn3.running_var]

    for a, b in zip(run(True), run(False)):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_feature_is_listed_and_gated():
    assert "fuse_bn_gram" in _native.FEATURES
    assert set(bnops._GRAM_FUSE_C) <= {64, 128, 256}
    # the torch path never counts as a fused Gram
    n0 = bnops.stats()["fused_gram"]
    bn, g = _bn(64, 4)
    bn(torch.randn(2, 64, 3, 3, generator=g, dtype=torch.float64), out_gram=True)
    assert bnops.stats()["fused_gram"] == n0
