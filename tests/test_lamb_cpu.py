"""LAMB without a GPU: ``_lamb_reference`` through ``MasterLAMB`` against the
float64 oracle at the bounds of tests/test_gpu_lamb.py (so the bounds hold
without the kernel), the trainer's switch, checkpoints, kernel resources."""
import os
import shutil

import pytest
import torch

from distributed_model_parallel_amd.ops.optim import (ForeignOptimizerState, MasterAdamW, MasterLAMB,
                                                      build_optimizer)
from tests.lamb_oracle import HP, SCALES, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(seed=0):
    torch.manual_seed(seed)
    shapes = [(8,), (5, 2), (64, 33), (33,), (3, 8), (24,), (7, 9)]
    ps = [torch.nn.Parameter(torch.randn(s) * SCALES[i % 3]) for i, s in enumerate(shapes)]
    ps[4].data.zero_()  # adapted, zero weights
    return ps


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_reference_matches_oracle(max_norm):
    ps = _params()
    opt = MasterLAMB(ps, max_grad_norm=max_norm, **HP)
    orc = Oracle(ps, [p.dim() > 1 for p in ps], max_norm)
    for t in range(4):
        for i, p in enumerate(ps):
            p.grad.copy_(torch.zeros_like(p) if i in (5, 6) else torch.randn_like(p))  # excluded / adapted, no gradient
        want = orc.step([p.grad for p in ps])
        opt.step()
        got = opt.last_trust_ratios[0].double()
        torch.testing.assert_close(got, want[:, 0], atol=0, rtol=1e-5)
        assert (float(got[4]) == 1.0) == (t == 0) and float(got[5]) == 1.0 and got[6] == pytest.approx(10.0, rel=1e-5)
    for p, w in zip(ps, orc.w):
        torch.testing.assert_close(p.detach().double(), w, atol=1e-5, rtol=1e-5)
    assert (opt.last_grad_norm is None) == (max_norm == 0) and opt.state_dict()["steps"] == 4
    adapted = want[[1, 2, 4, 6], 0]
    assert opt.last_trust_range() == (pytest.approx(float(adapted.min())), pytest.approx(float(adapted.max())))


def test_trainer_switch_and_checkpoints():
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    lamb = build_optimizer("adamw", _params(), False, lr=1e-3, trust_ratio=True)
    assert type(lamb) is MasterLAMB
    ps = _params()
    with pytest.raises(ValueError, match="lr scales"):
        build_optimizer("adamw", ps, False, lr=1e-3, trust_ratio=True, lr_scales={ps[0]: 0.5})
    adamw = MasterAdamW(_params(), lr=1e-3)
    assert lamb.state_dict()["kind"] == "lamb"
    for dst, src in ((adamw, lamb), (lamb, adamw)):
        with pytest.raises(ForeignOptimizerState):
            dst.load_state_dict(src.state_dict())
    p = build_parser()
    a = p.parse_args(["--optimizer", "adamw", "--lamb", "--lr", "3e-3", "--wd", "0.05", "--clip-grad-norm", "1.0"])
    check_args(p, a)
    assert a.lamb and not p.parse_args([]).lamb
    for argv in (["--lamb"], ["--optimizer", "adamw", "--arch", "vit_tiny", "--lamb", "--layer-decay", "0.75"]):
        with pytest.raises(SystemExit):
            check_args(p, p.parse_args(argv))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_lamb_kernel_instantiations_build_without_scratch():
    """lamb_moments_kernel per gradient dtype, lamb_trust_kernel, lamb_flat_kernel
    per P x MASTER x EMA (that pass reads no gradient): the 11 the host launches."""
    import sys
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources
    ks = resources(os.path.join(ROOT, "csrc/optim", "fused_lamb.hip"))
    count = {n: sum(n in k["name"] for k in ks) for n in ("lamb_moments_kernel", "lamb_trust_kernel", "lamb_flat_kernel")}
    assert count == {"lamb_moments_kernel": 2, "lamb_trust_kernel": 1, "lamb_flat_kernel": 8}, [k["name"] for k in ks]
    for k in ks:
        print(k)
        assert k["scratch"] == "0", k
