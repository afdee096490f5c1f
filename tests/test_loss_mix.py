"""Label smoothing and mixup / CutMix targets (ops/loss.py), batch mixing
(ops/mix.py), their CLI flags and the pipeline's smoothed training loss -- the
CPU side: the PyTorch compositions, the host-drawn plans and the argument checks."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_model_parallel_amd.ops.loss import cross_entropy, cross_entropy_with_stats
from distributed_model_parallel_amd.ops.mix import BatchMixer, batch_mix
from tests.dist_utils import run_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logits(B=9, C=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * 3
    a = torch.randint(0, C, (B,), generator=g)
    b = torch.randint(0, C, (B,), generator=g)
    return x, a, b


# ---------------------------------------------------------------- cross-entropy
def test_label_smoothing_matches_torch():
    x, a, _ = _logits()
    xa, xr = x.clone().requires_grad_(), x.clone().requires_grad_()
    la = cross_entropy(xa, a, label_smoothing=0.1)
    lr = F.cross_entropy(xr, a, label_smoothing=0.1)
    torch.testing.assert_close(la, lr, atol=1e-6, rtol=1e-6)
    la.backward()
    lr.backward()
    torch.testing.assert_close(xa.grad, xr.grad, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("e", [0.0, 0.1])
def test_paired_targets_match_the_two_term_sum(e):
    x, a, b = _logits()
    b[2] = a[2]
    got = cross_entropy(x, a, label_smoothing=e, target_b=b, lam=0.3)
    ref = 0.3 * F.cross_entropy(x, a, label_smoothing=e) + 0.7 * F.cross_entropy(x, b, label_smoothing=e)
    torch.testing.assert_close(got, ref, atol=1e-6, rtol=1e-6)


def test_paired_targets_row_formula_with_an_ignored_row():
    """The row formula of the kernels in float64; a row is ignored iff its first label is."""
    x, a, b = _logits(seed=3)
    a[4] = -100
    e, l = 0.1, 0.3
    xd = x.double()
    valid = a != -100
    ac, bc = a.clamp(min=0), b
    rows = (torch.logsumexp(xd, 1) - (1 - e) * (l * xd.gather(1, ac[:, None])[:, 0]
                                                + (1 - l) * xd.gather(1, bc[:, None])[:, 0]) - e * xd.mean(1))
    ref = rows[valid].sum() / valid.sum()
    got = cross_entropy(x, a, label_smoothing=e, target_b=b, lam=l)
    assert abs(float(got) - float(ref)) < 1e-5


def test_defaults_are_the_plain_loss_exactly():
    x, a, _ = _logits()
    a[1] = -100
    assert torch.equal(cross_entropy(x, a, label_smoothing=0.0, target_b=None), cross_entropy(x, a))
    assert torch.equal(cross_entropy(x, a), F.cross_entropy(x, a))
    s0, s1 = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    a[1] = 0
    l0 = cross_entropy_with_stats(x, a, 0.5, s0)
    l1 = cross_entropy_with_stats(x, a, 0.5, s1, label_smoothing=0.0, target_b=None, lam=1.0)
    assert torch.equal(l0, l1) and torch.equal(s0, s1)


def test_with_stats_counts_follow_the_first_label():
    x, a, b = _logits(B=16, C=9, seed=5)
    s = torch.zeros(3, dtype=torch.float64)
    loss = cross_entropy_with_stats(x, a, 0.25, s, label_smoothing=0.1, target_b=b, lam=0.6)
    ref = 0.25 * (0.6 * F.cross_entropy(x, a, label_smoothing=0.1) + 0.4 * F.cross_entropy(x, b, label_smoothing=0.1))
    torch.testing.assert_close(loss, ref, atol=1e-6, rtol=1e-6)
    assert float(s[0]) == pytest.approx(float(ref), abs=1e-6)
    top = x.topk(5, 1).indices
    assert float(s[1]) == float((top[:, 0] == a).sum())
    assert float(s[2]) == float((top == a[:, None]).any(1).sum())


@pytest.mark.parametrize("kw", [dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(lam=1.5),
                                dict(lam=-0.1), dict(target_b="short"), dict(target_b="int32")])
def test_argument_errors(kw):
    x, a, b = _logits()
    if kw.get("target_b") == "short":
        kw = dict(target_b=b[:-1])
    elif kw.get("target_b") == "int32":
        kw = dict(target_b=b.int())
    with pytest.raises(ValueError):
        cross_entropy(x, a, **kw)
    with pytest.raises(ValueError):
        cross_entropy_with_stats(x, a, 1.0, torch.zeros(3, dtype=torch.float64), **kw)


# ---------------------------------------------------------------- BatchMixer
def _plans(mixer, n=20, B=8, H=32, W=24):
    return [mixer.plan(B, H, W) for _ in range(n)]


def _same(p, q):
    return (p.kind == q.kind and p.lam == q.lam and p.box == q.box
            and (p.perm is None) == (q.perm is None) and (p.perm is None or np.array_equal(p.perm, q.perm)))


def test_mixer_plans_depend_on_seed_rank_epoch_only():
    def draw(seed, rank, epoch):
        m = BatchMixer(0.8, 1.0, seed=seed, rank=rank)
        m.set_epoch(epoch)
        return _plans(m)
    base = draw(3, 1, 2)
    assert all(_same(p, q) for p, q in zip(base, draw(3, 1, 2)))
    m = BatchMixer(0.8, 1.0, seed=3, rank=1)
    m.set_epoch(5)
    _plans(m, 7)
    m.set_epoch(2)  # a resumed run: back to the epoch's stream
    assert all(_same(p, q) for p, q in zip(base, _plans(m)))
    for other in (draw(3, 0, 2), draw(3, 1, 3), draw(4, 1, 2)):
        assert not all(_same(p, q) for p, q in zip(base, other))
    assert {p.kind for p in base} == {"mixup", "cutmix"}


def test_cutmix_boxes_are_inside_and_lam_is_the_kept_area():
    m = BatchMixer(0.0, 1.0, seed=1)
    H, W = 13, 22
    plans = _plans(m, 300, 6, H, W)
    assert all(p.kind == "cutmix" for p in plans)
    for p in plans:
        y0, y1, x0, x1 = p.box
        assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
        assert p.lam == 1.0 - ((y1 - y0) * (x1 - x0)) / (H * W)
        assert sorted(p.perm.tolist()) == list(range(6)) and p.perm.dtype == np.int64
    assert any(p.box[0] == 0 or p.box[2] == 0 for p in plans)  # clipped boxes occur
    assert len({p.box for p in plans}) > 100


def test_mixup_lam_is_beta_distributed():
    """Beta(1, 1) is uniform: the mean of 2000 draws has a standard deviation of
    0.2887 / sqrt(2000) = 0.0065, so 0.05 is more than seven of them (the numpy
    generator alone, seeds 0..9: |mean - 0.5| <= 0.012)."""
    m = BatchMixer(1.0, 0.0, seed=0)
    lams = [m.plan(4, 8, 8).lam for _ in range(2000)]
    assert all(0.0 <= v <= 1.0 for v in lams)
    assert abs(sum(lams) / len(lams) - 0.5) < 0.05
    assert np.std(lams) > 0.2


def test_mixer_prob_zero_never_mixes():
    m = BatchMixer(0.8, 1.0, prob=0.0)
    x, y = torch.randn(4, 3, 8, 8), torch.arange(4)
    for _ in range(20):
        xm, ya, yb, lam = m(x, y)
        assert xm is x and ya is y and yb is None and lam == 1.0
    off = BatchMixer(0.0, 0.0)
    assert off(x, y)[0] is x
    half = BatchMixer(1.0, 0.0, prob=0.5, seed=2)
    kinds = [p.kind for p in _plans(half, 200)]
    assert 60 < kinds.count("none") < 140


def test_mixer_call_applies_its_plan():
    twin = BatchMixer(0.8, 1.0, seed=7)
    m = BatchMixer(0.8, 1.0, seed=7)
    x, y = torch.randn(6, 3, 10, 12), torch.randint(0, 5, (6,))
    for _ in range(6):
        p = twin.plan(6, 10, 12)
        xm, ya, yb, lam = m(x, y)
        perm = torch.from_numpy(p.perm)
        assert torch.equal(xm, batch_mix(x, perm, p.lam, p.box))
        assert ya is y and torch.equal(yb, y[perm]) and lam == p.lam


# ---------------------------------------------------------------- batch_mix (CPU composition)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_mix_cpu(dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 3, 6, 7, generator=g).to(dtype)
    x0 = x.clone()
    perm = torch.tensor([2, 0, 1, 3, 4])
    out = batch_mix(x, perm, 0.4, (1, 4, 2, 7))
    ref = x.clone()
    for i in range(5):
        ref[i, :, 1:4, 2:7] = x[perm[i], :, 1:4, 2:7]
    assert torch.equal(out, ref)
    assert torch.equal(batch_mix(x, perm, 0.4, (2, 2, 0, 7)), x)  # empty box
    assert torch.equal(batch_mix(x, perm, 0.4, (0, 6, 0, 7)), x[perm])  # the whole image
    mix = batch_mix(x, perm, 0.25)
    assert mix.dtype == dtype
    assert torch.equal(mix, (0.25 * x.float() + 0.75 * x[perm].float()).to(dtype))
    assert torch.equal(batch_mix(x, perm, 1.0), x)
    assert torch.equal(x, x0)
    for bad in ((0, 7, 0, 7), (3, 2, 0, 7), (0, 6, -1, 7), (0, 6, 0)):
        with pytest.raises(ValueError):
            batch_mix(x, perm, 0.5, bad)
    with pytest.raises(ValueError):
        batch_mix(x, perm, 1.5)
    with pytest.raises(ValueError):
        batch_mix(x, perm[:-1], 0.5)


# ---------------------------------------------------------------- CLI
def test_cli_flags_and_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args([])
    check_args(p, a)
    assert (a.label_smoothing, a.mixup_alpha, a.cutmix_alpha, a.mix_prob) == (0.0, 0.0, 0.0, 1.0)
    a = p.parse_args(["--label-smoothing", "0.1", "--mixup-alpha", "0.8", "--cutmix-alpha", "1.0", "--mix-prob", "0.5"])
    check_args(p, a)
    assert (a.label_smoothing, a.mixup_alpha, a.cutmix_alpha, a.mix_prob) == (0.1, 0.8, 1.0, 0.5)
    check_args(p, p.parse_args(["--label-smoothing", "0.1", "--parallel", "pipe"]))  # smoothing may pipeline
    for argv, msg in ((["--label-smoothing", "1.0"], "[0, 1)"),
                      (["--label-smoothing", "-0.1"], "[0, 1)"),
                      (["--mixup-alpha", "-1"], "negative"),
                      (["--cutmix-alpha", "-0.5"], "negative"),
                      (["--mixup-alpha", "0.8", "--mix-prob", "1.5"], "[0, 1]"),
                      (["--mix-prob", "0.5"], "needs --mixup-alpha"),
                      (["--mixup-alpha", "0.8", "--parallel", "pipe"], "--parallel pipe"),
                      (["--cutmix-alpha", "1.0", "--parallel", "pipe"], "--parallel pipe")):
        with pytest.raises(SystemExit) as e:
            check_args(p, p.parse_args(argv))
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_cli_trains_with_smoothing_and_mixing(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(30000 + os.getpid() % 1000), PYTHONPATH=ROOT)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", "--parallel", "none",
                        "--arch", "mobilenetv2", "--synthetic", "-b", "8", "--epochs", "1", "--steps-per-epoch", "2",
                        "--label-smoothing", "0.1", "--mixup-alpha", "0.8", "--cutmix-alpha", "1.0",
                        "--lr", "0.05", "--warmup-epochs", "0",
                        "--log-dir", str(tmp_path / "log"), "-j", "0", "--checkpoint", str(tmp_path / "ck.pth")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()
    assert len(lines) == 1
    rec = dict(f.split(":", 1) for f in lines[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, lines[0]
    assert math.isfinite(float(rec["loss_val"])), lines[0]


def test_step_config_label_smoothing():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    assert StepConfig().label_smoothing == 0.0

    def first_loss(e):
        cfg = StepConfig(model="vit_tiny", parallel="none", dtype=torch.float32, batch_size=4, lr=0.01,
                         channels_last=False, label_smoothing=e)
        st = build_train_state(cfg, torch.device("cpu"))
        with torch.no_grad():
            out = st.model(st.images)
        return float(st.step().detach()), float(F.cross_entropy(out.float(), st.labels, label_smoothing=e))
    for e in (0.0, 0.1):
        got, ref = first_loss(e)
        assert got == pytest.approx(ref, rel=1e-5)


# ---------------------------------------------------------------- build
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_loss_and_mix_kernels_build_without_scratch():
    """Every instantiation (plain / soft, fp32 / bf16; mixup / CutMix, vector / scalar) for gfx950."""
    from tools.kernel_resources import resources  # (c++filt leaves the bf16 names mangled: match by substring)
    ce = resources(os.path.join(ROOT, "csrc", "loss", "cross_entropy.hip"))
    mix = resources(os.path.join(ROOT, "csrc", "data", "batch_mix.hip"))
    assert len([k for k in ce if "ce_fwd_kernel" in k["name"]]) == 4
    assert len([k for k in ce if "ce_bwd_kernel" in k["name"]]) == 4
    assert len([k for k in mix if "batch_mix_kernel" in k["name"]]) == 8
    bad = [(k["name"], k["scratch"]) for k in ce + mix if k["scratch"] != "0"]
    assert not bad, bad


# ---------------------------------------------------------------- pipeline
def _atoms():
    torch.manual_seed(0)
    return nn.Sequential(nn.Sequential(nn.Flatten(), nn.Linear(48, 32), nn.ReLU()), nn.Linear(32, 7))


def _pipe_worker(rank, world, smoothing, micro):
    from distributed_model_parallel_amd.comm.rccl import Communicator
    from distributed_model_parallel_amd.parallel.pipeline import Pipeline
    comm = Communicator(torch.device("cpu"))
    out = {}
    try:
        Pipeline(_atoms(), comm, (3, 4, 4), loss_fn=F.cross_entropy, label_smoothing=0.1)
    except ValueError as e:
        out["custom"] = str(e)
    try:
        Pipeline(_atoms(), comm, (3, 4, 4), label_smoothing=1.0)
    except ValueError as e:
        out["range"] = str(e)
    pipe = Pipeline(_atoms(), comm, (3, 4, 4), micro_batches=micro, schedule="1f1b", label_smoothing=smoothing)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(12, 3, 4, 4, generator=g), torch.randint(0, 7, (12,), generator=g)
    ref_model = _atoms()
    with torch.no_grad():
        logits = ref_model(x)
    out["ref_train"] = float(F.cross_entropy(logits, y, label_smoothing=smoothing))
    out["ref_eval"] = float(F.cross_entropy(logits, y))
    out["eval"] = pipe.eval_step(x, y).loss  # before the step: same weights as the reference
    out["train"] = pipe.train_step(x, y).loss
    (F.cross_entropy(ref_model(x), y, label_smoothing=smoothing)).backward()
    out["grad_err"] = max(float((p.grad - q.grad).abs().max())
                          for p, q in zip(pipe.module.parameters(), ref_model.parameters()))
    return out


@pytest.mark.parametrize("micro", [1, 3])
def test_pipeline_label_smoothing_trains_smoothed_and_evaluates_plain(micro):
    r = run_world(_pipe_worker, 1, 0.1, micro)[0]
    assert "default loss" in r["custom"] and "[0, 1)" in r["range"]
    assert r["train"] == pytest.approx(r["ref_train"], rel=1e-5)
    assert r["eval"] == pytest.approx(r["ref_eval"], rel=1e-5)
    assert abs(r["ref_train"] - r["ref_eval"]) > 1e-3  # the two differ: the check above can tell them apart
    assert r["grad_err"] < 1e-6
