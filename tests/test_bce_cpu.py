"""ops/loss.py binary_cross_entropy off the GPU: the PyTorch composition against timm's BinaryCrossEntropy
written out in float64, the argument checks, the CLI flags, StepConfig and the pipeline's training loss."""
import pytest
import torch
import torch.nn.functional as F

from distributed_model_parallel_amd.ops.loss import binary_cross_entropy, binary_cross_entropy_with_stats
from tests.dist_utils import run_world
from tests.test_loss_mix import _atoms, _logits

# (e, with target_b, lam, target_thresh)
MODES = [(0.0, False, 1.0, None), (0.1, False, 1.0, None), (0.1, True, 0.3, None), (0.1, True, 0.3, 0.2)]


def timm_bce(x, a, target_b=None, label_smoothing=0.0, lam=1.0, target_thresh=None, sum_classes=False):
    """timm's BinaryCrossEntropy on mixup_target's dense target, in float64 over the valid rows."""
    C, valid = x.shape[1], a != -100
    x, a = x[valid].double(), a[valid]
    b = a if target_b is None else target_b[valid]
    off, on = label_smoothing / C, 1.0 - label_smoothing + label_smoothing / C
    t = (torch.full_like(x, off).scatter_(1, a[:, None], on) * lam
         + torch.full_like(x, off).scatter_(1, b[:, None], on) * (1.0 - lam))
    if target_thresh is not None:
        t = t.gt(target_thresh).double()
    return F.binary_cross_entropy_with_logits(x, t, reduction="sum") / (len(a) * (1 if sum_classes else C))


@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("e,paired,lam,thresh", MODES)
def test_composition_matches_timm(e, paired, lam, thresh, sum_classes):
    x, a, b = _logits()
    a[0], b[2] = -100, a[2]  # an ignored row; both labels on one class
    xa, xr = x.clone().requires_grad_(), x.clone().requires_grad_()
    kw = dict(label_smoothing=e, target_b=b if paired else None, lam=lam, target_thresh=thresh, sum_classes=sum_classes)
    got, ref = binary_cross_entropy(xa, a, **kw), timm_bce(xr, a, **kw)
    torch.testing.assert_close(got.double(), ref, atol=1e-6, rtol=1e-5)
    got.backward()
    ref.backward()
    torch.testing.assert_close(xa.grad, xr.grad, atol=1e-7, rtol=1e-5)
    assert not xa.grad[0].any()
    a[0] = 4  # the statistics form has no ignored rows
    stats = torch.full((3,), 2.0, dtype=torch.float64)
    ls = binary_cross_entropy_with_stats(x, a, 0.25, stats, **kw)
    torch.testing.assert_close(ls.double(), 0.25 * timm_bce(x, a, **kw), atol=1e-6, rtol=1e-5)
    top = x.topk(5, 1).indices
    assert stats.tolist() == [2.0 + float(ls.double()), 2.0 + float((top[:, 0] == a).sum()),
                              2.0 + float((top == a[:, None]).any(1).sum())]


@pytest.mark.parametrize("kw", [dict(target_thresh=1.0), dict(target_thresh=-0.1), dict(label_smoothing=1.0),
                                dict(lam=1.5), dict(target_b=torch.zeros(3, dtype=torch.int64))])
def test_argument_errors(kw):
    x, a, _ = _logits()
    for call in (binary_cross_entropy, lambda *p, **k: binary_cross_entropy_with_stats(*p, 1.0, torch.zeros(3).double(), **k)):
        with pytest.raises(ValueError):
            call(x, a, **kw)


def test_cli_flags_and_parser_errors(capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args(["--bce-loss", "--bce-target-thresh", "0.2", "--bce-sum", "--label-smoothing", "0.1",
                      "--mixup-alpha", "0.8", "--cutmix-alpha", "1.0"])
    check_args(p, a)
    assert (a.bce_loss, a.bce_target_thresh, a.bce_sum) == (True, 0.2, True)
    check_args(p, p.parse_args(["--bce-loss", "--parallel", "pipe"]))
    for argv, msg in ((["--bce-target-thresh", "0.2"], "need --bce-loss"), (["--bce-sum"], "need --bce-loss"),
                      (["--bce-loss", "--bce-target-thresh", "1.0"], "[0, 1)"),
                      (["--bce-loss", "--bce-target-thresh", "-0.1"], "[0, 1)")):
        with pytest.raises(SystemExit):
            check_args(p, p.parse_args(argv))
        assert msg in capsys.readouterr().err


def test_step_config_bce():
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    cfg = StepConfig(model="vit_tiny", parallel="none", dtype=torch.float32, batch_size=4, lr=0.01,
                     channels_last=False, label_smoothing=0.1, bce=True, bce_target_thresh=0.2, bce_sum=True)
    st = build_train_state(cfg, torch.device("cpu"))
    with torch.no_grad():
        out = st.model(st.images)
    ref = timm_bce(out, st.labels, label_smoothing=0.1, target_thresh=0.2, sum_classes=True)
    assert float(st.step().detach()) == pytest.approx(float(ref), rel=1e-5)
    with pytest.raises(ValueError, match="bce=True"):
        build_train_state(StepConfig(model="vit_tiny", parallel="none", bce_sum=True), torch.device("cpu"))


def _pipe_worker(rank, world):
    from distributed_model_parallel_amd.comm.rccl import Communicator
    from distributed_model_parallel_amd.parallel.pipeline import Pipeline
    comm, out = Communicator(torch.device("cpu")), {}
    for name, kw in (("custom", dict(loss_fn=F.cross_entropy, bce=True)), ("needs", dict(bce_target_thresh=0.2))):
        with pytest.raises(ValueError) as e:
            Pipeline(_atoms(), comm, (3, 4, 4), **kw)
        out[name] = str(e.value)
    pipe = Pipeline(_atoms(), comm, (3, 4, 4), micro_batches=2, schedule="1f1b", label_smoothing=0.1, bce=True,
                    bce_target_thresh=0.2)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(12, 3, 4, 4, generator=g), torch.randint(0, 7, (12,), generator=g)
    with torch.no_grad():
        logits = _atoms()(x)
    out["ref_train"] = float(timm_bce(logits, y, label_smoothing=0.1, target_thresh=0.2))
    out["ref_eval"] = float(F.cross_entropy(logits, y))
    out["eval"] = pipe.eval_step(x, y).loss  # before the step: same weights as the reference
    out["train"] = pipe.train_step(x, y).loss
    return out


def test_pipeline_trains_on_bce_and_evaluates_plain():
    r = run_world(_pipe_worker, 1)[0]
    assert "default loss" in r["custom"] and "bce=True" in r["needs"]
    assert r["train"] == pytest.approx(r["ref_train"], rel=1e-5)
    assert r["eval"] == pytest.approx(r["ref_eval"], rel=1e-5)
    assert abs(r["ref_train"] - r["ref_eval"]) > 1e-3  # the two differ: the checks above can tell them apart
