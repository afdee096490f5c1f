"""The argument checks the four flat step entry points share
(csrc/optim/flat_step.h) on the MI355X: ``sgd_flat_step``, ``adamw_flat_step``,
``adamw_flat_step_scaled`` and ``lars_flat_step`` reject the same bad arguments
with the same words, and a rejected call launches nothing -- ``param``,
``master`` and the state flats are bit-equal to clones taken before it.  Flats
of 16 elements: nothing larger is needed to exercise a check."""
import pytest
import torch

from distributed_model_parallel_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 16
LR, WD, B1, B2, EPS, MU = 1e-2, 0.1, 0.9, 0.999, 1e-8, 0.9
BF16, F32 = torch.bfloat16, torch.float32


def _C():
    return _native.require("gpu tests")


def _sgd(a):
    _C().sgd_flat_step(a["master"], a["mom"], a["grad"], a["param"], LR, WD, a.get("momentum", MU), 0.0, False, 1.0,
                       False, a["ema"], a["ema_decay"])


def _adamw(a):
    _C().adamw_flat_step(a["master"], a["exp_avg"], a["exp_avg_sq"], a["grad"], a["param"], None, a["hyper"], LR,
                         B1, B2, EPS, WD, a["ema"], a["ema_decay"])


def _adamw_scaled(a):
    _C().adamw_flat_step_scaled(a["master"], a["exp_avg"], a["exp_avg_sq"], a["grad"], a["param"], None, a["hyper"],
                                a["lr_class"], a["lr_scales"], LR, B1, B2, EPS, WD, a["ema"], a["ema_decay"])


def _lars(a):
    _C().lars_flat_step(a["master"], a["mom"], a["grad"], a["param"], a["items"], a["coef"], LR, MU, a["ema"],
                        a["ema_decay"])


# entry point -> (call, its state flats)
STEPS = {"sgd": (_sgd, ("mom",)), "adamw": (_adamw, ("exp_avg", "exp_avg_sq")),
         "adamw_scaled": (_adamw_scaled, ("exp_avg", "exp_avg_sq")), "lars": (_lars, ("mom",))}
STATE_CASES = [(k, s) for k, (_, states) in STEPS.items() for s in states]


def _args(kind, n=N):
    """Valid arguments of entry point `kind` on fp32 flats of n elements, without master or EMA."""
    g = torch.Generator(device=DEV).manual_seed(3)
    a = {"master": None, "ema": None, "ema_decay": 0.0,
         "grad": torch.randn(n, device=DEV, generator=g), "param": torch.randn(n, device=DEV, generator=g),
         # adamw_prepare's output after one step, no clipping
         "hyper": torch.tensor([1 - B1, 1 - B2, 0.0, 1.0], device=DEV),
         "lr_class": torch.zeros(n // 8, dtype=torch.uint8, device=DEV), "lr_scales": torch.ones(256, device=DEV),
         # one work item over the whole flat, trust 1 and no decay
         "items": torch.tensor([[0, n // 8, 0]] if n else [], dtype=torch.int32, device=DEV).reshape(-1, 3),
         "coef": torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV)}
    for s in STEPS[kind][1]:
        a[s] = torch.zeros(n, device=DEV)
    return a


def _rejects(kind, a, words):
    """The call raises with `words`, and no tensor it was given has changed."""
    before = {k: v.clone() for k, v in a.items() if torch.is_tensor(v)}
    with pytest.raises(RuntimeError, match=words):
        STEPS[kind][0](a)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(a[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), (kind, k)


@pytest.mark.parametrize("kind", STEPS)
def test_common_checks(kind):
    a = _args(kind)
    a["param"] = a["param"].cpu()
    _rejects(kind, a, "GPU")

    a = _args(kind)
    a["grad"] = torch.randn(2 * N, device=DEV)[::2]
    _rejects(kind, a, "contiguous")

    _rejects(kind, _args(kind, 12), "multiple of 8")

    a = _args(kind)
    a["param"] = a["param"].bfloat16()
    _rejects(kind, a, "master")

    a = _args(kind)
    a["master"] = torch.randn(8, device=DEV)
    _rejects(kind, a, "master")
    a["param"] = a["param"].bfloat16()
    _rejects(kind, a, "master")

    a = _args(kind)
    a["ema"], a["ema_decay"] = a["param"], 0.9
    _rejects(kind, a, "ema")
    a["master"] = a["param"].clone()
    a["ema"] = a["master"]
    _rejects(kind, a, "ema")


@pytest.mark.parametrize("kind,state", STATE_CASES)
def test_state_flat_checks(kind, state):
    a = _args(kind)
    a[state] = torch.zeros(8, device=DEV)
    _rejects(kind, a, state)
    a[state] = torch.zeros(N, device=DEV).bfloat16()
    _rejects(kind, a, state)
    a[state] = torch.zeros(N)
    _rejects(kind, a, state)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_checks_mom_whatever_the_momentum(momentum):
    a = _args("sgd")
    a["momentum"] = momentum
    a["mom"] = torch.zeros(8, device=DEV)
    _rejects("sgd", a, "mom")
    a["mom"] = torch.zeros(N, device=DEV)
    _sgd(a)  # a full one passes


@pytest.mark.parametrize("kind", STEPS)
@pytest.mark.parametrize("pdtype,master", [(F32, False), (BF16, True)])
def test_valid_calls_empty_and_one_vector(kind, pdtype, master):
    for n in (0, 8):
        a = _args(kind, n)
        if master:
            a["master"] = a["param"].clone()
            a["param"] = a["param"].to(pdtype)
        a["ema"], a["ema_decay"] = (a["master"] if master else a["param"]).clone(), 0.5
        before = {k: a[k].clone() for k in ("param", "master", "ema", *STEPS[kind][1]) if a[k] is not None}
        STEPS[kind][0](a)
        torch.cuda.synchronize()
        for k, v in before.items():
            assert a[k].shape == v.shape and bool(torch.isfinite(a[k].float()).all()), (kind, n, k)
            if n and a[k].dtype == F32:  # every fp32 output moved everywhere: the gradient is nowhere 0
                assert bool((a[k] != v).all()), (kind, n, k)
        if master:  # the working copy is the master, rounded
            assert torch.equal(a["param"], a["master"].bfloat16()), (kind, n)
