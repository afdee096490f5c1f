"""One data-parallel training step, shared by bench.py, smoke() and the CLI.

Per step (DDP mode): forward of the local micro-batch (bf16, channels-last),
cross-entropy in fp32, backward with bucketed RCCL all-reduce overlapped by
the C++ reducer, one fused flat SGD launch per dtype group, one fill per
group to zero the gradient buckets.  Nothing is skipped or cached: every step
reads the input batch, runs the full model and updates every parameter.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..models import INPUT_SHAPES, build_model
from ..ops.loss import cross_entropy
from ..ops.optim import build_optimizer
from ..utils.precision import cast_model


@dataclass
class StepConfig:
    model: str = "resnet50"
    batch_size: int = 256            # per GPU
    image_size: Optional[int] = None
    num_classes: Optional[int] = None
    dtype: torch.dtype = torch.bfloat16
    channels_last: bool = True
    parallel: str = "ddp"           # ddp | syncbn | dp | pipe | none
    bucket_cap_mb: float = 25.0
    first_bucket_mb: float = 1.0
    dp_devices: int = 1             # parallel == "dp": GPUs driven by the single process
    dp_replicas: int = 1            # parallel == "dp": replicas per GPU (>1 aliases several
                                    # replicas onto one device, so scatter / replicate /
                                    # parallel_apply / gather / reduce-add all run on 1 GPU)
    graph: bool = False             # capture the whole step in a hipGraph (constant LR, static data)
    lr: float = 0.1
    momentum: float = 0.9
    weight_decay: float = 1e-4
    optimizer: str = "sgd"          # sgd | adamw | lars (ops/optim.py)
    betas: tuple = (0.9, 0.999)     # optimizer == "adamw"
    eps: float = 1e-8               # optimizer == "adamw" / "lars"
    clip_grad_norm: float = 0.0     # optimizer == "adamw": global-norm clipping (0 = off)
    trust_coefficient: float = 1e-3  # optimizer == "lars"
    label_smoothing: float = 0.0    # training loss (ops/loss.py); 0 = plain cross-entropy
    drop_path_rate: float = 0.0     # ViT / ConvNeXt: stochastic depth, linear over the blocks (ops/drop_path.py)
    ema_decay: float = 0.0          # weight EMA inside the optimizer's step kernels (ops/optim.py); 0 = off
    layer_decay: float = 1.0        # optimizer == "adamw", ViT / ConvNeXt: layer-wise lr decay (1 = off)
    seed: int = 0
    micro_batches: int = 8          # parallel == "pipe"
    schedule: str = "1f1b"          # parallel == "pipe": naive | gpipe | 1f1b
    partition: str = "balanced"     # parallel == "pipe": balanced | reference
    checkpoint_segments: int = 0    # activation checkpointing of the block trunk (0 = off)
    dp_graphs: bool = False         # parallel == "dp": replicas as captured hipGraphs (dp_graphs.py)
    pipe_graphs: bool = True        # parallel == "pipe" on GPU: 1F1B micro-batches on captured stage graphs
    extra: dict = field(default_factory=dict)


@dataclass
class TrainState:
    cfg: StepConfig
    model: nn.Module
    wrapped: nn.Module
    optimizer: torch.optim.Optimizer
    step: Callable[[], torch.Tensor]
    images: torch.Tensor
    labels: torch.Tensor


def synthetic_batch(cfg: StepConfig, device: torch.device, generator_seed: int = 1234,
                    batch: Optional[int] = None):
    (c, h, w), ncls = INPUT_SHAPES[cfg.model]
    if cfg.image_size:
        h = w = cfg.image_size
    ncls = cfg.num_classes or ncls
    b = batch or cfg.batch_size
    g = torch.Generator(device="cpu").manual_seed(generator_seed)
    x = torch.randn(b, c, h, w, generator=g).to(device=device, dtype=cfg.dtype)
    if cfg.channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, ncls, (b,), generator=g).to(device)
    return x, y


def _layer_scales(cfg: StepConfig, model: nn.Module):
    """The lr_scales of cfg.layer_decay for the BARE model (its Parameter objects
    survive DDP's re-homing onto the flats); None when the decay is off."""
    if not 0.0 < cfg.layer_decay <= 1.0:
        raise ValueError(f"layer_decay must be in (0, 1], got {cfg.layer_decay}")
    if cfg.layer_decay == 1.0:
        return None
    if cfg.optimizer != "adamw":
        raise ValueError("layer_decay needs optimizer='adamw'")
    from ..models.layer_decay import layer_decay_scales
    return layer_decay_scales(model, cfg.layer_decay)


def _optimizer(cfg: StepConfig, target, flat: bool, lr_scales=None) -> torch.optim.Optimizer:
    return build_optimizer(cfg.optimizer, target, flat, lr=cfg.lr, momentum=cfg.momentum,
                           weight_decay=cfg.weight_decay, betas=cfg.betas, eps=cfg.eps,
                           clip_grad_norm=cfg.clip_grad_norm, trust_coefficient=cfg.trust_coefficient,
                           ema_decay=cfg.ema_decay or None, lr_scales=lr_scales)


def build_train_state(cfg: StepConfig, device: torch.device) -> TrainState:
    if cfg.parallel == "pipe":
        return build_pipeline_state(cfg, device)
    if cfg.graph:
        if device.type != "cuda":
            raise ValueError("graph capture needs a GPU")
        # Build (and later warm up / capture) on ONE side stream: the DDP reducer
        # keeps the parameters' AccumulateGrad nodes alive, and a node created on
        # the default stream would sync against it inside the capture.
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            st = _build_train_state(cfg, device)
        from .graphed import GraphedStep
        # two eager calls, the capture on the third: bench.py's default
        # --warmup 3 then times replays only (with warmup=3 the capture landed
        # in the first timed step and inflated --graph rows by ~3 ms / 10 steps)
        st.step = GraphedStep(st.step, warmup=2, stream=side)
        return st
    return _build_train_state(cfg, device)


def _build_train_state(cfg: StepConfig, device: torch.device) -> TrainState:
    from ..parallel.distributed import DistributedDataParallel
    from ..parallel.sync_batchnorm import SyncBatchNorm

    torch.manual_seed(cfg.seed)
    kw = {}
    if cfg.num_classes:
        kw["num_classes"] = cfg.num_classes
    if cfg.image_size and cfg.model.startswith("vit"):
        kw["image_size"] = cfg.image_size
    if cfg.drop_path_rate:
        if not cfg.model.startswith(("vit", "convnext")):
            raise ValueError(f"--drop-path is for ViT archs only (and convnext_*): drop_path_rate does not apply "
                             f"to {cfg.model}")
        kw["drop_path_rate"] = cfg.drop_path_rate
    model = build_model(cfg.model, **kw)
    if cfg.checkpoint_segments > 1:
        from ..utils.checkpointing import enable_activation_checkpointing
        enable_activation_checkpointing(model, cfg.checkpoint_segments)
    if cfg.parallel == "syncbn":
        model = SyncBatchNorm.convert_sync_batchnorm(model)
    model = model.to(device)
    if cfg.channels_last:
        model = model.to(memory_format=torch.channels_last)
    if cfg.dtype != torch.float32:
        cast_model(model, cfg.dtype)
    scales = _layer_scales(cfg, model)  # on the bare model, before it is wrapped
    ndp = max(1, cfg.dp_devices) if (cfg.parallel == "dp" and device.type == "cuda") else 1
    # DP: the single process feeds batch_size images PER GPU (weak scaling, same
    # per-GPU work as DDP), scattered from device_ids[0]
    x, y = synthetic_batch(cfg, device, batch=cfg.batch_size * ndp)

    if cfg.parallel in ("ddp", "syncbn"):
        wrapped = DistributedDataParallel(model, bucket_cap_mb=cfg.bucket_cap_mb,
                                          first_bucket_mb=cfg.first_bucket_mb,
                                          flat_parameters=True)
        opt = _optimizer(cfg, wrapped, flat=True, lr_scales=scales)

        def step() -> torch.Tensor:
            out = wrapped(x)
            loss = cross_entropy(out, y, label_smoothing=cfg.label_smoothing)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss
    elif cfg.parallel == "dp":
        from ..parallel.data_parallel import DataParallel
        # fp32 master weights + state, one launch per dtype group (same update as DDP's flat optimizer)
        opt = _optimizer(cfg, model.parameters(), flat=False, lr_scales=scales)
        reps = max(1, cfg.dp_replicas)
        wrapped = DataParallel(model, device_ids=[d for d in range(ndp) for _ in range(reps)]
                               if device.type == "cuda" else None, graphs=cfg.dp_graphs)

        def step() -> torch.Tensor:
            out = wrapped(x)
            loss = cross_entropy(out, y, label_smoothing=cfg.label_smoothing)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss
    else:
        wrapped = model
        opt = _optimizer(cfg, model.parameters(), flat=False, lr_scales=scales)

        def step() -> torch.Tensor:
            out = model(x)
            loss = cross_entropy(out, y, label_smoothing=cfg.label_smoothing)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss

    return TrainState(cfg, model, wrapped, opt, step, x, y)


def build_pipeline_state(cfg: StepConfig, device: torch.device) -> TrainState:
    """Pipeline model parallelism across the process group (one stage per rank).

    ``cfg.batch_size`` is the WHOLE batch entering stage 0 (the reference's
    model-parallel run feeds 512 images per step through 4 stages,
    ``model_parallel.py:92``); it is cut into ``cfg.micro_batches`` micro-batches
    scheduled naive / gpipe / 1f1b.  Every stage updates its own slice with the
    same fp32-master optimizer as the data-parallel paths.  ``step()`` returns the
    loss on rank 0 (and a zero tensor elsewhere).
    """
    from ..comm.rccl import default_communicator
    from ..parallel.pipeline import Pipeline

    if cfg.layer_decay != 1.0:
        raise ValueError("layer_decay with parallel='pipe' is not supported (per-stage optimizers see partial models)")
    torch.manual_seed(cfg.seed)  # every rank builds the same full model, keeps its stage
    kw = {"num_classes": cfg.num_classes} if cfg.num_classes else {}
    model = build_model(cfg.model, **kw)
    if not hasattr(model, "as_sequential"):
        raise ValueError(f"--parallel pipe needs a model with as_sequential() (got {cfg.model})")
    (c, h, w), _ = INPUT_SHAPES[cfg.model]
    if cfg.image_size:
        h = w = cfg.image_size
    comm = default_communicator(device)
    pipe = Pipeline(model.as_sequential(), comm, (c, h, w), micro_batches=cfg.micro_batches,
                    schedule=cfg.schedule, device=device, dtype=cfg.dtype,
                    channels_last=cfg.channels_last, partition=cfg.partition,
                    static_batch=cfg.batch_size,  # every rank knows it: no per-step size message
                    label_smoothing=cfg.label_smoothing,
                    # captured stage slots on one GPU only: the multi-stage slot
                    # schedule is verified on the CPU stand-ins (tests/test_pipeline.py)
                    # but never with RCCL between captured stages (a 1-GPU box cannot
                    # host two RCCL ranks), so multi-rank GPU pipelines run eagerly
                    graphs=cfg.pipe_graphs and device.type == "cuda" and comm.size == 1)
    if cfg.clip_grad_norm and comm.size > 1:
        raise ValueError("clip_grad_norm with a multi-stage pipeline needs a cross-stage norm reduction "
                         "(not implemented)")
    opt = _optimizer(cfg, pipe.module.parameters(), flat=False)
    x, y = synthetic_batch(cfg, device) if pipe.is_first else (None, None)
    zero = torch.zeros((), device=device)

    def step() -> torch.Tensor:
        r = pipe.train_step(x, y)
        opt.step()
        opt.zero_grad()
        lt = r.loss_tensor if r.valid else None  # device tensor: no host sync per step
        return lt if lt is not None else zero

    return TrainState(cfg, pipe.module, pipe, opt, step, x, y)
