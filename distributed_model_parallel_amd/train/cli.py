"""Training CLI: data parallel (DDP / single-process DP) and pipeline model
parallel, flag-compatible with the reference scripts.

Reference entry points (§5.6):
  ``python model_parallel.py DIR --world-size 4 --dist-url tcp://127.0.0.1:1224
  --dist-backend nccl --lr 0.4 --epochs 90 -type Imagenet -b 512 -j 12 --wd 1e-4
  --momentum 0.9`` and ``python data_parallel.py --lr 0.4 [-r]``.

Equivalents here::

  torchrun --nproc-per-node 8 -m distributed_model_parallel_amd.train.cli DIR \\
      --parallel ddp --arch resnet50 -type Imagenet -b 256 --epochs 90
  python -m distributed_model_parallel_amd.train.cli --parallel dp --arch mobilenetv2 \\
      -type CIFAR10 DIR -b 512 -r
  python -m distributed_model_parallel_amd.train.cli --parallel pipe --world-size 4 \\
      --arch mobilenetv2 -type CIFAR10 DIR --micro-batches 8 --schedule 1f1b

``--synthetic`` (or no DIR) trains on synthetic data of the dataset's shape.
Honoured flags the reference parsed but ignored (defect 4): ``-b``, ``-j``,
``-type`` and ``DIR``.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F


TRUST_COEFFICIENT = 1e-3  # --trust-coefficient when the flag is absent
_VIT_PATCH = {"vit_b_16": 16, "vit_tiny": 8}  # --image-size must be a multiple of it


def _betas(text: str):
    try:
        b1, b2 = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected B1,B2 (two numbers), got {text!r}")
    return b1, b2


def check_args(parser: argparse.ArgumentParser, args) -> None:
    """Flag combinations that cannot run (parser errors, before any process starts)."""
    if args.clip_grad_norm < 0:
        parser.error("--clip-grad-norm must not be negative")
    if args.clip_grad_norm and args.optimizer != "adamw":
        parser.error("--clip-grad-norm needs --optimizer adamw")
    if args.trust_coefficient is not None and args.optimizer != "lars":
        parser.error("--trust-coefficient needs --optimizer lars")
    if args.trust_coefficient is None:
        args.trust_coefficient = TRUST_COEFFICIENT
    if args.trust_coefficient <= 0:
        parser.error("--trust-coefficient must be positive")
    if not 0.0 <= args.label_smoothing < 1.0:
        parser.error("--label-smoothing must be in [0, 1)")
    if args.mixup_alpha < 0 or args.cutmix_alpha < 0:
        parser.error("--mixup-alpha / --cutmix-alpha must not be negative")
    mixing = args.mixup_alpha > 0 or args.cutmix_alpha > 0
    if args.mix_prob is not None and not mixing:
        parser.error("--mix-prob needs --mixup-alpha or --cutmix-alpha")
    if args.mix_prob is None:
        args.mix_prob = 1.0
    if not 0.0 <= args.mix_prob <= 1.0:
        parser.error("--mix-prob must be in [0, 1]")
    if mixing and args.parallel == "pipe":
        parser.error("--mixup-alpha / --cutmix-alpha with --parallel pipe is not supported "
                     "(images enter at stage 0, labels are used at the last stage)")
    if not 0.0 <= args.drop_path < 1.0:
        parser.error("--drop-path must be in [0, 1)")
    if args.drop_path > 0:
        if not args.arch.startswith(("vit", "convnext")):
            parser.error(f"--drop-path is for ViT archs only (vit_b_16, vit_tiny) and ConvNeXt (convnext_*), "
                         f"not --arch {args.arch}")
    if args.image_size is not None:
        if not args.arch.startswith("vit"):
            parser.error(f"--image-size is for ViT archs only (vit_b_16, vit_tiny), not --arch {args.arch}")
        patch = _VIT_PATCH.get(args.arch, 16)
        if args.image_size < patch or args.image_size % patch:
            parser.error(f"--image-size must be a positive multiple of the patch size {patch} of {args.arch}")
        if args.parallel == "pipe":
            parser.error("--image-size with --parallel pipe is not supported")
    if not 0.0 <= args.model_ema_decay < 1.0:
        parser.error("--model-ema-decay must be in [0, 1)")
    if args.model_ema_warmup and not args.model_ema_decay:
        parser.error("--model-ema-warmup needs --model-ema-decay")
    if args.model_ema_decay and args.parallel == "pipe":
        parser.error("--model-ema-decay with --parallel pipe is not supported "
                     "(per-stage optimizers and eval_step do not carry the average)")
    if args.init_from_ema and not args.init_from:
        parser.error("--init-from-ema needs --init-from")
    if args.init_from:
        if not os.path.exists(args.init_from):
            parser.error(f"--init-from: no such file {args.init_from}")
        if args.resume and os.path.exists(args.checkpoint):
            parser.error(f"--init-from and --resume from an existing checkpoint ({args.checkpoint}) "
                         "are mutually exclusive")
        if args.parallel == "pipe":
            parser.error("--init-from with --parallel pipe is not supported")
    if args.reset_head and not args.init_from:
        parser.error("--reset-head needs --init-from")
    if not 0.0 < args.layer_decay <= 1.0:
        parser.error("--layer-decay must be in (0, 1]")
    if args.layer_decay < 1.0:
        if args.optimizer != "adamw":
            parser.error("--layer-decay needs --optimizer adamw")
        if not args.arch.startswith(("vit", "convnext")):
            parser.error(f"--layer-decay is for ViT (vit_*) and ConvNeXt (convnext_*) archs, not --arch {args.arch}")
        if args.parallel == "pipe":
            parser.error("--layer-decay with --parallel pipe is not supported "
                         "(per-stage optimizers see partial models)")
    if not 0.0 <= args.reprob <= 1.0:
        parser.error("--reprob must be in [0, 1]")
    if args.remode is not None and not args.reprob:
        parser.error("--remode needs --reprob")
    if args.remode is None:
        args.remode = "pixel"
    if args.reprob and args.parallel == "pipe":
        parser.error("--reprob with --parallel pipe is not supported "
                     "(the pipeline path feeds its stages itself and has no batch-level augmentation)")
    if args.augment_staging is not None and not args.gpu_augment:
        parser.error("--augment-staging needs --gpu-augment")
    if args.rand_augment is not None:
        if not args.gpu_augment:
            parser.error("--rand-augment needs --gpu-augment")
        from ..data.rand_augment import parse_rand_augment
        try:
            parse_rand_augment(args.rand_augment)
        except ValueError as e:
            parser.error(str(e))
    if args.gpu_augment:
        if args.parallel == "pipe":
            parser.error("--gpu-augment with --parallel pipe is not supported "
                         "(the pipeline's first-stage feed takes finished images)")
        if args.augment_staging is not None and not 1 <= args.augment_staging <= 16384:
            parser.error("--augment-staging must be in [1, 16384]")
    world = args.world_size or int(os.environ.get("WORLD_SIZE", "1"))
    if args.clip_grad_norm and args.parallel == "pipe" and world > 1:
        parser.error("--clip-grad-norm with --parallel pipe at world size > 1 is not supported "
                     "(a pipeline's global norm needs a cross-stage reduction)")


def _optimizer(args, target, flat: bool, lr_scales=None):
    from ..ops.optim import build_optimizer
    trust = TRUST_COEFFICIENT if args.trust_coefficient is None else args.trust_coefficient
    return build_optimizer(args.optimizer, target, flat, lr=args.lr, momentum=args.momentum,
                           weight_decay=args.weight_decay, betas=args.betas, eps=args.eps,
                           clip_grad_norm=args.clip_grad_norm, trust_coefficient=trust,
                           ema_decay=getattr(args, "model_ema_decay", 0.0) or None,
                           ema_warmup=getattr(args, "model_ema_warmup", False), lr_scales=lr_scales)


def _optimizer_log(args, opt) -> dict:
    """What the epoch log line says about the optimizer's last step (one device read per epoch)."""
    extra = {}
    if args.clip_grad_norm and opt.last_grad_norm is not None:
        extra["grad_norm"] = float(opt.last_grad_norm)
    if args.optimizer == "lars":
        span = opt.last_trust_range()  # over the adapted tensors
        if span is not None:
            extra["trust_min"], extra["trust_max"] = span
    return extra


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="MI355X-native data / model parallel training")
    p.add_argument("data", nargs="?", default="", metavar="DIR", help="dataset root (empty: synthetic)")
    p.add_argument("--dist-url", default=None, help="init method (default env:// from torchrun)")
    p.add_argument("--world-size", default=None, type=int,
                   help="processes to spawn for --parallel pipe without torchrun")
    p.add_argument("--dist-backend", default=None, help="nccl (=RCCL) on GPU, gloo on CPU")
    p.add_argument("--lr", "--learning-rate", default=0.4, type=float, dest="lr")
    p.add_argument("--epochs", default=90, type=int)
    p.add_argument("-type", "--dataset-type", default="CIFAR10", dest="dataset_type")
    p.add_argument("-b", "--batch-size", default=512, type=int,
                   help="per-process batch for ddp; total batch for dp and pipe")
    p.add_argument("-j", "--workers", default=4, type=int)
    p.add_argument("--wd", "--weight-decay", default=1e-4, type=float, dest="weight_decay")
    p.add_argument("--momentum", default=0.9, type=float)
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "adamw", "lars"],
                   help="adamw: decoupled weight decay (off for biases / norm weights), e.g. --lr 1e-3 --wd 0.05; "
                        "lars: momentum SGD with per-tensor trust ratios (biases / norm weights excluded), "
                        "for large batches")
    p.add_argument("--betas", default=(0.9, 0.999), type=_betas, metavar="B1,B2", help="--optimizer adamw")
    p.add_argument("--eps", default=1e-8, type=float, help="--optimizer adamw / lars")
    p.add_argument("--trust-coefficient", default=None, type=float, metavar="ETA",
                   help=f"--optimizer lars: trust ratio = ETA |w| / (|g| + wd |w| + eps) (default {TRUST_COEFFICIENT})")
    p.add_argument("--clip-grad-norm", default=0.0, type=float, metavar="X",
                   help="--optimizer adamw: clip the global gradient norm to X (0 = off)")
    p.add_argument("--label-smoothing", default=0.0, type=float, metavar="E",
                   help="training loss: weight E spread uniformly over the classes, in [0, 1) "
                        "(validation loss stays plain)")
    p.add_argument("--mixup-alpha", default=0.0, type=float, metavar="A",
                   help="mixup with lam ~ Beta(A, A) on the training batches (0 = off; not with --parallel pipe); "
                        "acc1_train stays top-1 against each sample's own (first) label")
    p.add_argument("--cutmix-alpha", default=0.0, type=float, metavar="A",
                   help="CutMix with lam ~ Beta(A, A) (0 = off); with --mixup-alpha each mixed batch picks one "
                        "of the two with equal odds; acc1_train as for --mixup-alpha")
    p.add_argument("--mix-prob", default=None, type=float, metavar="P",
                   help="probability that a training batch is mixed (default 1.0; needs an alpha)")
    p.add_argument("--drop-path", default=0.0, type=float, metavar="R",
                   help="ViT and ConvNeXt archs only: stochastic depth, block i of L drops its residual branches per sample "
                        "with probability R * i / (L - 1), in [0, 1) (0 = off; e.g. 0.1 for ViT-B from scratch, "
                        "0.5 for ConvNeXt-B)")
    p.add_argument("--model-ema-decay", default=0.0, type=float, metavar="D",
                   help="keep an exponential moving average of the fp32 master weights inside the optimizer's "
                        "step kernels, decay D in [0, 1) (0 = off; e.g. 0.9999); every epoch also evaluates it "
                        "(loss_val_ema / acc1_val_ema) and checkpoints carry it as net_ema.  BatchNorm running "
                        "statistics are not averaged: the EMA evaluation uses the live buffers.  Checkpoint "
                        "selection stays on the live accuracy; not with --parallel pipe")
    p.add_argument("--model-ema-warmup", action="store_true",
                   help="--model-ema-decay: update k uses min(D, (1 + k) / (10 + k)), so the average follows "
                        "the weights early on")
    p.add_argument("-r", "--resume", action="store_true")
    p.add_argument("--init-from", default="", metavar="CKPT",
                   help="initialise the model from CKPT's weights only (fine-tuning: no optimizer / scheduler / "
                        "RNG state; a ViT position embedding of another resolution is resized bicubically); "
                        "not together with --resume from an existing checkpoint")
    p.add_argument("--init-from-ema", action="store_true",
                   help="--init-from: take CKPT's averaged weights (net_ema, written by a --model-ema-decay run)")
    p.add_argument("--reset-head", action="store_true",
                   help="--init-from: a classifier whose shape differs from the model's (another class count) is "
                        "left at its fresh initialisation instead of being an error")
    p.add_argument("--layer-decay", default=1.0, type=float, metavar="D",
                   help="--optimizer adamw, ViT and ConvNeXt archs: layer-wise lr decay for fine-tuning, the head "
                        "trains at --lr and a layer k below it at lr * D^k, in (0, 1] (1 = off; e.g. 0.75 for "
                        "ViT-B, 0.65 for smaller ones); not with --parallel pipe")
    p.add_argument("--image-size", default=None, type=int, metavar="N",
                   help="ViT archs only: train at N x N pixels (model, ImageNet transforms and synthetic data)")
    p.add_argument("--arch", default="mobilenetv2")
    p.add_argument("--parallel", default="ddp", choices=["ddp", "dp", "pipe", "none"])
    p.add_argument("--bucket-cap-mb", default=25.0, type=float)
    p.add_argument("--dp-graphs", action="store_true",
                   help="--parallel dp: replicas' forward/backward as captured hipGraphs (no replica threads)")
    p.add_argument("--sync-bn", action="store_true")
    p.add_argument("--dtype", default="auto", choices=["auto", "fp32", "bf16"],
                   help="auto: bf16 (fp32 master weights) on GPU -- the native MFMA path -- fp32 on CPU")
    p.add_argument("--channels-last", dest="channels_last", action="store_true", default=None,
                   help="NHWC activations (default on GPU: every native conv/BN kernel is NHWC)")
    p.add_argument("--no-channels-last", dest="channels_last", action="store_false")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--gpu-augment", action="store_true",
                   help="loader workers only decode to uint8; the batch goes up as bytes and one kernel crops "
                        "(CIFAR-type sets: pad 4 + random crop; otherwise random resized crop), flips, normalises, "
                        "casts and lays out (data/gpu_augment.py); validation takes the same kernel with the "
                        "identity plan; not with --parallel pipe")
    p.add_argument("--augment-staging", default=None, type=int, metavar="S",
                   help="--gpu-augment, ImageNet-style sets: workers resize the shorter side to S and keep the "
                        "central S x S square, from which the random resized crops are drawn "
                        "(default round(size * 8 / 7): 256 for 224, 439 for 384)")
    p.add_argument("--rand-augment", default=None, metavar="SPEC",
                   help="--gpu-augment, training batches: RandAugment after the crop / flip, e.g. rand-m9-mstd0.5-inc1 "
                        "(keys m, n, mstd, p; inc1 required: the 15 'increasing' ops; data/rand_augment.py); the "
                        "affine ops fill with the dataset's mean colour")
    p.add_argument("--reprob", default=0.0, type=float, metavar="P",
                   help="random erasing of training batches on the device, after the augmentation and before "
                        "mixup / CutMix: each sample with probability P gets one box of 2 %% to 1/3 of its area "
                        "overwritten (data/random_erase.py; 0 = off; with or without --gpu-augment; not with "
                        "--parallel pipe)")
    p.add_argument("--remode", default=None, choices=["pixel", "rand", "const"],
                   help="--reprob: what the box is filled with: N(0, 1) noise per element (pixel, the default), "
                        "one N(0, 1) value per sample and channel (rand) or zeros (const)")
    p.add_argument("--micro-batches", default=1, type=int)
    p.add_argument("--no-pipe-graphs", action="store_true",
                   help="--parallel pipe on GPU: eager micro-batches instead of captured stage graphs")
    p.add_argument("--schedule", default="1f1b", choices=["naive", "gpipe", "1f1b"])
    p.add_argument("--partition", default="balanced", choices=["balanced", "reference"],
                   help="pipeline stage cut: FLOP-balanced (any ws) or the reference's MobileNetV2 cut")
    p.add_argument("--warmup-epochs", default=10, type=int, help="linear lr warm-up (0 = none)")
    p.add_argument("--lr-steps", default="", metavar="E1,E2,...",
                   help="step decay at these epochs instead of cosine (reference no-BN study: 30,60)")
    p.add_argument("--lr-gamma", default=0.1, type=float, help="decay factor of --lr-steps")
    p.add_argument("--checkpoint-segments", default=0, type=int, metavar="K",
                   help="activation checkpointing: recompute the model in K segments in backward "
                        "(reference large-batch runs '2048(checkpoint)', Readme.md:168,192; 0 = off)")
    p.add_argument("--steps-per-epoch", default=0, type=int, help="cap iterations per epoch (0 = all)")
    p.add_argument("--log-dir", default="./log")
    p.add_argument("--checkpoint", default="./checkpoint/ckpt.pth")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--watchdog", default=None, type=float, metavar="SECONDS",
                   help="abort (exit 1, so torchrun can restart) when the collective stream makes "
                        "no progress for SECONDS (default 1800 when distributed on GPU, 0 = off)")
    return p


def _augment_geometry(args):
    """(CIFAR-type?, output side, training source side) of the --gpu-augment path: CIFAR-type sets
    crop their own 32 x 32 images with padding, the others resize crops of the staging square."""
    synthetic = args.synthetic or not args.data
    cifar = (_synthetic_kind(args) == "SyntheticCIFAR") if synthetic else args.dataset_type == "CIFAR10"
    size = args.image_size if args.image_size is not None else (32 if cifar else 224)
    if cifar:
        return True, size, size if synthetic else 32  # the CIFAR-10 files hold 32 x 32 images
    return False, size, args.augment_staging if args.augment_staging is not None else round(size * 8 / 7)


def _datasets(args):
    from ..data import DatasetCollection, transforms as T
    cifar = args.dataset_type in ("CIFAR10", "SyntheticCIFAR")
    if getattr(args, "gpu_augment", False):  # uint8 HWC: decoded (and staged) only
        from ..data import SyntheticImages
        is_cifar, size, source = _augment_geometry(args)
        if args.synthetic or not args.data:
            nc = _num_classes(args)
            n_train, n_val = (5000, 1000) if is_cifar else (1281, 500)
            return (SyntheticImages(n_train, (3, source, source), nc, uint8=True),
                    SyntheticImages(n_val, (3, size, size), nc, seed=1, uint8=True))
        if is_cifar:
            tr = va = T.cifar_staging_transform()
        else:
            tr, va = T.imagenet_train_staging_transform(source), T.imagenet_val_staging_transform(size)
        return DatasetCollection(args.dataset_type, args.data, tr, va).init()
    if args.synthetic or not args.data:
        if args.image_size is not None:  # the stock synthetic sets, at the ViT's own resolution
            from ..data import SyntheticImages
            shape, nc = (3, args.image_size, args.image_size), _num_classes(args)
            n_train, n_val = (5000, 1000) if _synthetic_kind(args) == "SyntheticCIFAR" else (1281, 500)
            return SyntheticImages(n_train, shape, nc), SyntheticImages(n_val, shape, nc, seed=1)
        return DatasetCollection(_synthetic_kind(args), "").init()
    if cifar:
        tr, va = T.cifar_train_transform(), T.cifar_test_transform()
    elif args.image_size is not None:
        tr, va = T.imagenet_train_transform(args.image_size), T.imagenet_val_transform(args.image_size)
    else:
        tr, va = T.imagenet_train_transform(), T.imagenet_val_transform()
    return DatasetCollection(args.dataset_type, args.data, tr, va).init()


def _synthetic_kind(args) -> str:
    """Synthetic data of the dataset type's shape -- except for a ViT, whose position
    embedding fixes the input size: it gets data of the model's own shape and class count
    (and so does a ConvNeXt: convnext_test is a 32-pixel model)."""
    if args.arch.startswith(("vit", "convnext")):
        from ..models import INPUT_SHAPES
        return "SyntheticCIFAR" if INPUT_SHAPES[args.arch][0][1] == 32 else "Synthetic"
    cifar = args.dataset_type in ("CIFAR10", "SyntheticCIFAR")
    return "SyntheticCIFAR" if cifar or args.arch.startswith("mobilenet") else "Synthetic"


def _lr_steps(args):
    return [int(v) for v in args.lr_steps.split(",") if v.strip()] if args.lr_steps else None


def _num_classes(args) -> int:
    if (args.synthetic or not args.data) and args.arch.startswith(("vit", "convnext")):
        return 10 if _synthetic_kind(args) == "SyntheticCIFAR" else 1000
    return {"CIFAR10": 10, "SyntheticCIFAR": 10, "CUB200": 200, "Place365": 365}.get(
        args.dataset_type, 10 if (args.synthetic or not args.data) and args.arch.startswith("mobilenet") else 1000)


# --------------------------------------------------------------------------- #
def run_data_parallel(args, env) -> None:
    from ..data import prepare_dataloaders
    from ..models import build_model
    from ..parallel.data_parallel import DataParallel
    from ..parallel.distributed import DistributedDataParallel
    from ..parallel.sync_batchnorm import SyncBatchNorm
    from ..utils.checkpoint import load_checkpoint, save_checkpoint
    from ..utils.logging import MetricsLogger
    from ..utils.metrics import AverageMeter, accuracy
    from ..utils.precision import cast_model, parse_dtype
    from ..ops.loss import cross_entropy
    from ..utils.profiling import trace_range
    from ..utils.schedule import build_schedule
    from ..utils.timers import StepTimer

    dev = env.device
    dtype = parse_dtype(args.dtype)
    size_kw = {} if args.image_size is None else {"image_size": args.image_size}
    if args.drop_path > 0:
        size_kw["drop_path_rate"] = args.drop_path
    model = build_model(args.arch, num_classes=_num_classes(args), **size_kw)
    if args.init_from:
        from ..utils.checkpoint import load_weights
        # before the cast and the optimizer: masters start from these
        load_weights(args.init_from, model, ema=args.init_from_ema, reset_head=args.reset_head)
    if args.checkpoint_segments > 1:
        from ..utils.checkpointing import enable_activation_checkpointing
        enable_activation_checkpointing(model, args.checkpoint_segments)
    if args.sync_bn and args.parallel == "ddp":
        model = SyncBatchNorm.convert_sync_batchnorm(model)
    model = model.to(dev)
    if args.channels_last:
        model = model.to(memory_format=torch.channels_last)
    if dtype != torch.float32:
        cast_model(model, dtype)
    scales = None
    if args.layer_decay < 1.0:  # on the bare model: its Parameter objects survive DDP's re-homing onto the flats
        from ..models.layer_decay import layer_decay_scales
        scales = layer_decay_scales(model, args.layer_decay)
    if args.parallel == "ddp":
        net = DistributedDataParallel(model, bucket_cap_mb=args.bucket_cap_mb, flat_parameters=True)
        opt = _optimizer(args, net, flat=True, lr_scales=scales)
    else:
        # fp32 master weights for bf16 models: same update as DDP's flat optimizer
        opt = _optimizer(args, model.parameters(), flat=False, lr_scales=scales)
        net = DataParallel(model, graphs=args.dp_graphs) if args.parallel == "dp" else model
    sched = build_schedule(opt, args.epochs, args.warmup_epochs, _lr_steps(args), args.lr_gamma)
    from ..utils.debug import rank0_first
    with rank0_first():  # defect 6: rank 0 prepares / indexes the dataset before the others read it
        train_ds, val_ds = _datasets(args)
    sampler, train_loader, val_loader = prepare_dataloaders(
        train_ds, val_ds, args.batch_size, args.workers, distributed=args.parallel == "ddp" and env.distributed,
        pin_memory=dev.type == "cuda", seed=args.seed)
    start_epoch, best = 0, 0.0
    if args.resume and os.path.exists(args.checkpoint):
        meta = load_checkpoint(args.checkpoint, net, opt, sched, map_location=dev)
        start_epoch, best = meta["epoch"] + 1, meta["acc"]
    logger = MetricsLogger(args.log_dir, f"{args.parallel}_{args.arch}", env.rank,
                           text_file=f"{args.parallel}_{args.batch_size}.txt")
    if scales is not None:  # once, at start-up (host-side values: no device read)
        lo, hi = opt.lr_scale_range()
        logger.event("layer_decay", decay=args.layer_decay, distinct_scales=len(set(scales.values())),
                     lr_scale_min=lo, lr_scale_max=hi)
        if env.is_main:
            print(f"layer_decay:{args.layer_decay}  distinct_scales:{len(set(scales.values()))}  "
                  f"lr_scale_min:{lo}  lr_scale_max:{hi}", flush=True)

    def to_dev(x, y):
        x = x.to(dev, dtype, non_blocking=True)
        if args.channels_last and x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        return x, y.to(dev, non_blocking=True)

    to_dev_val = to_dev  # without --gpu-augment validation batches go up as training batches do
    planner = rand_planner = None
    if args.gpu_augment:  # the batch goes up as bytes; crop / flip / normalise / cast / layout in one kernel
        from ..data import AugmentPlanner, gpu_augment, transforms as T
        is_cifar, size, source = _augment_geometry(args)
        mean, std = (T.CIFAR_MEAN, T.CIFAR_STD) if is_cifar else (T.IMAGENET_MEAN, T.IMAGENET_STD)
        planner = AugmentPlanner("pad_crop" if is_cifar else "rrc", size, source, seed=args.seed,
                                 rank=env.rank if args.parallel == "ddp" else 0)
        eval_planner = AugmentPlanner("identity", size, size)
        if args.rand_augment is not None:  # training batches only
            from ..data.rand_augment import RandAugmentPlanner, fill_from_mean, parse_rand_augment
            rand_planner = RandAugmentPlanner(**parse_rand_augment(args.rand_augment), fill=fill_from_mean(mean),
                                              seed=args.seed, rank=env.rank if args.parallel == "ddp" else 0)

        def augment_to_dev(plans, rand=None):
            def feed(x, y):
                ops = rand.plan(x.shape[0], size, size) if rand is not None else None
                x = gpu_augment(x.to(dev, non_blocking=True), plans.plan(x.shape[0]), size, mean, std, dtype=dtype,
                                channels_last=bool(args.channels_last), ops=ops,
                                fill=rand.fill if rand is not None else None)
                return x, y.to(dev, non_blocking=True)
            return feed

        to_dev, to_dev_val = augment_to_dev(planner, rand_planner), augment_to_dev(eval_planner)

    eraser = None
    if args.reprob > 0:  # training batches only, in place on the normalised batch
        from ..data import RandomErasePlanner, random_erase_
        eraser = RandomErasePlanner(args.reprob, args.remode, seed=args.seed,
                                    rank=env.rank if args.parallel == "ddp" else 0)
    mixer = None
    if args.mixup_alpha > 0 or args.cutmix_alpha > 0:
        from ..ops.mix import BatchMixer
        mixer = BatchMixer(args.mixup_alpha, args.cutmix_alpha, prob=args.mix_prob, seed=args.seed,
                           rank=env.rank if args.parallel == "ddp" else 0)
    timer = StepTimer(dev)
    for epoch in range(start_epoch, args.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        if planner is not None:
            planner.set_epoch(epoch)
        if rand_planner is not None:
            rand_planner.set_epoch(epoch)
        if eraser is not None:
            eraser.set_epoch(epoch)
        if mixer is not None:
            mixer.set_epoch(epoch)
        net.train()
        lm, am = AverageMeter(), AverageMeter()
        it = iter(train_loader)
        i = 0
        while not (args.steps_per_epoch and i >= args.steps_per_epoch):
            with timer.region("data"):  # reference data_time (utils.py:48): host wait + H2D
                batch = next(it, None)
                if batch is None:
                    break
                x, y = to_dev(*batch)
                if eraser is not None:
                    x = random_erase_(x, *eraser.plan(x.shape[0], x.shape[2], x.shape[3]), noise=eraser.noise)
            with timer.region("step"), trace_range("train.step"):
                y_b, lam = None, 1.0
                if mixer is not None:
                    x, y, y_b, lam = mixer(x, y)
                out = net(x)
                loss = cross_entropy(out, y, label_smoothing=args.label_smoothing, target_b=y_b, lam=lam)
                loss.backward()
                opt.step()
                opt.zero_grad()
            lm.update(loss.detach(), y.shape[0])
            am.update(accuracy(out, y)[0], y.shape[0])
            i += 1
        if dev.type == "cuda":
            torch.cuda.synchronize()
        tm = timer.summary()  # device time of the step (HIP events), host time of the data wait
        step_s, data_s = tm.get("step", 0.0) / 1e3, tm.get("data_host", 0.0) / 1e3
        vl, va = evaluate(net, val_loader, to_dev_val, args)
        ema_log, ck_extra = {}, None
        if args.model_ema_decay:  # the averaged weights on the live buffers (BN statistics are not averaged)
            with opt.ema_weights():
                vle, vae = evaluate(net, val_loader, to_dev_val, args)
            ema_log = {"loss_val_ema": vle, "acc1_val_ema": vae, "ema_decay": args.model_ema_decay}
            ck_extra = {"acc_ema": float(vae)}
        sched.step()
        if env.is_main and va > best:  # selection stays on the live accuracy
            best = va
            save_checkpoint(args.checkpoint, net, opt, sched, epoch, best, extra=ck_extra)
        extra = _optimizer_log(args, opt)  # the epoch's last step; one read per epoch
        extra.update(ema_log)
        if args.drop_path > 0:
            extra["drop_path"] = args.drop_path  # the run's setting, in every epoch's JSONL record
        logger.log(epoch, loss_train=lm.avg, acc1_train=am.avg, loss_val=vl, acc1_val=va,
                   time_per_batch=step_s + data_s, time_load_perbatch=data_s,
                   images_per_sec=(args.batch_size * max(1, env.world_size if args.parallel == "ddp" else 1))
                   / max(step_s + data_s, 1e-9), lr=opt.param_groups[0]["lr"], **extra)


@torch.no_grad()
def evaluate(net, loader, to_dev, args):
    from ..utils.metrics import AverageMeter, accuracy
    net.eval()
    lm, am = AverageMeter(), AverageMeter()
    for i, (x, y) in enumerate(loader):
        if args.steps_per_epoch and i >= args.steps_per_epoch:
            break
        x, y = to_dev(x, y)
        out = net(x)
        lm.update(F.cross_entropy(out.float(), y), y.shape[0])
        am.update(accuracy(out, y)[0], y.shape[0])
    return lm.avg, am.avg


# --------------------------------------------------------------------------- #
def batch_schedule(loader, batch_size: int):
    """(number of batches, size of the last) of `loader`, read from its batch
    sampler without loading data; ValueError unless every batch but the last
    has `batch_size` samples (the pipeline's static shape contract)."""
    bsamp = getattr(loader, "batch_sampler", None)
    sampler = getattr(bsamp, "sampler", None)
    if bsamp is not None and type(bsamp) is torch.utils.data.BatchSampler and sampler is not None:
        n_items, bs, drop = len(sampler), bsamp.batch_size, bsamp.drop_last
        if bs != batch_size:
            raise ValueError(f"loader batch size {bs} != contract {batch_size}")
        n = n_items // bs if drop else -(-n_items // bs)
        last = bs if (drop or n_items % bs == 0) else n_items % bs
    else:  # a custom batch sampler: walk its index lists (no data is loaded)
        sizes = [len(b) for b in (bsamp if bsamp is not None else [])]
        if not sizes:
            raise ValueError("loader has no inspectable batch sampler")
        if any(s != batch_size for s in sizes[:-1]) or sizes[-1] > batch_size:
            raise ValueError(f"batch sizes {sorted(set(sizes))} do not follow the contract {batch_size}")
        n, last = len(sizes), sizes[-1]
    if n != len(loader):
        raise ValueError(f"batch sampler yields {n} batches, len(loader) = {len(loader)}")
    return n, last


def run_pipeline(args, env) -> None:
    from ..comm.rccl import Communicator
    from ..data import prepare_dataloaders
    from ..models import INPUT_SHAPES, build_model
    from ..parallel.pipeline import Pipeline
    from ..utils.checkpoint import save_checkpoint, stage_checkpoint_path
    from ..utils.logging import MetricsLogger
    from ..utils.precision import parse_dtype
    from ..utils.profiling import trace_range
    from ..utils.schedule import build_schedule
    from ..utils.timers import StepTimer

    torch.manual_seed(args.seed)  # every rank builds the same full model (reference: unseeded)
    model = build_model(args.arch, num_classes=_num_classes(args))
    (c, h, w), _ = INPUT_SHAPES.get(args.arch, ((3, 32, 32), 10))
    comm = Communicator(env.device)
    pipe = Pipeline(model.as_sequential(), comm, (c, h, w), micro_batches=args.micro_batches,
                    schedule=args.schedule, dtype=parse_dtype(args.dtype),
                    channels_last=args.channels_last, partition=args.partition,
                    label_smoothing=args.label_smoothing,
                    # one GPU only (see train/step.py): multi-rank GPU pipelines run eagerly
                    graphs=env.device.type == "cuda" and not args.no_pipe_graphs and comm.size == 1)
    opt = _optimizer(args, pipe.module.parameters(), flat=False)
    sched = build_schedule(opt, args.epochs, args.warmup_epochs, _lr_steps(args), args.lr_gamma)
    logger = MetricsLogger(args.log_dir, f"pipe_{args.arch}", env.rank, text_file=f"{args.batch_size}.txt")
    if env.rank == 0:
        train_ds, val_ds = _datasets(args)
        _, train_loader, val_loader = prepare_dataloaders(train_ds, val_ds, args.batch_size, args.workers,
                                                          pin_memory=env.device.type == "cuda")
        vbs = val_loader.batch_size or args.batch_size
        # the static batch contract of every step, checked against the loaders'
        # batch samplers BEFORE the loop: a mismatch found later would raise on
        # rank 0 only while the other stages wait in a receive
        bad = ""
        try:
            n_train, last_t = batch_schedule(train_loader, args.batch_size)
            n_val, last_v = batch_schedule(val_loader, vbs)
        except ValueError as e:
            bad, n_train = str(e), -1
            n_val = last_t = last_v = 0
    else:
        train_loader = val_loader = None
        n_train = n_val = last_t = last_v = vbs = 0
    # only rank 0 loads data; the others learn the iteration counts and batch
    # sizes once (defect 6), so no step needs a batch-size message or host sync
    counts = torch.tensor([n_train, n_val, last_t, last_v, vbs], dtype=torch.int64, device=env.device)
    comm.broadcast(counts, 0)
    comm.synchronize()
    n_train, n_val, last_t, last_v, vbs = (int(v) for v in counts.tolist())
    if n_train < 0:  # every rank stops here, together
        raise ValueError("pipeline: the data loader's batches do not follow the static batch contract"
                         + (f" ({bad})" if env.rank == 0 else " (see rank 0)"))
    n_train_all, n_val_all = n_train, n_val
    if args.steps_per_epoch:
        n_train, n_val = min(n_train, args.steps_per_epoch), min(n_val, args.steps_per_epoch)
    timer = StepTimer(env.device)
    for epoch in range(args.epochs):
        it = iter(train_loader) if train_loader is not None else None
        sums = []  # per-step device stats, read once per epoch
        for i in range(n_train):
            with timer.region("data"):
                x, y = next(it) if it is not None else (None, None)
            bs = last_t if i == n_train_all - 1 else args.batch_size
            with timer.region("step"), trace_range("pipe.train_step"):
                r = pipe.train_step(x, y, batch_size=bs)
                opt.step()
                opt.zero_grad()
            if r.valid:
                sums.append(r)
        loss_s = sum(r.loss for r in sums)
        acc_s = sum(r.top1 for r in sums)
        tm = timer.summary()
        tot_t = (tm.get("step", 0.0) + tm.get("data_host", 0.0)) / 1e3 * max(n_train, 1)
        tot_d = tm.get("data_host", 0.0) / 1e3 * max(n_train, 1)
        vit = iter(val_loader) if val_loader is not None else None
        vl, va = 0.0, 0.0
        for i in range(n_val):
            x, y = next(vit) if vit is not None else (None, None)
            r = pipe.eval_step(x, y, batch_size=last_v if i == n_val_all - 1 else vbs)
            if r.valid:
                vl += r.loss
                va += r.top1
        sched.step()
        save_checkpoint(stage_checkpoint_path(args.checkpoint, env.rank), pipe.module, opt, sched, epoch,
                        all_ranks=True)
        if env.rank == 0:
            extra = _optimizer_log(args, opt)
            logger.log(epoch, loss_train=loss_s / max(n_train, 1), acc1_train=acc_s / max(n_train, 1),
                       loss_val=vl / max(n_val, 1), acc1_val=va / max(n_val, 1),
                       time_per_batch=tot_t / max(n_train, 1), time_load_perbatch=tot_d / max(n_train, 1),
                       **extra)


def _spawn_entry(rank: int, world: int, args) -> None:
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    main_worker(args)


def main_worker(args) -> None:
    from ..utils.env import destroy_distributed, init_distributed, seed_everything
    from ..utils import miopen_db
    env = init_distributed(backend=args.dist_backend, dist_url=args.dist_url)
    gpu = env.device.type == "cuda"
    if args.dtype == "auto":
        args.dtype = "bf16" if gpu else "fp32"
    if args.channels_last is None:
        args.channels_last = gpu
    if env.device.type == "cuda":
        miopen_db.seed("use")  # committed MIOpen find db (skips the first-step solver search)
    seed_everything(args.seed + (env.rank if args.parallel == "ddp" else 0))
    dog = start_watchdog(args.watchdog, env)
    try:
        if args.parallel == "pipe":
            run_pipeline(args, env)
        else:
            run_data_parallel(args, env)
    finally:
        if dog is not None:
            dog.stop()
        destroy_distributed()


def start_watchdog(seconds: Optional[float], env):
    """Start a CommWatchdog on the process's communicator: a
    collective stream stuck for `seconds` ends the process with exit code 1
    (no re-exec), so torchrun --max-restarts can restart the job."""
    if seconds is None:
        seconds = 1800.0 if (env.distributed and env.device.type == "cuda") else 0.0
    if seconds <= 0 or env.device.type != "cuda":
        return None
    from ..comm.rccl import default_communicator
    from ..utils.debug import CommWatchdog
    return CommWatchdog(default_communicator(env.device), timeout_s=seconds,
                        interval_s=min(5.0, seconds / 4)).start()


def main(argv: Optional[list] = None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    check_args(parser, args)
    if args.parallel == "pipe" and args.world_size and "RANK" not in os.environ:
        import torch.multiprocessing as mp
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        mp.spawn(_spawn_entry, args=(args.world_size, args), nprocs=args.world_size, join=True)
        return 0
    main_worker(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
