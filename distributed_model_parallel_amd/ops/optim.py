"""Flat optimizers: torch.optim.SGD / torch.optim.AdamW semantics and LARS, a
constant number of HIP launches per dtype group.

``FlatSGD`` / ``FlatAdamW`` / ``FlatLARS`` work on the flat parameter /
gradient buffers of ``DistributedDataParallel(..., flat_parameters=True)``:
gradients there are already RCCL-averaged bucket views, parameters are views
of a flat buffer with the same layout, so the update of all 161 ResNet-50
tensors is a single vectorised pass (``csrc/optim/fused_sgd.hip``,
``csrc/optim/fused_adamw.hip``, ``csrc/optim/fused_lars.hip``, on the shared
host path and device helpers of ``csrc/optim/flat_step.h``).
``MasterSGD`` / ``MasterAdamW`` / ``MasterLARS`` build the same kind of flat
buffers for any parameter list.  bf16 parameter groups keep an fp32 master copy
and fp32 optimizer state inside the optimizer; the kernel writes the bf16
working weights back in the same pass.

The six classes are a layout (``_DDPLayout`` / ``_ListLayout``: where the
flats come from, how state follows a bucket rebuild, checkpoint format) times
an update rule (``_SGDRule`` / ``_AdamWRule`` / ``_LARSRule``), on the shared
``_FlatOptimizer`` step.

Reference parity: SGD(lr, momentum 0.9, weight_decay 1e-4) at
``model_parallel.py:105`` / ``data_parallel.py:90``.  AdamW
with decoupled decay off for biases / norm weights and global-norm clipping is
what every ViT recipe trains with; LARS (per-tensor trust ratios from a
segmented norm over the flats) is what large-batch ResNet recipes train with.

Every class can keep an exponential moving average of the weights
(``ema_decay``): an fp32 flat per group, averaged over the fp32 MASTERS (a bf16
average at decay 0.9999 never moves: the increment is far below one bf16 ulp)
and updated inside the step kernel, which holds every new master value in
registers when it stores it (+8 B per element, no launch).
``DMP_DISABLE=fuse_ema`` (or ``set_fused_ema(False)``) runs the step kernel
without it and a ``lerp_`` pass after it.
"""
from __future__ import annotations

import contextlib
import math
import warnings
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from .. import _native
from . import wgrad_stream, wt_cache

_FUSED_EMA = not _native.disabled("fuse_ema")


def set_fused_ema(on: bool) -> None:
    """Weight EMA inside the step kernels (True) or as a ``lerp_`` pass after them."""
    global _FUSED_EMA
    _FUSED_EMA = bool(on)


def fused_ema() -> bool:
    return _FUSED_EMA


class ForeignOptimizerState(ValueError):
    """The state dict was written by another optimizer class (e.g. a
    torch.optim.SGD state from an older DataParallel run, or an AdamW state
    offered to an SGD class): nothing in it maps onto this optimizer.
    ``load_checkpoint`` tolerates only this case; a layout mismatch of our own
    format stays a hard error."""


# --------------------------------------------------------------------------- #
# shared step
# --------------------------------------------------------------------------- #
class _FlatOptimizer(torch.optim.Optimizer):
    """What every flat optimizer does around its update rule.

    A *group* is a dict with the flat ``param`` and ``grad`` of one
    dtype/device group, an fp32 ``master`` when the parameters are not fp32,
    and one fp32 flat per name in ``STATE_KEYS``.  The layout mixin supplies
    ``_current_groups`` / ``_slots`` / ``_layout_id``; the rule mixin supplies
    ``KIND`` / ``STATE_KEYS`` / ``_update``.
    """

    KIND = ""
    STATE_KEYS: Tuple[str, ...] = ()

    def _name(self) -> str:
        return type(self).__name__

    def _init_ema(self, ema_decay: Optional[float], ema_warmup: bool) -> None:
        d = float(ema_decay or 0.0)
        if not 0.0 <= d < 1.0:
            raise ValueError("%s: ema_decay must be in [0, 1), got %r" % (self._name(), ema_decay))
        self.ema_decay = d
        self.ema_warmup = bool(ema_warmup)
        self._ema_updates = 0      # host counter: the warm-up's k
        self._ema_now = 0.0        # decay of the update in flight (a host scalar, like lr)
        self._ema_swapped = False  # inside ema_weights()

    @property
    def ema_enabled(self) -> bool:
        return self.ema_decay > 0.0

    def _alloc_state(self, st: dict) -> None:
        pflat = st["param"]
        if pflat.dtype != torch.float32 and self.master_weights:
            st["master"] = pflat.float()
        for k in self.STATE_KEYS:
            st[k] = torch.zeros(pflat.numel(), dtype=torch.float32, device=pflat.device)
        if self.ema_enabled:  # starts at the weights the optimizer was built on; slot padding stays 0
            st["ema"] = st.get("master", pflat).detach().to(torch.float32, copy=True)

    def ema_decay_of_update(self, k: int) -> float:
        """Decay of EMA update number ``k`` (0-based): ``ema_decay``, or with
        ``ema_warmup`` ``min(ema_decay, (1 + k) / (10 + k))``."""
        if self.ema_warmup:
            return min(self.ema_decay, (1.0 + k) / (10.0 + k))
        return self.ema_decay

    def _aligned_slots(self, gi: int):
        """``_slots(gi)``, every offset checked to be a multiple of the kernels' 8-element vector."""
        for p, off in self._slots(gi):
            if off % 8:
                raise RuntimeError("%s: parameter slot at offset %d is not 8-element aligned"
                                   % (self._name(), off))
            yield p, off

    def _ema_args(self, st: dict):
        """(ema, ema_decay) for the group's step kernel: (None, 0.0) where the
        EMA is off or follows the kernel as a pass of its own."""
        if self.ema_enabled and _FUSED_EMA and st["param"].is_cuda:
            return st["ema"], self._ema_now
        return None, 0.0

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.ema_enabled:
            if self._ema_swapped:
                raise RuntimeError("%s.step() inside ema_weights(): the working weights are the EMA's"
                                   % self._name())
            if self.ema_warmup and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise ValueError("%s: ema_warmup cannot be captured into a graph: the decay is a host scalar, "
                                 "a replay would keep the warm-up value of the captured step for ever; "
                                 "use a constant ema_decay" % self._name())
            self._ema_now = self.ema_decay_of_update(self._ema_updates)
        groups = self._current_groups()
        if groups and groups[0]["param"].is_cuda:
            wgrad_stream.join(groups[0]["param"].device)  # gradients from the side stream
        self._update(groups)
        self._steps += 1
        if self.ema_enabled:
            for st in groups:
                if self._ema_args(st)[0] is None:  # CPU, or the unfused route on the GPU
                    _ema_reference(st["ema"], st.get("master", st["param"]), 1.0 - self._ema_now)
            self._ema_updates += 1
        # the updated weights' W^T, one launch (ops/wt_cache.py)
        wt_cache.after_optimizer_step(p for grp in self.param_groups for p in grp["params"])
        return loss

    @torch.no_grad()
    def sync_from_params(self) -> None:
        """Re-seed the fp32 masters from the current working weights.  The masters
        are snapshotted when the flat state is built, so weights loaded afterwards
        without optimizer state (the reference's {'net','acc','epoch'} checkpoints,
        a plain ``model.load_state_dict``) must be adopted here, or the next step
        would overwrite them with the stale masters."""
        for st in self._state_groups():
            if "master" in st:
                st["master"].copy_(st["param"])
        self._seed_ema()  # an average of the replaced weights means nothing

    @torch.no_grad()
    def _seed_ema(self) -> None:
        for st in self._state_groups():
            if "ema" in st:
                st["ema"].copy_(st.get("master", st["param"]))
        self._ema_updates = 0

    def ema_tensors(self) -> List[torch.Tensor]:
        """Per parameter (``param_groups`` order) an fp32 view of its EMA slot, shaped like the parameter."""
        if not self.ema_enabled:
            raise RuntimeError("%s was built without ema_decay" % self._name())
        views = {}
        for gi, st in enumerate(self._current_groups()):
            for p, off in self._slots(gi):
                views[id(p)] = st["ema"].as_strided(p.shape, p.stride(), off)
        return [views[id(p)] for grp in self.param_groups for p in grp["params"]]

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model's working weights are the EMA
        (``ema.to(dtype)``); afterwards they are the live ones again, bit for
        bit.  The EMA and its update count are unchanged by a round trip.
        Buffers (BatchNorm running statistics) are not averaged: the live ones
        are used.  ``step()`` must not be called inside, and ``state_dict()`` /
        ``ema_tensors()`` not be read there: the EMA flat of an fp32 group
        without a master holds the live weights meanwhile."""
        if not self.ema_enabled:
            raise RuntimeError("%s was built without ema_decay" % self._name())
        if self._ema_swapped:
            raise RuntimeError("%s.ema_weights() is already entered" % self._name())
        groups = self._current_groups()
        params = [p for grp in self.param_groups for p in grp["params"]]

        def swap(st):  # fp32 parameters that are their own master: exchange contents
            tmp = st["param"].clone()
            st["param"].copy_(st["ema"])
            st["ema"].copy_(tmp)

        for st in groups:
            if "master" not in st and st["param"].dtype != torch.float32:
                raise RuntimeError("%s.ema_weights(): %s parameters without an fp32 master"
                                   % (self._name(), st["param"].dtype))
        with torch.no_grad():
            for st in groups:
                if "master" in st:
                    st["param"].copy_(st["ema"])  # rounds as .to(dtype)
                else:
                    swap(st)
            # writes through the flat do not bump p._version: cached W^T / casts are re-formed here
            wt_cache.after_optimizer_step(params)
        self._ema_swapped = True
        try:
            yield self
        finally:
            with torch.no_grad():
                for st in groups:
                    if "master" in st:
                        st["param"].copy_(st["master"])  # param == dtype(master), the step's invariant
                    else:
                        swap(st)
                wt_cache.after_optimizer_step(params)
            self._ema_swapped = False

    def _step_count(self) -> int:
        return self._steps

    def _set_step_count(self, n: int) -> None:
        self._steps = int(n)

    def _saved_keys(self) -> Tuple[str, ...]:
        return self.STATE_KEYS + (("master", "ema") if self.ema_enabled else ("master",))

    def _state_header(self) -> dict:
        sd = {"steps": self._step_count(),
              "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}
        if self.KIND != "sgd":  # SGD states keep the format older checkpoints have
            sd["kind"] = self.KIND
        if self.ema_enabled:
            sd["ema_updates"] = self._ema_updates
        return sd

    def _check_kind(self, sd) -> None:
        kind = sd.get("kind", "sgd") if isinstance(sd, dict) else None
        if kind != self.KIND:
            raise ForeignOptimizerState("%s.load_state_dict: the state was written by another kind of "
                                        "optimizer (%r, this one is %r)" % (self._name(), kind, self.KIND))

    def _load_header(self, sd) -> None:
        self._set_step_count(sd["steps"])
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            g.update(sg)
        self._ema_updates = int(sd.get("ema_updates", 0)) if self.ema_enabled else 0

    def _ema_after_load(self, sd) -> None:
        """A state written without EMA, loaded with EMA on: the average starts at the restored weights."""
        if self.ema_enabled and not all("ema" in sst for sst in sd["flat_state"]):
            self._seed_ema()
            warnings.warn("%s.load_state_dict: the state has no weight EMA; it starts from the restored "
                          "weights" % self._name())

    @torch.no_grad()
    def _params_follow_masters(self) -> None:
        for st in self._state_groups():
            if "master" in st:  # working weights follow the restored fp32 master
                st["param"].copy_(st["master"].to(st["param"].dtype))


# --------------------------------------------------------------------------- #
# layouts
# --------------------------------------------------------------------------- #
class _DDPLayout:
    """Flats borrowed from ``DistributedDataParallel(flat_parameters=True)``."""

    def _init_layout(self, ddp, master_weights: bool, ema_decay=None, ema_warmup=False) -> None:
        self._init_ema(ema_decay, ema_warmup)
        self.ddp = ddp
        self.master_weights = master_weights
        self._version = -1
        self._flat_state: List[dict] = []
        self._steps = 0

    # ------------------------------------------------------------------ #
    def _ensure_state(self) -> None:
        if self._version == self.ddp.layout_version:
            return
        groups = self.ddp.flat_groups()
        old = self._flat_state
        old_layout = getattr(self.ddp, "_last_old_layout", None)
        new_state = []
        for pflat, gflat in groups:
            st = {"param": pflat, "grad": gflat}
            self._alloc_state(st)
            new_state.append(st)
        if old and old_layout is not None:
            self._remap(old, new_state, old_layout, self.ddp.param_layout())
        self._flat_state = new_state
        self._version = self.ddp.layout_version

    @torch.no_grad()
    def _remap(self, old, new, old_layout, new_layout) -> None:
        """Carry the state / master buffers across a bucket rebuild."""
        for p, (og, oo), (ng, no) in zip(self.ddp._params, old_layout, new_layout):
            n = p.numel()
            for key in self._saved_keys():
                if key in old[og] and key in new[ng]:
                    new[ng][key].narrow(0, no, n).copy_(old[og][key].narrow(0, oo, n))

    def _current_groups(self) -> List[dict]:
        self._ensure_state()
        return self._flat_state

    def _state_groups(self) -> List[dict]:
        return self._flat_state

    def _layout_id(self) -> int:
        return self._version

    def _slots(self, gi: int):
        """(parameter, element offset) of every parameter in group `gi`."""
        return [(p, off) for p, (g, off) in zip(self.ddp._params, self.ddp.param_layout()) if g == gi]

    def zero_grad(self, set_to_none: bool = False):
        self.ddp.zero_grad()

    def state_dict(self):
        self._ensure_state()
        sd = self._state_header()
        sd["flat_state"] = [{k: v for k, v in st.items() if k in self._saved_keys()}
                            for st in self._flat_state]
        sd["layout"] = self.ddp.param_layout()
        return sd

    def load_state_dict(self, sd):
        """Restore state / master weights parameter by parameter.

        The saved flats follow the bucket layout of the run that wrote them
        (usually the post-rebuild autograd-ready order), while a fresh DDP
        starts in registration order -- so every parameter's slice is moved
        from ``sd['layout']`` to the current layout, never copied flat-to-flat.
        """
        self._check_kind(sd)
        if "layout" not in sd or "flat_state" not in sd:
            raise ForeignOptimizerState("%s.load_state_dict: not a %s state (e.g. a torch.optim "
                                        "state dict)" % (self._name(), self._name()))
        self._ensure_state()
        self._load_header(sd)
        dev = self._flat_state[0]["param"].device if self._flat_state else None
        saved = [{k: v.to(dev) for k, v in sst.items()} for sst in sd["flat_state"]]
        old_layout = [tuple(int(v) for v in e) for e in sd["layout"]]
        if len(old_layout) != len(self.ddp._params):
            raise ValueError("%s.load_state_dict: checkpoint has %d parameters, model has %d"
                             % (self._name(), len(old_layout), len(self.ddp._params)))
        self._remap(saved, self._flat_state, old_layout, self.ddp.param_layout())
        self._params_follow_masters()
        self._ema_after_load(sd)


class _ListLayout:
    """Flats built here for ANY parameter list: at construction the parameters
    of each dtype/device group are moved into one flat buffer (parameters
    become views, channels-last strides preserved) and their ``.grad`` is
    pre-set to views of a flat gradient buffer, so autograd accumulates in
    place and the update is one launch per group."""

    def _init_layout(self, params, master_weights: bool, ema_decay=None, ema_warmup=False) -> None:
        self._init_ema(ema_decay, ema_warmup)
        self.master_weights = master_weights
        self._steps = 0
        self._groups = []
        by_key = {}
        for p in params:
            by_key.setdefault((p.dtype, p.device), []).append(p)
        with torch.no_grad():
            for (dt, dev), ps in by_key.items():
                offs, o = [], 0
                for p in ps:
                    offs.append(o)
                    o += (p.numel() + 7) // 8 * 8  # kernel works in 8-element vectors
                pflat = torch.zeros(o, dtype=dt, device=dev)
                gflat = torch.zeros(o, dtype=dt, device=dev)
                gviews = []
                for p, off in zip(ps, offs):
                    view = pflat.as_strided(p.shape, p.stride(), off)
                    view.copy_(p.detach())
                    p.data = view
                    gv = gflat.as_strided(p.shape, p.stride(), off)
                    p.grad = gv
                    gviews.append(gv)
                st = {"params": ps, "offs": offs, "param": pflat, "grad": gflat, "gviews": gviews}
                self._alloc_state(st)
                self._groups.append(st)

    @torch.no_grad()
    def _adopt_grads(self, st) -> None:
        """Grads replaced behind our back (set_to_none, a stolen tensor) go back into the flat."""
        for p, gv in zip(st["params"], st["gviews"]):
            g = p.grad
            if g is gv or (g is not None and g.data_ptr() == gv.data_ptr() and g.stride() == gv.stride()):
                continue
            if g is None:
                gv.zero_()
            else:
                gv.copy_(g)
            p.grad = gv

    def _current_groups(self) -> List[dict]:
        for st in self._groups:
            self._adopt_grads(st)
        return self._groups

    def _state_groups(self) -> List[dict]:
        return self._groups

    def _layout_id(self) -> int:
        return 0

    def _slots(self, gi: int):
        st = self._groups[gi]
        return list(zip(st["params"], st["offs"]))

    def zero_grad(self, set_to_none: bool = False):
        """One fill per group; gradients stay flat views (``set_to_none`` is ignored)."""
        for st in self._groups:
            st["grad"].zero_()
            for p, gv in zip(st["params"], st["gviews"]):
                if p.grad is not gv:
                    p.grad = gv

    def _numels(self):
        return [[p.numel() for p in st["params"]] for st in self._groups]

    def state_dict(self):
        sd = self._state_header()
        sd["numels"] = self._numels()
        sd["flat_state"] = [{k: st[k] for k in self._saved_keys() if k in st} for st in self._groups]
        return sd

    def load_state_dict(self, sd):
        self._check_kind(sd)
        if "numels" not in sd or "flat_state" not in sd:
            raise ForeignOptimizerState("%s.load_state_dict: not a %s state (e.g. a torch.optim "
                                        "state dict)" % (self._name(), self._name()))
        if sd["numels"] != self._numels():
            raise ValueError("%s.load_state_dict: parameter layout differs from the checkpoint"
                             % self._name())
        self._load_header(sd)
        with torch.no_grad():
            for st, sst in zip(self._groups, sd["flat_state"]):
                for k, v in sst.items():
                    if k in st:
                        st[k].copy_(v)
        self._params_follow_masters()
        self._ema_after_load(sd)


# --------------------------------------------------------------------------- #
# update rules
# --------------------------------------------------------------------------- #
class _SGDRule:
    KIND = "sgd"
    STATE_KEYS = ("momentum",)

    @staticmethod
    def _sgd_defaults(lr, momentum, dampening, weight_decay, nesterov) -> dict:
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        return dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                    nesterov=nesterov)

    def _update(self, groups: List[dict]) -> None:
        g = self.param_groups[0]
        first = self._steps == 0
        for st in groups:
            pflat, gflat, master = st["param"], st["grad"], st.get("master")
            if pflat.is_cuda:
                _native.require(self._name()).sgd_flat_step(
                    master, st["momentum"], gflat, pflat, float(g["lr"]), float(g["weight_decay"]),
                    float(g["momentum"]), float(g["dampening"]), bool(g["nesterov"]), 1.0, first,
                    *self._ema_args(st))
            else:
                _sgd_reference(master, st["momentum"], gflat, pflat, g, first)


# hyper[] slots written by adamw_prepare (csrc/optim/fused_adamw.hip)
_BC1, _BC2, _NORM, _CLIP = range(4)
_SUMSQ_BLOCKS = 1024  # partial sums per group: 4 blocks per CU of an MI355X
_LR_CLASSES = 256     # entries of the lr-scale table: one per value of a class byte


class _AdamWRule:
    """torch.optim.AdamW (amsgrad=False, maximize=False), optionally after
    ``clip_grad_norm_(max_grad_norm)`` over ALL groups of the optimizer.

    The step count, the bias corrections, the gradient norm and the clip
    coefficient live in device tensors written by ``adamw_prepare``: ``step()``
    never syncs the host, and a step captured into a hipGraph advances them on
    every replay.  ``lr`` is passed as a host scalar (a captured graph bakes
    it, the constant-LR limit of ``--graph``).

    ``lr_scales`` (layer-wise lr decay for fine-tuning) maps parameters to a
    factor on ``lr``; a parameter not in it gets 1.0.  The update stays one
    launch per dtype group: every 8-element vector of a flat carries a class
    byte (``lr_class``, built like the decay mask and rebuilt with the layout)
    that indexes a 256-entry fp32 table on the device, read by
    ``adamw_flat_step_scaled`` (``csrc/optim/fused_adamw.hip``).  A
    scale of 0 freezes a tensor (its moments still update); with no scales, or
    all of them 1.0, the step is ``adamw_flat_step`` as before.  The scales are
    configuration, like ``lr``: they are not in ``state_dict()``, a resumed run
    passes them again.
    """

    KIND = "adamw"
    STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def _adamw_defaults(self, lr, betas, eps, weight_decay, max_grad_norm, no_decay_1d, amsgrad,
                        maximize) -> dict:
        if amsgrad or maximize:
            raise ValueError("%s: amsgrad and maximize are not supported" % self._name())
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("%s: betas must be in [0, 1), got %r" % (self._name(), (b1, b2)))
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError("%s: lr, eps and weight_decay must not be negative" % self._name())
        self.no_decay_1d = bool(no_decay_1d)
        self._dev_state: Dict[torch.device, dict] = {}
        self._partials: Optional[torch.Tensor] = None
        self._masks: List[Optional[torch.Tensor]] = []
        self._mask_key = None
        return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=weight_decay,
                    max_grad_norm=float(max_grad_norm or 0.0))

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("%s supports one param group (decay is switched per parameter by "
                             "no_decay_1d)" % self._name())
        super().add_param_group(param_group)

    # ------------------------------------------------------------------ #
    # per-parameter lr scales
    def _check_lr_scales(self, lr_scales) -> Dict[int, float]:
        own = {id(p) for grp in self.param_groups for p in grp["params"]}
        out: Dict[int, float] = {}
        for p, v in (lr_scales or {}).items():
            if id(p) not in own:
                raise ValueError("%s: lr_scales has a key that is not one of the optimizer's parameters"
                                 % self._name())
            v = float(v)
            if not math.isfinite(v) or v < 0.0:
                raise ValueError("%s: lr scales must be finite and not negative, got %r" % (self._name(), v))
            out[id(p)] = v
        values = sorted({out.get(i, 1.0) for i in own})
        if len(values) > _LR_CLASSES:
            raise ValueError("%s: %d distinct lr scales, at most %d fit the class byte"
                             % (self._name(), len(values), _LR_CLASSES))
        return out

    def _init_lr_scales(self, lr_scales) -> None:
        self._lr_dev: List[dict] = []  # per group: {"cls": uint8 [numel / 8], "table": fp32 [256]}
        self._lr_key = None
        self._lr_by_id = self._check_lr_scales(lr_scales)

    def _lr_values(self) -> List[float]:
        """The distinct scales, ascending: a parameter's class byte is its scale's index here."""
        return sorted({self._lr_by_id.get(id(p), 1.0) for grp in self.param_groups for p in grp["params"]})

    @property
    def lr_scaled(self) -> bool:
        """Some parameter's scale is not 1.0: ``step()`` runs the scaled kernel."""
        return any(v != 1.0 for v in self._lr_by_id.values())

    def lr_scale_of(self, p) -> float:
        return self._lr_by_id.get(id(p), 1.0)

    def lr_scale_range(self) -> Tuple[float, float]:
        """(min, max) of the scales over the optimizer's parameters (host-side)."""
        values = self._lr_values()
        return (values[0], values[-1]) if values else (1.0, 1.0)

    def _lr_host(self, gi: int, numel: int) -> Tuple[torch.Tensor, torch.Tensor]:
        values = self._lr_values()
        index = {v: i for i, v in enumerate(values)}
        cls = torch.zeros(numel // 8, dtype=torch.uint8)
        for p, off in self._aligned_slots(gi):
            cls[off // 8:(off + p.numel() + 7) // 8] = index[self.lr_scale_of(p)]  # the slot's padding too
        # a class no tensor uses poisons what reads it, rather than training it at some other rate
        table = torch.full((_LR_CLASSES,), float("nan"), dtype=torch.float32)
        table[:len(values)] = torch.tensor(values, dtype=torch.float64).float()
        return cls, table

    def _lr_tensors(self, groups: List[dict]) -> List[dict]:
        """Per group the class bytes and the table on the group's device,
        rebuilt when the layout changes (a DDP bucket rebuild), as the decay masks are."""
        key = (self._layout_id(), len(groups))
        if self._lr_key != key:
            dev = []
            for gi, st in enumerate(groups):
                cls, table = self._lr_host(gi, st["param"].numel())
                dev.append({"cls": cls.to(st["param"].device), "table": table.to(st["param"].device)})
            self._lr_dev, self._lr_key = dev, key
        return self._lr_dev

    @torch.no_grad()
    def set_lr_scales(self, lr_scales: Optional[Mapping[torch.nn.Parameter, float]]) -> None:
        """Replace the scales (``None``: all 1.0).  Class bytes and table that are
        already on the device are rewritten IN PLACE, so a step captured into a
        hipGraph with scales sees the new ones on its next replay (a step
        captured without scales runs the unscaled kernel and stays that way)."""
        self._lr_by_id = self._check_lr_scales(lr_scales)
        if self._lr_key is None:
            return
        groups = self._current_groups()
        if self._lr_key != (self._layout_id(), len(groups)):
            return  # stale: the next step rebuilds them
        for gi, (st, d) in enumerate(zip(groups, self._lr_dev)):
            cls, table = self._lr_host(gi, st["param"].numel())
            d["cls"].copy_(cls)
            d["table"].copy_(table)

    # ------------------------------------------------------------------ #
    def _device_state(self, dev: torch.device) -> dict:
        ds = self._dev_state.get(dev)
        if ds is None:
            ds = {"step": torch.full((1,), self._steps, dtype=torch.int64, device=dev),
                  "hyper": torch.tensor([1.0, 1.0, 0.0, 1.0], dtype=torch.float32, device=dev)}
            self._dev_state[dev] = ds
        return ds

    def _clip_devices(self, groups: List[dict]) -> List[torch.device]:
        devs = list(dict.fromkeys(st["param"].device for st in groups))
        if self.param_groups[0]["max_grad_norm"] > 0 and len(devs) > 1:
            raise ValueError("%s: max_grad_norm is a global norm, all parameters must be on one "
                             "device (got %s)" % (self._name(), ", ".join(str(d) for d in devs)))
        return devs

    def _decay_masks(self, groups: List[dict]) -> List[Optional[torch.Tensor]]:
        """One uint8 per 8-element vector of each group's flat: 1 = weight decay
        applies.  Every parameter's slot is padded to 8 elements, so a vector
        belongs to one parameter.  ``None``: decay everywhere."""
        if not self.no_decay_1d:
            return [None] * len(groups)
        key = (self._layout_id(), len(groups))
        if self._mask_key != key:
            masks = []
            for gi, st in enumerate(groups):
                mask = torch.ones(st["param"].numel() // 8, dtype=torch.uint8)
                for p, off in self._aligned_slots(gi):
                    if p.dim() <= 1:  # biases, LayerNorm / BatchNorm weights
                        mask[off // 8:(off + p.numel() + 7) // 8] = 0
                masks.append(mask.to(st["param"].device))
            self._masks, self._mask_key = masks, key
        return self._masks

    def _update(self, groups: List[dict]) -> None:
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        clip = float(g["max_grad_norm"] or 0.0)
        devs = self._clip_devices(groups)
        if not groups:
            return
        masks = self._decay_masks(groups)
        # a step that has ever run scaled keeps reading the device tables (a captured one does anyway)
        scaled = self.lr_scaled or self._lr_key == (self._layout_id(), len(groups))
        scales = self._lr_tensors(groups) if scaled else [None] * len(groups)
        part = None
        if clip > 0:
            part = self._partials
            if part is None or part.shape[0] != len(groups) or part.device != devs[0]:
                part = self._partials = torch.zeros(len(groups), _SUMSQ_BLOCKS, dtype=torch.float32,
                                                    device=devs[0])
            for i, st in enumerate(groups):
                if st["grad"].is_cuda:
                    _native.require(self._name()).flat_sumsq_partials(st["grad"], part[i])
                else:
                    _sumsq_reference(st["grad"], part[i])
        for dev in devs:
            ds = self._device_state(dev)
            if dev.type == "cuda":
                _native.require(self._name()).adamw_prepare(part, ds["hyper"], ds["step"], clip,
                                                            float(b1), float(b2))
            else:
                _adamw_prepare_reference(part, ds["hyper"], ds["step"], clip, b1, b2)
        for st, mask, sc in zip(groups, masks, scales):
            pflat = st["param"]
            hyper = self._dev_state[pflat.device]["hyper"]
            if pflat.is_cuda and sc is not None:
                _native.require(self._name()).adamw_flat_step_scaled(
                    st.get("master"), st["exp_avg"], st["exp_avg_sq"], st["grad"], pflat, mask, hyper,
                    sc["cls"], sc["table"], float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                    float(g["weight_decay"]), *self._ema_args(st))
            elif pflat.is_cuda:
                _native.require(self._name()).adamw_flat_step(
                    st.get("master"), st["exp_avg"], st["exp_avg_sq"], st["grad"], pflat, mask, hyper,
                    float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]),
                    *self._ema_args(st))
            else:
                _adamw_reference(st.get("master"), st["exp_avg"], st["exp_avg_sq"], st["grad"], pflat,
                                 mask, hyper, g, None if sc is None else sc["table"][sc["cls"].long()])

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Total gradient norm of the last step as a device scalar (reading it is
        the caller's sync); ``None`` while clipping is off or before a step."""
        if not self.param_groups[0]["max_grad_norm"] > 0 or not self._dev_state:
            return None
        return next(iter(self._dev_state.values()))["hyper"][_NORM]

    # the step count is the device tensor's: a replayed graph advances only that
    def _step_count(self) -> int:
        if self._dev_state:
            return int(next(iter(self._dev_state.values()))["step"].item())
        return self._steps

    def _set_step_count(self, n: int) -> None:
        self._steps = int(n)
        for ds in self._dev_state.values():
            ds["step"].fill_(int(n))


# coef[] columns written by lars_trust (csrc/optim/fused_lars.hip): trust ratio, weight decay, |w|, |g|
_TRUST, _COEF_COLS = 0, 4


class _LARSRule:
    """LARS (You et al. 2017) with momentum: per tensor
    ``trust = eta |w| / (|g| + wd |w| + eps)`` (1 where ``|w|`` or ``|g|`` is
    exactly 0), ``d = trust (g + wd w)``, ``m <- mu m + d``, ``w <- w - lr m``.
    With ``exclude_1d`` parameters with ``ndim <= 1`` (biases, BatchNorm /
    LayerNorm weights) get ``trust = 1`` and no weight decay: ``d = g``.

    The norms are taken over the fp32 masters (the fp32 parameters where there
    is no master) and the averaged gradient, per tensor, by a segmented
    reduction over the flats: three launches per dtype group whatever the number
    of tensors.  Norms and trust ratios stay on the device, so ``step()`` never
    syncs the host and a step captured into a hipGraph stays correct on replay;
    ``lr`` is a host scalar outside the momentum, as in the SGD classes (the
    schedules write ``param_groups[0]['lr']``).  Gradients are equal on every
    rank after the all-reduce and the norms are per tensor, so LARS needs no
    communication of its own and works per stage in a pipeline.
    """

    KIND = "lars"
    STATE_KEYS = ("momentum",)

    def _lars_defaults(self, lr, momentum, weight_decay, trust_coefficient, eps, exclude_1d) -> dict:
        if lr < 0 or momentum < 0 or weight_decay < 0 or trust_coefficient <= 0 or eps < 0:
            raise ValueError("%s: lr, momentum, weight_decay and eps must not be negative, "
                             "trust_coefficient must be positive" % self._name())
        self.exclude_1d = bool(exclude_1d)
        self._plans: List[dict] = []
        self._plan_key = None
        self._stepped = False
        return dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                    trust_coefficient=trust_coefficient, eps=eps)

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("%s supports one param group (adaptation is switched per parameter by "
                             "exclude_1d)" % self._name())
        super().add_param_group(param_group)

    def _lars_plans(self, groups: List[dict]) -> List[dict]:
        """Per group, the work items of the segmented reduction and the update,
        built on the host once per layout and kept on the group's device:

        ``items``    int32 [I, 3]: first vector, vector count, tensor -- every
                     parameter's slot cut into pieces of at most
                     ``lars_chunk_elems()`` elements, none across a boundary
        ``tensors``  int32 [T, 3]: first item, item count, adapted?  (``_slots`` order)
        ``partials`` fp32 [I, 2], ``coef`` fp32 [T, 4]: the kernels' outputs
        """
        key = (self._layout_id(), len(groups))
        if self._plan_key == key:
            return self._plans
        plans = []
        for gi, st in enumerate(groups):
            dev = st["param"].device
            # vectors per work item (the CPU path works on `spans`: one item per tensor there)
            chunk = _native.require(self._name()).lars_chunk_elems() // 8 if dev.type == "cuda" else 1 << 30
            items, tensors, spans = [], [], []
            nitems = 0
            for t, (p, off) in enumerate(self._aligned_slots(gi)):
                nvec = (p.numel() + 7) // 8
                adapted = not self.exclude_1d or p.dim() > 1
                first = torch.arange(off // 8, off // 8 + nvec, chunk, dtype=torch.int32)
                count = torch.clamp(off // 8 + nvec - first, max=chunk)
                items.append(torch.stack([first, count, torch.full_like(first, t)], dim=1))
                tensors.append((nitems, first.numel(), int(adapted)))
                spans.append((off, nvec * 8, adapted))
                nitems += first.numel()
            items = torch.cat(items) if items else torch.zeros(0, 3, dtype=torch.int32)
            tensors = torch.tensor(tensors, dtype=torch.int32).reshape(-1, 3)
            plans.append({"items": items.contiguous().to(dev), "tensors": tensors.to(dev), "spans": spans,
                          "adapted": tensors[:, 2].bool().to(dev),
                          "partials": torch.zeros(nitems, 2, dtype=torch.float32, device=dev),
                          "coef": torch.zeros(len(spans), _COEF_COLS, dtype=torch.float32, device=dev)})
        self._plans, self._plan_key = plans, key
        return plans

    def _update(self, groups: List[dict]) -> None:
        g = self.param_groups[0]
        if not groups:
            return
        for st, plan in zip(groups, self._lars_plans(groups)):
            pflat, master = st["param"], st.get("master")
            if pflat.is_cuda:
                C = _native.require(self._name())
                C.lars_norm_partials(master, st["grad"], pflat, plan["items"], plan["partials"])
                C.lars_trust(plan["partials"], plan["tensors"], plan["coef"], float(g["trust_coefficient"]),
                             float(g["weight_decay"]), float(g["eps"]))
                C.lars_flat_step(master, st["momentum"], st["grad"], pflat, plan["items"], plan["coef"],
                                 float(g["lr"]), float(g["momentum"]), *self._ema_args(st))
            else:
                _lars_reference(master, st["momentum"], st["grad"], pflat, plan["spans"], plan["coef"], g)
        self._stepped = True

    @property
    def last_trust_ratios(self) -> Optional[List[torch.Tensor]]:
        """The last step's trust ratios: one fp32 device tensor per dtype group,
        one value per parameter in ``_slots(group)`` order, 1 for an excluded
        parameter (reading it is the caller's sync); ``None`` before a step."""
        if not self._stepped or self._plan_key is None:
            return None
        return [plan["coef"][:, _TRUST] for plan in self._plans]

    def last_trust_range(self) -> Optional[Tuple[float, float]]:
        """(min, max) of the last step's trust ratios over the adapted
        parameters (this reads the device: once per epoch in the trainer)."""
        ratios = self.last_trust_ratios
        if ratios is None:
            return None
        vals = [r[plan["adapted"]] for r, plan in zip(ratios, self._plans)]
        vals = torch.cat([v.float().cpu() for v in vals]) if vals else torch.zeros(0)
        if vals.numel() == 0:
            return None
        return float(vals.min()), float(vals.max())


# --------------------------------------------------------------------------- #
# the six optimizers
# --------------------------------------------------------------------------- #
def _trainable_of_one_group(params, name: str, switch: str) -> list:
    """The trainable parameters of a parameter list, or of a list of exactly one param-group dict."""
    params = list(params)
    if params and isinstance(params[0], dict):
        if len(params) > 1:
            raise ValueError("%s supports one param group (%s)" % (name, switch))
        params = list(params[0]["params"])
    return [p for p in params if p.requires_grad]


class FlatSGD(_SGDRule, _DDPLayout, _FlatOptimizer):
    def __init__(self, ddp, lr: float, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, master_weights: bool = True,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        defaults = self._sgd_defaults(lr, momentum, dampening, weight_decay, nesterov)
        super().__init__(list(ddp._params), defaults)
        self._init_layout(ddp, master_weights, ema_decay, ema_warmup)


class MasterSGD(_SGDRule, _ListLayout, _FlatOptimizer):
    """torch.optim.SGD semantics with fp32 master weights for ANY parameter list.

    Used where there is no DDP flat layout to borrow: single-process
    DataParallel (its parameters live on ``device_ids[0]``), pipeline stages
    and plain single-GPU training.  The update is ONE ``sgd_flat_step`` launch
    per dtype/device group, fp32 master + fp32 momentum for bf16 groups (bf16
    SGD would drop every update below one bf16 ulp).  Same kernel and numerics
    as :class:`FlatSGD` under DDP, so DP, pipeline and DDP train at equal
    precision.
    """

    def __init__(self, params, lr: float, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, master_weights: bool = True,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        defaults = self._sgd_defaults(lr, momentum, dampening, weight_decay, nesterov)
        params = [p for p in params if p.requires_grad]
        super().__init__(params, defaults)
        self._init_layout(params, master_weights, ema_decay, ema_warmup)


class FlatAdamW(_AdamWRule, _DDPLayout, _FlatOptimizer):
    """AdamW + global-norm clipping on the DDP flat buffers (twin of :class:`FlatSGD`).

    ``no_decay_1d`` switches weight decay off for parameters with ``ndim <= 1``
    (biases, LayerNorm / BatchNorm weights) and nothing else: a ViT's
    ``cls_token`` and ``pos_embedding`` are 3-D and keep decay, as in
    torchvision's reference recipe.  ``max_grad_norm`` (``None`` / 0 = off)
    clips the gradient of the whole model to that norm before the update.
    """

    def __init__(self, ddp, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, no_decay_1d: bool = True,
                 master_weights: bool = True, amsgrad: bool = False, maximize: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False,
                 lr_scales: Optional[Mapping[torch.nn.Parameter, float]] = None):
        defaults = self._adamw_defaults(lr, betas, eps, weight_decay, max_grad_norm, no_decay_1d,
                                        amsgrad, maximize)
        super().__init__(list(ddp._params), defaults)
        self._init_lr_scales(lr_scales)
        self._init_layout(ddp, master_weights, ema_decay, ema_warmup)


class MasterAdamW(_AdamWRule, _ListLayout, _FlatOptimizer):
    """:class:`FlatAdamW` for ANY parameter list (twin of :class:`MasterSGD`)."""

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None,
                 no_decay_1d: bool = True, master_weights: bool = True, amsgrad: bool = False,
                 maximize: bool = False, ema_decay: Optional[float] = None, ema_warmup: bool = False,
                 lr_scales: Optional[Mapping[torch.nn.Parameter, float]] = None):
        defaults = self._adamw_defaults(lr, betas, eps, weight_decay, max_grad_norm, no_decay_1d,
                                        amsgrad, maximize)
        params = _trainable_of_one_group(params, "MasterAdamW", "decay is switched per parameter by no_decay_1d")
        super().__init__(params, defaults)
        self._init_lr_scales(lr_scales)
        self._init_layout(params, master_weights, ema_decay, ema_warmup)
        self._clip_devices(self._groups)


class FlatLARS(_LARSRule, _DDPLayout, _FlatOptimizer):
    """LARS with momentum on the DDP flat buffers (twin of :class:`FlatSGD`), the
    optimizer of large-batch ResNet recipes.  ``exclude_1d`` keeps parameters
    with ``ndim <= 1`` (biases, BatchNorm / LayerNorm weights) on plain momentum
    SGD without weight decay."""

    def __init__(self, ddp, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 trust_coefficient: float = 1e-3, eps: float = 1e-8, exclude_1d: bool = True,
                 master_weights: bool = True,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        defaults = self._lars_defaults(lr, momentum, weight_decay, trust_coefficient, eps, exclude_1d)
        super().__init__(list(ddp._params), defaults)
        self._init_layout(ddp, master_weights, ema_decay, ema_warmup)


class MasterLARS(_LARSRule, _ListLayout, _FlatOptimizer):
    """:class:`FlatLARS` for ANY parameter list (twin of :class:`MasterSGD`)."""

    def __init__(self, params, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 trust_coefficient: float = 1e-3, eps: float = 1e-8, exclude_1d: bool = True,
                 master_weights: bool = True,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        defaults = self._lars_defaults(lr, momentum, weight_decay, trust_coefficient, eps, exclude_1d)
        params = _trainable_of_one_group(params, "MasterLARS",
                                         "adaptation is switched per parameter by exclude_1d")
        super().__init__(params, defaults)
        self._init_layout(params, master_weights, ema_decay, ema_warmup)


def build_optimizer(kind: str, target, flat: bool, lr: float, momentum: float = 0.9,
                    weight_decay: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                    clip_grad_norm: float = 0.0, trust_coefficient: float = 1e-3,
                    ema_decay: Optional[float] = None, ema_warmup: bool = False,
                    lr_scales: Optional[Mapping[torch.nn.Parameter, float]] = None):
    """The trainer's optimizer: ``kind`` sgd | adamw | lars; ``flat`` picks the
    DDP-flat class (``target`` is the DDP wrapper) over the parameter-list one.
    ``ema_decay`` (``None`` / 0 = off) keeps a weight EMA in the optimizer;
    ``lr_scales`` (adamw only) maps parameters to a factor on ``lr``."""
    if kind in ("sgd", "lars") and clip_grad_norm:
        raise ValueError("gradient clipping needs optimizer='adamw'")
    if kind in ("sgd", "lars") and lr_scales is not None:
        raise ValueError("per-parameter lr scales (layer-wise lr decay) need optimizer='adamw'")
    ema = dict(ema_decay=ema_decay, ema_warmup=ema_warmup)
    if kind == "sgd":
        return (FlatSGD if flat else MasterSGD)(target, lr=lr, momentum=momentum, weight_decay=weight_decay,
                                                **ema)
    if kind == "adamw":
        return (FlatAdamW if flat else MasterAdamW)(target, lr=lr, betas=betas, eps=eps,
                                                    weight_decay=weight_decay,
                                                    max_grad_norm=clip_grad_norm or None,
                                                    lr_scales=lr_scales, **ema)
    if kind == "lars":
        return (FlatLARS if flat else MasterLARS)(target, lr=lr, momentum=momentum, weight_decay=weight_decay,
                                                  trust_coefficient=trust_coefficient, eps=eps, **ema)
    raise ValueError(f"unknown optimizer {kind!r} (sgd | adamw | lars)")


# --------------------------------------------------------------------------- #
# PyTorch implementations of the kernels (CPU path / test oracle)
# --------------------------------------------------------------------------- #
def _ema_reference(ema: torch.Tensor, w: torch.Tensor, omd: float) -> None:
    """``ema += omd * (w - ema)`` in fp32: the CPU path, and the unfused GPU
    route (one more read of the weights and one more launch than the kernels')."""
    ema.lerp_(w if w.dtype == torch.float32 else w.float(), float(omd))


def _sgd_reference(master: Optional[torch.Tensor], mom: torch.Tensor, grad: torch.Tensor,
                   param: torch.Tensor, g: dict, first: bool) -> None:
    """PyTorch implementation of the flat kernel (CPU path / test oracle)."""
    w = master if master is not None else param
    d = grad.float() + g["weight_decay"] * w.float()
    if g["momentum"] != 0:
        if first:
            mom.copy_(d)
        else:
            mom.mul_(g["momentum"]).add_(d, alpha=1 - g["dampening"])
        d = d + g["momentum"] * mom if g["nesterov"] else mom
    w.add_(d.to(w.dtype), alpha=-g["lr"])
    if master is not None:
        param.copy_(master.to(param.dtype))


def _lars_reference(master: Optional[torch.Tensor], mom: torch.Tensor, grad: torch.Tensor,
                    param: torch.Tensor, spans, coef: torch.Tensor, g: dict) -> None:
    """PyTorch implementation of the three LARS kernels, fp32 like them (norms
    and trust ratio in double).  ``spans``: (offset, padded length, adapted?) per
    tensor; ``coef`` [T, 4] receives {trust, weight decay, |w|, |g|}."""
    w = master if master is not None else param
    wf = w if w.dtype == torch.float32 else w.float()
    eta, wd, eps = float(g["trust_coefficient"]), float(g["weight_decay"]), float(g["eps"])
    for t, (off, n, adapted) in enumerate(spans):
        ws, ms = wf.narrow(0, off, n), mom.narrow(0, off, n)
        gs = grad.narrow(0, off, n).float()
        wn, gn = ws.double().norm(), gs.double().norm()
        trust, decay = 1.0, 0.0
        if adapted:
            decay = wd
            if float(wn) != 0.0 and float(gn) != 0.0:
                trust = float(eta * wn / (gn + wd * wn + eps))
        coef[t] = torch.tensor([trust, decay, float(wn), float(gn)], dtype=torch.float32)
        d = gs + decay * ws if decay else gs
        if trust != 1.0:
            d = d * torch.tensor(trust, dtype=torch.float32)
        ms.mul_(g["momentum"]).add_(d)
        ws.sub_(ms, alpha=g["lr"])
    if wf is not w:
        w.copy_(wf.to(w.dtype))
    if master is not None:
        param.copy_(master.to(param.dtype))


def _sumsq_reference(grad: torch.Tensor, partials_row: torch.Tensor) -> None:
    partials_row.zero_()
    partials_row[0] = grad.float().pow(2).sum()


def _adamw_prepare_reference(partials: Optional[torch.Tensor], hyper: torch.Tensor, step: torch.Tensor,
                             max_norm: float, beta1: float, beta2: float) -> None:
    step += 1
    t = int(step.item())
    hyper[_BC1] = 1.0 - float(beta1) ** t
    hyper[_BC2] = 1.0 - float(beta2) ** t
    if max_norm > 0 and partials is not None:
        norm = partials.double().sum().sqrt()
        hyper[_NORM] = norm.float()
        hyper[_CLIP] = (max_norm / (norm + 1e-6)).clamp(max=1.0).float()
    else:
        hyper[_NORM] = 0.0
        hyper[_CLIP] = 1.0


def _adamw_reference(master: Optional[torch.Tensor], exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                     grad: torch.Tensor, param: torch.Tensor, decay_mask: Optional[torch.Tensor],
                     hyper: torch.Tensor, g: dict, scale: Optional[torch.Tensor] = None) -> None:
    """PyTorch implementation of adamw_flat_step, fp32 like the kernel; with
    ``scale`` (fp32 [numel / 8], one lr factor per 8-element vector) of
    adamw_flat_step_scaled: a vector with scale 1 takes the arithmetic of the
    unscaled call, any other one ``lr * scale`` in fp32, and a vector with
    scale 0 keeps its weights bit for bit while its moments update."""
    w = master if master is not None else param
    b1, b2 = g["betas"]
    wf = w if w.dtype == torch.float32 else w.float()
    gr = grad.float() * hyper[_CLIP]
    decay = 1.0 - g["lr"] * g["weight_decay"]
    step = g["lr"] / hyper[_BC1]
    frozen = None
    if scale is not None:
        sv = scale.to(device=wf.device, dtype=torch.float32).repeat_interleave(8)
        unit, frozen = sv == 1, sv == 0
        lr_v = torch.tensor(g["lr"], dtype=torch.float32, device=wf.device) * sv
        decay = torch.where(unit, torch.tensor(decay, dtype=torch.float32, device=wf.device),
                            1.0 - lr_v * g["weight_decay"])
        step = torch.where(unit, step, lr_v / hyper[_BC1])
        w0 = wf.clone()
    if decay_mask is None:
        wf.mul_(decay)
    else:
        keep = decay_mask.repeat_interleave(8) != 0
        wf.mul_(torch.where(keep, torch.as_tensor(decay, dtype=torch.float32, device=wf.device),
                            torch.ones((), dtype=torch.float32, device=wf.device)))
    exp_avg.mul_(b1).add_(gr, alpha=1 - b1)
    exp_avg_sq.mul_(b2).addcmul_(gr, gr, value=1 - b2)
    denom = (exp_avg_sq.sqrt() / hyper[_BC2].sqrt()).add_(g["eps"])  # sqrt(v) + eps: 0 / eps = 0
    wf.sub_(step * (exp_avg / denom))
    if frozen is not None:
        wf.copy_(torch.where(frozen, w0, wf))
    if wf is not w:
        w.copy_(wf.to(w.dtype))
    if master is not None:
        param.copy_(master.to(param.dtype))
