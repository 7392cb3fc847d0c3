"""Optimizers over :class:`pcmp.utils.flat.FlatParams` (one fused kernel per step) and LR schedules.

Reference parity:
  * ``SGD``   — Keras ``SGD(lr=0.001)`` (resnet.py:24) and the north-star ResNet SGD;
  * ``Adam``  — ``optim.Adam(model.fc.parameters(), lr=0.003)`` (another_neural_net.py:114) and
    ``optim.Adam(model.parameters())`` (:258);
  * ``AdamW`` — HF ``AdamW(lr=2e-5, eps=1e-8)`` (pytorch_on_language_distr.py:167-170; HF's default
    weight_decay 0.0);
  * ``linear_schedule_with_warmup`` — ``get_linear_schedule_with_warmup`` (:182-183);
  * ``clip_grad_norm`` — ``clip_grad_norm_(model.parameters(), 1.0)`` (:271-273), computed on
    device and applied inside the optimizer kernel (no host sync).
LR and step live in device scalars so a captured hipGraph replays correctly across steps.

Parameter groups (``groups=``): per-group learning-rate multiplier and weight decay, still one launch
per step.  The groups become a per-run table on the device (:class:`ParamGroups`) that
``sgd_flat_groups`` / ``adam_flat_groups`` look up per 4-element vector; an optimizer built without
groups stays on the table-free ``sgd_flat`` / ``adam_flat``.  Both paths instantiate the one definition
of the arithmetic (csrc/optim.hip ``sgd_update`` / ``adam_update``).  ``no_decay_1d`` /
``backbone_head_groups`` build the two standard groupings, ``compose_groups`` intersects them.
"""
from __future__ import annotations

import math

import torch

from .ops.kernels import K
from .ops.params import bump_weight_gen
from .utils.flat import FlatParams


MAX_RUNS = 2048   # csrc/optim.hip kMaxRuns: the run table is staged in LDS


class ParamGroups:
    """The groups of one optimizer over one arena, resolved to the kernels' run table.

    ``groups`` is a list of dicts as in torch: ``{"params": [...], "lr_mult": 1.0, "weight_decay":
    wd}`` (both settings optional: ``lr_mult`` defaults to 1, ``weight_decay`` to ``default_wd``).
    Arena parameters that no group lists form one more group with the defaults.  A parameter listed
    twice, or one that is not in the arena, is a ``ValueError``."""

    def __init__(self, flat: FlatParams, groups, default_wd: float = 0.0):
        in_arena = {id(p) for p in flat.params}
        owner = {}
        self.lr_mult, self.weight_decay = [], []
        for gi, grp in enumerate(groups):
            unknown = set(grp) - {"params", "lr_mult", "weight_decay"}
            if unknown or "params" not in grp:
                raise ValueError(f"parameter group {gi}: needs 'params', takes 'lr_mult' and 'weight_decay' "
                                 f"(got {sorted(grp)})")
            for p in grp["params"]:
                if id(p) not in in_arena:
                    raise ValueError(f"parameter group {gi}: a parameter of shape {tuple(p.shape)} is not in the "
                                     f"optimizer's arena (frozen, or of another model)")
                if id(p) in owner:
                    raise ValueError(f"parameter group {gi}: a parameter of shape {tuple(p.shape)} is already in "
                                     f"group {owner[id(p)]}")
                owner[id(p)] = gi
            self.lr_mult.append(float(grp.get("lr_mult", 1.0)))
            self.weight_decay.append(float(grp.get("weight_decay", default_wd)))
        if len(owner) < len(flat.params):   # the default group
            self.lr_mult.append(1.0)
            self.weight_decay.append(float(default_wd))
        default = len(self.lr_mult) - 1
        self.numel = [0] * len(self.lr_mult)
        for p in flat.params:
            self.numel[owner.get(id(p), default)] += p.numel()
        self.runs = flat.runs(lambda p: owner.get(id(p), default))
        # what the kernels cannot check without reading the table back: increasing multiples of 16
        # that end at the arena size
        ends = [e for _, e, _ in self.runs]
        assert ends[-1] == flat.numel and all(e % 16 == 0 for e in ends) and all(a < b for a, b in zip(ends, ends[1:]))
        if len(ends) > MAX_RUNS:
            raise ValueError(f"{len(ends)} runs of adjacent same-group parameters; the kernels take {MAX_RUNS}")
        dev = flat.device
        self.arena_size = flat.numel
        self.run_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self.run_lr_mult = torch.tensor([self.lr_mult[g] for _, _, g in self.runs], dtype=torch.float32, device=dev)
        self.run_wd = torch.tensor([self.weight_decay[g] for _, _, g in self.runs], dtype=torch.float32, device=dev)

    def table(self, base):
        """The table arguments of the grouped ops for the slice of the arena that starts at ``base``."""
        return self.run_end, self.run_lr_mult, self.run_wd, base, self.arena_size

    def describe(self):
        """Per group: lr_mult, weight_decay, parameter elements and number of runs (the ``--json`` field)."""
        nruns = [0] * len(self.lr_mult)
        for _, _, g in self.runs:
            nruns[g] += 1
        return [{"lr_mult": m, "weight_decay": w, "numel": n, "runs": r}
                for m, w, n, r in zip(self.lr_mult, self.weight_decay, self.numel, nruns)]

    def state_dict(self):
        return {"groups": [{"lr_mult": m, "weight_decay": w} for m, w in zip(self.lr_mult, self.weight_decay)],
                "runs": [list(r) for r in self.runs]}


class _FlatOptimizer:
    def __init__(self, flat: FlatParams, lr: float, groups=None, weight_decay: float = 0.0):
        self.flat = flat
        self.groups = ParamGroups(flat, groups, weight_decay) if groups is not None else None
        dev = flat.device
        self.lr_t = torch.tensor([float(lr)], dtype=torch.float32, device=dev)
        self._lr = float(lr)
        self.base_lr = float(lr)
        self.grad_scale = None   # optional device scalar (clip coef * 1/world)
        self.steps = 0

    @property
    def lr(self):
        return self._lr

    def set_lr(self, lr: float):
        self._lr = float(lr)
        self.lr_t.fill_(self._lr)

    def zero_grad(self, set_to_none: bool = True):
        self.flat.zero_grad()

    def clip_grad_norm(self, max_norm: float, pre_scale: float = 1.0, post_scale: float = 1.0):
        """Global L2 norm of (pre_scale * grad); sets the device-side multiplier
        ``min(1, max_norm/norm) * post_scale`` consumed by the next ``step``.  Returns the norm
        as a device tensor (no sync)."""
        norm, coef = K.grad_clip_coef(self.flat.grad, pre_scale, max_norm, post_scale)
        self.grad_scale = coef
        return norm

    def set_grad_scale(self, scale: float | None):
        if scale is None or scale == 1.0:
            self.grad_scale = None
        else:
            self.grad_scale = torch.tensor([float(scale)], device=self.flat.device)

    # ---- ranged steps: DistributedDataParallel.finish_gradient_sync(opt=...) updates each gradient
    # bucket as soon as its all-reduce completes: begin_step(), step_range() per flat slice, end_step().
    # The same elementwise kernel over a sub-range: bitwise equal to step() over the whole arena.
    def begin_step(self):
        pass

    def step_range(self, lo: int, hi: int):
        raise NotImplementedError

    def end_step(self):
        self.steps += 1
        bump_weight_gen()

    def step(self):
        self.begin_step()
        self.step_range(0, self.flat.numel)
        self.end_step()

    def state_dict(self):
        sd = {"lr": self._lr, "steps": self.steps, "state": {k: v.detach().clone() for k, v in self._state().items()}}
        if self.groups is not None:
            sd["param_groups"] = self.groups.state_dict()
        return sd

    def load_state_dict(self, sd):
        """Raises ``ValueError`` when the checkpoint's parameter groups are not this optimizer's: the
        state would otherwise continue under another grouping without a word."""
        want = self.groups.state_dict() if self.groups is not None else None
        got = sd.get("param_groups")
        if got is not None:
            got = {"groups": [dict(g) for g in got["groups"]], "runs": [list(r) for r in got["runs"]]}
        if got != want:
            raise ValueError("load_state_dict: parameter groups differ -- checkpoint "
                             f"{'without groups' if got is None else got['groups']}, optimizer "
                             f"{'without groups' if want is None else want['groups']}"
                             + ("" if got is None or want is None or got["groups"] != want["groups"]
                                else " (same settings, another run table)"))
        self.set_lr(sd["lr"])
        self.steps = sd["steps"]
        for k, v in self._state().items():
            v.copy_(sd["state"][k].to(v.device))

    def _state(self):
        return {}


class SGD(_FlatOptimizer):
    def __init__(self, flat, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, groups=None):
        super().__init__(flat, lr, groups, weight_decay)
        self.momentum, self.dampening, self.wd, self.nesterov = momentum, dampening, weight_decay, nesterov
        self.mom = torch.zeros_like(flat.master) if momentum != 0 else flat.master.new_empty(0)

    def step_range(self, lo, hi):
        f = self.flat
        bufs = (f.master[lo:hi], f.grad[lo:hi], self.mom[lo:hi] if self.mom.numel() else self.mom,
                f.shadow[lo:hi] if f.shadow is not None else None)
        scalars, tail = (self.lr_t, self.grad_scale), (self.nesterov, self.steps == 0)
        if self.groups is None:
            K.sgd_flat(*bufs, None, *scalars, self.momentum, self.dampening, self.wd, *tail)
        else:
            K.sgd_flat_groups(*bufs, *scalars, *self.groups.table(lo), self.momentum, self.dampening, *tail)

    def _state(self):
        return {"mom": self.mom}


class Adam(_FlatOptimizer):
    decoupled = False

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, groups=None):
        super().__init__(flat, lr, groups, weight_decay)
        self.beta1, self.beta2 = betas
        self.eps, self.wd = eps, weight_decay
        self.m1 = torch.zeros_like(flat.master)
        self.m2 = torch.zeros_like(flat.master)
        self.step_t = torch.zeros(1, dtype=torch.float32, device=flat.device)

    def begin_step(self):
        self.step_t.add_(1.0)

    def step_range(self, lo, hi):
        f = self.flat
        bufs = (f.master[lo:hi], f.grad[lo:hi], self.m1[lo:hi], self.m2[lo:hi],
                f.shadow[lo:hi] if f.shadow is not None else None)
        scalars, hyper = (self.lr_t, self.grad_scale, self.step_t), (self.beta1, self.beta2, self.eps)
        if self.groups is None:
            K.adam_flat(*bufs, None, *scalars, *hyper, self.wd, self.decoupled)
        else:
            K.adam_flat_groups(*bufs, *scalars, *self.groups.table(lo), *hyper, self.decoupled)

    def _state(self):
        return {"m1": self.m1, "m2": self.m2, "step_t": self.step_t}


class AdamW(Adam):
    decoupled = True

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, groups=None):
        super().__init__(flat, lr, betas, eps, weight_decay, groups)


class LambdaLR:
    def __init__(self, opt: _FlatOptimizer, fn):
        self.opt, self.fn, self.last_step = opt, fn, 0
        opt.set_lr(opt.base_lr * fn(0))

    def step(self):
        self.last_step += 1
        self.opt.set_lr(self.opt.base_lr * self.fn(self.last_step))

    def get_last_lr(self):
        return [self.opt.lr]


def linear_schedule_with_warmup(opt, num_warmup_steps, num_training_steps):
    """transformers.get_linear_schedule_with_warmup semantics."""
    def fn(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))
    return LambdaLR(opt, fn)


def cosine_schedule(opt, total_steps, warmup=0):
    def fn(step):
        if step < warmup:
            return step / max(1, warmup)
        return 0.5 * (1 + math.cos(math.pi * min(1.0, (step - warmup) / max(1, total_steps - warmup))))
    return LambdaLR(opt, fn)


# ------------------------------------------------------------------------------ standard groupings
def _trainable(params):
    return [p for p in params if p.requires_grad]


def no_decay_1d(model, weight_decay: float):
    """Groups of the standard "no weight decay on 1-D parameters" recipe: trainable parameters with
    ``ndim <= 1`` (biases, BatchNorm / LayerNorm gains and shifts) at decay 0, the rest at
    ``weight_decay`` (HF's ``no_decay = ["bias", "LayerNorm.weight"]``; the ResNet SGD recipes)."""
    ps = _trainable(model.parameters())
    return [{"params": [p for p in ps if p.ndim > 1], "weight_decay": float(weight_decay)},
            {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0}]


def head_module(model):
    """The replaced head of a transfer-learning model: ``ResNet.fc`` (a Linear or an ``MLPHead``),
    ``VGG.classifier[-1]``, ``KerasResNet50TL.dense``, BERT's ``classifier``.  ``ValueError`` for a
    model without a distinguishable head (BiLSTM, a bare MLP)."""
    from .models.bert import BertForSequenceClassification
    from .models.keras_resnet import KerasResNet50TL
    from .models.resnet import ResNet
    from .models.vgg import VGG
    if isinstance(model, ResNet):
        head = model.fc
    elif isinstance(model, VGG):
        head = model.classifier[-1]
    elif isinstance(model, KerasResNet50TL):
        head = model.dense
    elif isinstance(model, BertForSequenceClassification):
        head = model.classifier
    else:
        raise ValueError(f"{type(model).__name__} has no distinguishable head")
    if not any(True for _ in head.parameters()):
        raise ValueError(f"{type(model).__name__}: the head has no parameters")
    return head


def backbone_head_groups(model, backbone_lr_mult: float):
    """Discriminative fine-tuning: every trainable parameter outside :func:`head_module` at
    ``lr_mult = backbone_lr_mult``, the head at 1.  ``ValueError`` when nothing outside the head is
    trainable (a frozen backbone: the multiplier would do nothing)."""
    head = {id(p) for p in head_module(model).parameters()}
    ps = _trainable(model.parameters())
    backbone = [p for p in ps if id(p) not in head]
    if not backbone:
        raise ValueError(f"{type(model).__name__}: no trainable parameter outside the head (frozen backbone)")
    return [{"params": backbone, "lr_mult": float(backbone_lr_mult)},
            {"params": [p for p in ps if id(p) in head], "lr_mult": 1.0}]


def compose_groups(*groupings):
    """Intersect groupings: a parameter takes every setting its group gives it in each grouping (a later
    grouping wins a setting both give); parameters with the same settings form one group.
    ``compose_groups(no_decay_1d(m, wd), backbone_head_groups(m, r))`` has up to four groups."""
    settings, order = {}, []
    for grouping in groupings:
        seen = set()
        for grp in grouping:
            kv = {k: v for k, v in grp.items() if k != "params"}
            for p in grp["params"]:
                if id(p) in seen:
                    raise ValueError(f"compose_groups: a parameter of shape {tuple(p.shape)} is listed twice")
                seen.add(id(p))
                if id(p) not in settings:
                    settings[id(p)] = {}
                    order.append(p)
                settings[id(p)].update(kv)
    out = {}
    for p in order:
        key = tuple(sorted(settings[id(p)].items()))
        out.setdefault(key, {"params": [], **settings[id(p)]})["params"].append(p)
    return [g for g in out.values() if g["params"]]


def build(name: str, flat: FlatParams, **kw):
    name = name.lower()
    if name == "sgd":
        return SGD(flat, **kw)
    if name == "adam":
        return Adam(flat, **kw)
    if name == "adamw":
        return AdamW(flat, **kw)
    raise ValueError(name)
