"""fp64 truths and cases of the grouped flat optimizers (``sgd_flat_groups`` / ``adam_flat_groups``).

The truth is ``torch.optim.SGD`` / ``Adam`` / ``AdamW`` on fp64 parameters with real ``param_groups``
(``lr = base_lr * lr_mult``, ``weight_decay = wd`` per group), one torch parameter per arena
parameter; the learning rate moves between steps through ``torch.optim.lr_scheduler.LambdaLR``, which
scales every group as ``pcmp.optim.LambdaLR`` does.  Nothing here mirrors the kernels' roundings.
Cases are built on the CPU from fixed seeds.  Comparator and segments are those of the optimizer
cases of ``truth_image``: ``norm_err`` with one segment per state tensor per *run* (a maximal
stretch of adjacent same-group parameters, alignment padding included), so a run updated with a
neighbour's rate or decay cannot hide behind a larger run.

Arenas (sizes in elements, arena order; a slice is the size rounded up to 16):
  edge   1 | 15 | 16 | 17, 4097 | 928 | 1536 | 100 over groups 0 1 2 0 0 1 2 0: runs of one 16-element
         slice, padding inside a run, run boundaries at 16, 32, 48 and 4192 and 6656 (inside a
         workgroup's 1024-element span) and at 5120 (exactly on one);
  r300   300 parameters of 16 elements over groups 0 1 2 0 1 2 ...: 300 runs, more than the 256
         threads that stage the table;
  wrap   2048*256*4 + 1024 | 3072 over groups 0 1: 2048*256*4 + 4096 elements, the grid of 2048
         workgroups wraps and the second trip of workgroups 1.. lies in another run than the first.
Groups: 0 = (lr_mult 1, decay 0.01), 1 = (lr_mult 0.1, decay 0), 2 = (lr_mult 0, decay 0.02).
"""
from __future__ import annotations

import functools

import torch

from .truth import assert_elementwise, norm_err  # noqa: F401  (re-exported)

BF = torch.bfloat16
LR = 0.05
LR_FACTORS = (1.0, 0.5, 0.25)          # the schedule: lr of step i = LR * LR_FACTORS[i]
GROUP_SETTINGS = [(1.0, 0.01), (0.1, 0.0), (0.0, 0.02)]   # (lr_mult, weight_decay)
WRAP = 2048 * 256 * 4

ARENAS = {
    "edge": dict(sizes=[1, 15, 16, 17, 4097, 928, 1536, 100], group=[0, 1, 2, 0, 0, 1, 2, 0]),
    "r300": dict(sizes=[16] * 300, group=[i % 3 for i in range(300)]),
    "wrap": dict(sizes=[WRAP + 1024, 3072], group=[0, 1]),
}
# [lo, hi) of the edge arena: inside one run at both ends, one vector, the last run only
EDGE_SLICES = [(1000, 3000), (5124, 5128), (6656, 6768)]
SGD_VARIANTS = [dict(momentum=0.9, nesterov=True, dampening=0.0), dict(momentum=0.9, nesterov=False, dampening=0.1),
                dict(momentum=0.0, nesterov=False, dampening=0.0)]
ADAM_KW = dict(betas=(0.9, 0.999), eps=1e-8)


def layout(name):
    """(offsets, arena size) of an arena: 16-element aligned slices in order."""
    offs, off = [], 0
    for n in ARENAS[name]["sizes"]:
        offs.append(off)
        off += (n + 15) // 16 * 16
    return offs, off


def runs(name):
    """[(start, end, group)] of an arena, worked out here and not through FlatParams.runs."""
    offs, total = layout(name)
    grp = ARENAS[name]["group"]
    out = []
    for i, o in enumerate(offs):
        end = offs[i + 1] if i + 1 < len(offs) else total
        if out and out[-1][2] == grp[i]:
            out[-1] = (out[-1][0], end, grp[i])
        else:
            out.append((o, end, grp[i]))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """Initial fp32 values and three fp32 gradients per parameter (fixed seed per arena)."""
    gen = torch.Generator().manual_seed(1000 + sorted(ARENAS).index(name))
    sizes = ARENAS[name]["sizes"]
    return dict(w=[torch.randn(n, generator=gen) for n in sizes],
                grads=[[torch.randn(n, generator=gen) for n in sizes] for _ in LR_FACTORS])


def build_arena(name, device="cpu", shadow=True):
    """(flat, params, groups): a FlatParams over plain nn.Parameters in arena order with the case's
    values, and the ``groups=`` list of the optimizer (group 0 is left to the default group when
    ``weight_decay=GROUP_SETTINGS[0][1]`` is the constructor's)."""
    from ..utils.flat import FlatParams
    c, a = case(name), ARENAS[name]
    params = [torch.nn.Parameter(w.clone().to(device)) for w in c["w"]]
    flat = FlatParams(params, shadow_dtype=BF if shadow else None, reverse=False)
    groups = [{"params": [p for p, g in zip(params, a["group"]) if g == gi], "lr_mult": m, "weight_decay": wd}
              for gi, (m, wd) in enumerate(GROUP_SETTINGS) if gi > 0 and gi in a["group"]]
    return flat, params, groups


def set_grads(flat, params, name, step, device="cpu"):
    for p, g in zip(params, case(name)["grads"][step]):
        p.main_grad.copy_(g.to(device))


def to_arena(name, tensors):
    """Per-parameter tensors scattered into an arena-shaped fp64 tensor (padding zero)."""
    offs, total = layout(name)
    out = torch.zeros(total, dtype=torch.float64)
    for o, t in zip(offs, tensors):
        out[o:o + t.numel()] = t.detach().double().reshape(-1)
    return out


def truth_steps(kind, name, gscale=None, **kw):
    """Three steps of torch.optim on fp64 parameters with param_groups and a LambdaLR schedule; per
    step the arena-shaped fp64 w and state tensors (mom | m1, m2)."""
    c, a = case(name), ARENAS[name]
    ps = [torch.nn.Parameter(w.double().clone()) for w in c["w"]]
    pg = [{"params": [p for p, g in zip(ps, a["group"]) if g == gi], "lr": LR * m, "weight_decay": wd}
          for gi, (m, wd) in enumerate(GROUP_SETTINGS) if gi in a["group"]]
    cls = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
    opt = cls(pg, lr=LR, **kw)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda i: LR_FACTORS[min(i, len(LR_FACTORS) - 1)])
    out = []
    for grads in c["grads"]:
        for p, g in zip(ps, grads):
            p.grad = g.double() * (1.0 if gscale is None else float(gscale))
        opt.step()
        sched.step()
        if kind == "sgd":
            st = {"w": ps}
            if kw.get("momentum", 0.0) != 0.0:
                st["mom"] = [opt.state[p]["momentum_buffer"] for p in ps]
        else:
            st = {"w": ps, "m1": [opt.state[p]["exp_avg"] for p in ps], "m2": [opt.state[p]["exp_avg_sq"] for p in ps]}
        out.append({k: to_arena(name, v) for k, v in st.items()})
    return out


def run_steps(optim_mod, kind, name, device="cpu", gscale=None, shadow=True, **kw):
    """Three ``step()``s of the pcmp optimizer with groups under ``pcmp.optim.LambdaLR``; per step the
    arena-shaped copies of w, the state tensors and the shadow (on the CPU)."""
    flat, params, groups = build_arena(name, device, shadow)
    opt = optim_mod.build(kind, flat, lr=LR, weight_decay=GROUP_SETTINGS[0][1], groups=groups, **kw)
    sched = optim_mod.LambdaLR(opt, lambda i: LR_FACTORS[min(i, len(LR_FACTORS) - 1)])
    opt.set_grad_scale(gscale)
    out = []
    for i in range(len(LR_FACTORS)):
        set_grads(flat, params, name, i, device)
        opt.step()
        sched.step()
        st = {"w": flat.master, **{k: v for k, v in opt._state().items() if k != "step_t" and v.numel()}}
        if shadow:
            st["shadow"] = flat.shadow
        out.append({k: v.detach().cpu().clone() for k, v in st.items()})
    return out, opt


def chunks(name, got, truth):
    """(output, got, truth, seg_dims) per state tensor per run, over every step; the shadow is judged
    against the truth of w."""
    for g, t in zip(got, truth):
        for k, v in g.items():
            tv = t["w" if k == "shadow" else k]
            for s, e, _ in runs(name):
                yield k, v[s:e], tv[s:e], (0,)


def worst(name, got, truth):
    out = {}
    for k, a, t, seg in chunks(name, got, truth):
        out[k] = max(out.get(k, 0.0), float(norm_err(a, t, seg).max()))
    return out


def check(bounds, op, name, got, truth, what=""):
    """Every element of every run within ``bounds[(op, output)][1]``; the worst figures are printed
    first so a failing run still reports them."""
    print("norm_err", op, name, what, {k: float("%.3g" % v) for k, v in worst(name, got, truth).items()})
    for k, a, t, seg in chunks(name, got, truth):
        assert_elementwise(a, t, seg, bounds[(op, k)][1], f"{op} {k} {name} {what}")


def padding_mask(name):
    """True at the alignment padding of an arena."""
    offs, total = layout(name)
    m = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, ARENAS[name]["sizes"]):
        m[o:o + n] = False
    return m
