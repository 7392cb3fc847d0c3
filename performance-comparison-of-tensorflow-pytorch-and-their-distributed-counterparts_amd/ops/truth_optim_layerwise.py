"""fp64 truths and cases of the layer-wise optimizers (``lars_flat`` / ``lamb_flat``, csrc/optim_layerwise.hip).

Nothing here mirrors the kernels' roundings.  LAMB is a plain per-parameter fp64 loop of the formulas
(You et al. 2020, bias-corrected, decay inside the update); LARS is ``torch.optim.SGD`` on fp64
parameters with ``weight_decay=0``, fed ``r_p * (g' + wd_p * w)`` computed in fp64.  Three steps under
``LambdaLR`` factors (1, 0.5, 0.25) with the group settings of ``truth_optim_groups``.  The comparator is
``norm_err`` with one segment per parameter (padding included).

Arenas in terms of the kernels' chunk size C (sizes in elements; a slice is the size rounded up to 16):
  edge   1 | 15 | 16 | 17 | C-16 (1-D) | C | C+16 | 2C+1 over groups 0 1 2 0 0 1 2 0: a one-vector segment,
         padding inside a segment, exactly one chunk, a one-vector tail chunk, three chunks with a short last;
  many   300 parameters of 16 elements: more segments than a workgroup has threads;
  long   257*C + 16 | 48: more partials than ``trust_ratio`` has threads, then a segment whose slots must
         start in the right place.
``degenerate`` (on edge): the 17-element parameter's weights are zeros and the C-element parameter (group 1,
decay 0) has a zero gradient in every step.

The ratio bound.  A sum of squares has only positive terms, so every fp32 add contributes at most one
relative rounding u = 2^-24: C / 256 fused adds per thread, 6 adds of the wave's shuffle tree and 3 over the
four waves; the fp64 sum of the partials, the two square roots, the division and the rounding of the
ratio to fp32 are covered by 2 u.  The two norms share the ratio, each contributing half of its sum's
error.  What is summed also differs from the truth: after up to three steps an element of w, g' or u has
been through at most 32 fp32 roundings of the update (products, the moment blends, a division, a square
root, the bias corrections) and a norm's relative error is at most its elements', twice for a ratio of two
norms: 64 u.  RATIO_RTOL = (C / 256 + 9 + 2 + 64) u.
"""
from __future__ import annotations

import functools

import torch

from ..optim import CHUNK as C
from .truth import assert_elementwise, norm_err
from .truth_optim_groups import GROUP_SETTINGS, LR, LR_FACTORS

BF = torch.bfloat16
ARENAS = {
    "edge": dict(sizes=[1, 15, 16, 17, C - 16, C, C + 16, 2 * C + 1], group=[0, 1, 2, 0, 0, 1, 2, 0], one_d=[4]),
    "many": dict(sizes=[16] * 300, group=[i % 3 for i in range(300)], one_d=[]),
    "long": dict(sizes=[257 * C + 16, 48], group=[0, 1], one_d=[]),
}
ZERO_W, ZERO_G, ONE_D = 3, 5, 4          # parameters of the degenerate edge case
KW = {"lamb": dict(betas=(0.9, 0.999), eps=1e-6), "lars": dict(momentum=0.9, nesterov=True, trust_coef=0.001, eps=1e-8)}
BOUNDS = {"w": 0.01, "mom": 0.01, "m1": 0.01, "m2": 0.01, "shadow": 1.0}      # k of docs/PARITY.md
RATIO_RTOL = (C // 256 + 9 + 2 + 64) * 2.0 ** -24


def layout(name):
    """(offsets, arena size): 16-element aligned slices in order."""
    offs, off = [], 0
    for n in ARENAS[name]["sizes"]:
        offs.append(off)
        off += (n + 15) // 16 * 16
    return offs, off


@functools.lru_cache(maxsize=None)
def case(name, degenerate=False):
    """Initial fp32 values and three fp32 gradients per parameter (fixed seed per arena)."""
    gen = torch.Generator().manual_seed(2000 + sorted(ARENAS).index(name))
    sizes = ARENAS[name]["sizes"]
    c = dict(w=[torch.randn(n, generator=gen) for n in sizes],
             grads=[[torch.randn(n, generator=gen) for n in sizes] for _ in LR_FACTORS])
    if degenerate:
        c["w"][ZERO_W].zero_()
        for grads in c["grads"]:
            grads[ZERO_G].zero_()
    return c


def to_arena(name, tensors):
    offs, total = layout(name)
    out = torch.zeros(total, dtype=torch.float64)
    for o, t in zip(offs, tensors):
        out[o:o + t.numel()] = t.detach().double().reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def truth_steps(kind, name, gscale=None, degenerate=False, adapt_1d=False):
    """Per step the arena-shaped fp64 w and state tensors and the fp64 ``ratio`` per parameter."""
    c, a, kw = case(name, degenerate), ARENAS[name], KW[kind]
    gs = 1.0 if gscale is None else float(gscale)
    mult, wd = zip(*(GROUP_SETTINGS[g] for g in a["group"]))
    adapt = [adapt_1d or i not in a["one_d"] for i in range(len(mult))]
    ws = [torch.nn.Parameter(w.double().clone()) for w in c["w"]]
    if kind == "lars":
        sgd = torch.optim.SGD([{"params": [p], "lr": LR * m} for p, m in zip(ws, mult)], lr=LR, weight_decay=0.0,
                              momentum=kw["momentum"], nesterov=kw["nesterov"])
        sched = torch.optim.lr_scheduler.LambdaLR(sgd, lambda i: LR_FACTORS[min(i, len(LR_FACTORS) - 1)])
    m1, m2 = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
    out = []
    for t, grads in enumerate(c["grads"], 1):
        ratio = []
        for i, (w, g) in enumerate(zip(ws, grads)):
            g, wn = g.double() * gs, float(w.detach().norm())
            if kind == "lars":
                gn = float(g.norm())
                r = kw["trust_coef"] * wn / (gn + wd[i] * wn + kw["eps"]) if adapt[i] and wn > 0 and gn > 0 else 1.0
                w.grad = r * (g + wd[i] * w.detach())
            else:
                (b1, b2), eps = kw["betas"], kw["eps"]
                m1[i] = b1 * m1[i] + (1 - b1) * g
                m2[i] = b2 * m2[i] + (1 - b2) * g * g
                u = (m1[i] / (1 - b1 ** t)) / ((m2[i] / (1 - b2 ** t)).sqrt() + eps) + wd[i] * w.detach()
                un = float(u.norm())
                r = wn / un if adapt[i] and wn > 0 and un > 0 else 1.0
                w.data -= LR * LR_FACTORS[t - 1] * mult[i] * r * u
            ratio.append(r)
        if kind == "lars":
            sgd.step()
            sched.step()
            st = {"w": ws, "mom": [sgd.state[p]["momentum_buffer"] for p in ws]}
        else:
            st = {"w": ws, "m1": m1, "m2": m2}
        out.append({**{k: to_arena(name, v) for k, v in st.items()}, "ratio": torch.tensor(ratio, dtype=torch.float64)})
    return out


def build_opt(optim_mod, kind, name, device="cpu", degenerate=False, adapt_1d=False):
    """(flat, params, opt): the arena over plain nn.Parameters (2-D, the ``one_d`` ones 1-D) and the optimizer
    with groups 1 and 2 listed and group 0 left to the default group."""
    from ..utils.flat import FlatParams
    a = ARENAS[name]
    params = [torch.nn.Parameter((w if i in a["one_d"] else w.view(1, -1)).clone().to(device))
              for i, w in enumerate(case(name, degenerate)["w"])]
    flat = FlatParams(params, shadow_dtype=BF, reverse=False)
    groups = [{"params": [p for p, g in zip(params, a["group"]) if g == gi], "lr_mult": m, "weight_decay": wd}
              for gi, (m, wd) in enumerate(GROUP_SETTINGS) if gi > 0 and gi in a["group"]]
    opt = optim_mod.build(kind, flat, lr=LR, weight_decay=GROUP_SETTINGS[0][1], groups=groups, adapt_1d=adapt_1d,
                          **KW[kind])
    return flat, params, opt


def run_steps(optim_mod, kind, name, device="cpu", gscale=None, degenerate=False, adapt_1d=False, partition=None):
    """Three steps of the pcmp optimizer under ``pcmp.optim.LambdaLR`` -- ``step()``, or ``begin_step`` /
    ``step_range`` over ``partition`` / ``end_step`` -- and per step CPU copies of w, state, shadow, ratio."""
    flat, params, opt = build_opt(optim_mod, kind, name, device, degenerate, adapt_1d)
    sched = optim_mod.LambdaLR(opt, lambda i: LR_FACTORS[min(i, len(LR_FACTORS) - 1)])
    opt.set_grad_scale(gscale)
    out = []
    for grads in case(name, degenerate)["grads"]:
        for p, g in zip(params, grads):
            p.main_grad.copy_(g.view_as(p).to(device))
        if partition is None:
            opt.step()
        else:
            opt.begin_step()
            for lo, hi in partition:
                opt.step_range(lo, hi)
            opt.end_step()
        sched.step()
        st = {"w": flat.master, "shadow": flat.shadow, "ratio": opt.trust_ratio,
              **{k: v for k, v in opt._state().items() if k != "step_t"}}
        out.append({k: v.detach().cpu().clone() for k, v in st.items()})
    return out


def worst(name, got, truth):
    """Worst ``norm_err`` per output over every step and parameter, and the worst relative ratio error."""
    offs, total = layout(name)
    out = {}
    for g, t in zip(got, truth):
        for k, v in g.items():
            if k == "ratio":
                e = float(((v.double() - t[k]).abs() / t[k]).max())
            else:
                tv = t["w" if k == "shadow" else k]
                e = max(float(norm_err(v[a:b], tv[a:b], (0,)).max()) for a, b in zip(offs, offs[1:] + [total]))
            out[k] = max(out.get(k, 0.0), e)
    return out


def check(name, got, truth, what=""):
    """w, state and shadow within ``BOUNDS`` per parameter, the ratios within ``RATIO_RTOL`` and exactly 1.0
    where the truth's is, the padding exact zeros; the worst figures are printed first."""
    print("layerwise", name, what, {k: float("%.3g" % v) for k, v in worst(name, got, truth).items()})
    offs, total = layout(name)
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, ARENAS[name]["sizes"]):
        pad[o:o + n] = False
    for step, (g, t) in enumerate(zip(got, truth)):
        for k, v in g.items():
            if k == "ratio":
                one = t[k] == 1.0
                assert torch.equal(v[one], torch.ones_like(v[one])), f"{what} step {step}: ratio exactly 1"
                rel = (v.double() - t[k]).abs() / t[k]
                assert float(rel.max()) <= RATIO_RTOL, f"{what} step {step}: ratio off by {float(rel.max()):.3g}"
                continue
            assert int((v[pad] != 0).sum()) == 0, f"{what} {k}: padding stays exact zeros"
            tv = t["w" if k == "shadow" else k]
            for a, b in zip(offs, offs[1:] + [total]):
                assert_elementwise(v[a:b], tv[a:b], (0,), BOUNDS[k], f"{what} {k} step {step} [{a}, {b})")
