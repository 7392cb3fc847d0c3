"""fp64 truths, cases and runners of the loss head every model ends in, in both dtypes: ``softmax_xent``,
``loss_mean``, ``xent_grad_scale``, ``log_softmax_bwd`` (csrc/elementwise.hip) and the bf16 ``colsum``
(the fp32 one is with the fp32 image path, ``ops/truth_image_f32.py``).  As in ``ops/truth.py`` every
truth is plain fp64 torch on the values the inputs hold as given (bf16 logits are rounded first), the
backward by ``torch.autograd`` of ``log_softmax``; tests/test_loss_truth_cpu.py runs ``ops/ref.py``
through the runners here, tests/test_loss_truth_gpu.py ``torch.ops.pcmp``.

What is judged:

* ``loss_rows`` and ``logp`` are fp32 outputs in both dtypes: ``seg_rel`` (``loss_rows`` as one segment,
  ``logp`` per row).
* ``dlogits = (softmax - onehot) * grad_scale`` is judged *as the softmax it encodes*:
  ``dlogits / grad_scale + onehot`` against the truth's softmax, per row (``seg_rel`` in fp32, ``norm_err``
  in bf16).  ``p - onehot`` itself cancels to ~1e-26 of the row's size on a confidently-right row and
  cannot carry a relative criterion.
* Rows without a valid label (``ignore_index``, a label outside [0, V), ``labels = None``) have
  ``loss_rows == 0`` and ``dlogits == 0`` exactly.
"""
from __future__ import annotations

import functools

import torch

from .truth import norm_err, seg_rel  # noqa: F401  (re-exported)
from .truth_image_run import _cpu, chunks, to  # noqa: F401

F32, BF = torch.float32, torch.bfloat16
IGNORE = -100
XENT_B = [1, 37]
XENT_V = [2, 10, 64, 65, 1000]       # 64 / 65: one element per lane and one lane's second trip
GRAD_SCALES = [1.0, 0.5, 1.0 / 37]
ROW_KINDS = ["wide", "const", "confident", "randn"]
# B = 1 runs one row of each of these kinds with its *least* likely class as the label.  loss = lse - z[y]
# carries the absolute error of lse, half an ulp of max|z| in fp32, whatever the loss's own size; as the
# only row of its segment the loss has to be of lse's size for a relative criterion to apply to it.  The
# confident row (loss ~ 1e-26) is a row among others at B = 37, as the criterion reads there.
ROW_KINDS_B1 = ["wide", "const", "randn"]
LABEL_KINDS = ["mixed", "all_ignored", "none"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _row(kind, V, gen):
    if kind == "wide":          # exp() over 160 units of range
        return torch.linspace(-80.0, 80.0, V)
    if kind == "const":
        return torch.full((V,), 1.25)
    r = torch.randn(V, generator=gen) * 3
    if kind == "confident":     # the label is the argmax by a margin of 60: p - onehot cancels
        y = int(torch.randint(0, V, (1,), generator=gen))
        r[y] = r.max() + 60.0
    return r


@functools.lru_cache(maxsize=None)
def xent_case(B, V, dtype, kind0="wide"):
    """logits [B, V] in ``dtype`` and the three label vectors.  B = 37: row 0 wide-range, 1 constant, 2
    confident, the others 3 * randn; labels random, row 2's its argmax, row 5 ignore_index, row 6 a label
    >= V, row 7 a negative label other than ignore_index.  B = 1: the one row is of kind ``kind0`` with a
    valid label, the row's argmin (ROW_KINDS_B1)."""
    gen = _gen(1000 * B + V + (7 if dtype == BF else 0) + ROW_KINDS.index(kind0))
    kinds = [kind0] if B == 1 else ROW_KINDS[:3] + ["randn"] * (B - 3)
    z = torch.stack([_row(k, V, gen) for k in kinds]).to(dtype)
    lab = torch.randint(0, V, (B,), generator=gen)
    for i, k in enumerate(kinds):
        if k == "confident":
            lab[i] = int(z[i].float().argmax())
    if B > 7:
        lab[5], lab[6], lab[7] = IGNORE, V + 3, -5
    if B == 1:
        lab[0] = int(z[0].float().argmin())
    return dict(z=z, labels={"mixed": lab, "all_ignored": torch.full((B,), IGNORE, dtype=torch.long), "none": None})


def xent_truth(z, labels):
    """fp64: logp, softmax p, valid [B] (bool), onehot [B, V], loss_rows (0 at invalid rows) and, by
    autograd of log_softmax, d(sum of the valid rows' losses) / d(logits) = (p - onehot) at valid rows."""
    B, V = z.shape
    z64 = z.detach().double().requires_grad_(True)
    logp = torch.log_softmax(z64, dim=1)
    if labels is None:
        valid, lab = torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.long)
    else:
        valid = (labels != IGNORE) & (labels >= 0) & (labels < V)
        lab = torch.where(valid, labels, torch.zeros_like(labels))
    onehot = torch.zeros(B, V, dtype=torch.float64)
    onehot[torch.arange(B), lab] = valid.double()
    loss = -(logp * onehot).sum(1)
    dz = torch.autograd.grad(loss.sum(), z64)[0] if bool(valid.any()) else torch.zeros(B, V, dtype=torch.float64)
    return dict(logp=logp.detach(), p=torch.softmax(z64.detach(), dim=1), valid=valid, onehot=onehot,
                loss_rows=loss.detach(), dz=dz)


def run_xent(impl, B, V, dtype, gs, label_kind, want_logp, want_grad, dev="cpu", kind0="wide"):
    """Returns (res, zero, raw): ``res`` {output: (got, truth, seg_dims)} -- "loss_rows", "logp", "p" (the
    softmax recovered from dlogits at the valid rows) --, ``zero`` the tensors that must be exactly 0 (the
    invalid rows of loss_rows and dlogits), ``raw`` the implementation's outputs."""
    c = xent_case(B, V, dtype, kind0)
    labels = c["labels"][label_kind]
    t = xent_truth(c["z"], labels)
    z, lab = to(dev, c["z"], labels)
    out = impl.softmax_xent(z, lab, want_logp, want_grad, gs, IGNORE)
    assert len(out) == 1 + int(want_logp) + int(want_grad)
    v = t["valid"]
    lr = _cpu(out[0])
    assert lr.dtype == F32 and tuple(lr.shape) == (B,)
    res, zero = {"loss_rows": (lr, t["loss_rows"], (0,))}, [lr[~v]]
    if want_logp:
        lp = _cpu(out[1])
        assert lp.dtype == F32
        res["logp"] = (lp, t["logp"], (1,))
    if want_grad:
        dl = _cpu(out[-1])
        assert dl.dtype == dtype
        zero.append(dl[~v])
        got, oh = dl[v].double() / gs + t["onehot"][v], t["onehot"][v]
        if dtype == F32:
            res["p"] = (got, t["p"][v], (1,))
        else:
            # bf16 stores (p_y - 1) * grad_scale at the label: 2^-9 of ~1, which says nothing about a small p_y.
            # The other classes are judged as the softmax they encode (the label's entry set to the truth's);
            # the label's entry as what it stores: the bf16 rounding (twice 2^-9, relative) of a p_y - 1 whose
            # p_y meets the fp32 criterion 1e-5 (absolute: p <= 1)
            res["p"] = (torch.where(oh > 0, t["p"][v], got), t["p"][v], (1,))
            el, tl = (got - oh)[oh > 0], (t["p"][v] - oh)[oh > 0]
            assert bool(((el - tl).abs() <= 2.0 ** -8 * tl.abs() + 1e-5).all()), "the label's entry of dlogits"
        # the truth's own gradient encodes the same softmax (autograd and softmax agree)
        assert float((t["dz"][v] + t["onehot"][v] - t["p"][v]).abs().max() if v.any() else 0.0) < 1e-14
    return res, zero, list(out)


# ------------------------------------------------------------------------------ loss_mean / grad scale
LOSS_MEAN_B = [1, 255, 256, 257, 1000]      # both sides of the 256-thread loop
GRAD_SCALE_N = [1, 255, 256 * 37 + 3]
LSM_BWD_SHAPES = [(B, V) for B in (1, 37) for V in (2, 65, 1000)]
COLSUM_SHAPES = [(M, C) for M in (1, 17, 300) for C in (8, 520)]   # 520: a second, one-vector column block


@functools.lru_cache(maxsize=None)
def loss_mean_case(B, all_ignored=False):
    """Per-row losses as softmax_xent leaves them (0 at invalid rows) and labels for V = 10 with ignored,
    too-large and negative ones among them."""
    gen = _gen(B)
    V = 10
    lab = torch.randint(0, V, (B,), generator=gen)
    if all_ignored:
        lab = torch.full((B,), IGNORE, dtype=torch.long)
    elif B > 1:
        k = torch.rand(B, generator=gen)
        lab = torch.where(k < 0.1, torch.full_like(lab, IGNORE), lab)
        lab = torch.where((k >= 0.1) & (k < 0.15), torch.full_like(lab, V + 1), lab)
        lab = torch.where((k >= 0.15) & (k < 0.2), torch.full_like(lab, -3), lab)
        lab[0] = 3      # at least one valid row
    valid = (lab != IGNORE) & (lab >= 0) & (lab < V)
    rows = torch.where(valid, torch.rand(B, generator=gen) * 4 + 0.01, torch.zeros(B))
    return dict(rows=rows, labels=lab, V=V, valid=valid)


def run_loss_mean(impl, B, all_ignored=False, dev="cpu"):
    """(res, valid count got, valid count truth, raw)."""
    c = loss_mean_case(B, all_ignored)
    out = impl.loss_mean(c["rows"].to(dev), c["labels"].to(dev), c["V"], IGNORE)
    o = _cpu(out)
    assert o.dtype == F32 and tuple(o.shape) == (2,)
    n = int(c["valid"].sum())
    t = c["rows"].double().sum() / max(n, 1)
    return {"mean": (o[:1], t.reshape(1), (0,))}, float(o[1]), float(n), [out]


@functools.lru_cache(maxsize=None)
def grad_scale_case(n, dtype):
    gen = _gen(n + (5 if dtype == BF else 0))
    return dict(dl=torch.randn(n, generator=gen).to(dtype), gout=torch.tensor([0.75]))


def run_grad_scale(impl, n, dtype, valid, dev="cpu"):
    """xent_grad_scale: dl * gout / max(1, valid)."""
    c = grad_scale_case(n, dtype)
    out = impl.xent_grad_scale(c["dl"].to(dev), c["gout"].to(dev), torch.tensor([float(valid)], device=dev))
    assert out.dtype == dtype
    t = c["dl"].double() * (c["gout"].double()[0] / max(float(valid), 1.0))
    return {"out": (_cpu(out), t, (0,))}, [out]


@functools.lru_cache(maxsize=None)
def lsm_bwd_case(B, V, dtype, grid=False):
    """z = 3 * randn, g a random upstream gradient; ``grid`` (fp32): g on multiples of 1/8 with every row
    summing to exactly zero, so that dz = g - exp(logp) * 0 must be g bitwise.  At V = 2 the two elements
    of a row of g get opposite signs: dz0 = -dz1 = g0 * p1 - g1 * p0 cancels where the two products meet,
    and by chance one row in 37 then loses a factor of 100 of fp32's precision against its own norm, in any
    implementation of g - p * sum(g)."""
    gen = _gen(100 * B + V + (3 if dtype == BF else 0) + (11 if grid else 0))
    z = torch.randn(B, V, generator=gen) * 3
    if grid:
        g = torch.randint(-16, 17, (B, V), generator=gen).float() / 8
        g[:, -1] = -g[:, :-1].sum(1)
        assert float(g.double().sum(1).abs().max()) == 0.0
    else:
        g = torch.randn(B, V, generator=gen)
        if V == 2:
            g[:, 1] = -g[:, 1].abs() * torch.sign(g[:, 0])
    return dict(z=z, g=g.to(dtype))


def run_lsm_bwd(impl, B, V, dtype, dev="cpu", grid=False):
    """log_softmax_bwd on the fp32 logp of the fp64 log_softmax (what the forward saves): dz against the
    autograd gradient of log_softmax for the upstream g, per row."""
    c = lsm_bwd_case(B, V, dtype, grid)
    z64 = c["z"].double().requires_grad_(True)
    logp = torch.log_softmax(z64, dim=1)
    t = torch.autograd.grad((logp * c["g"].double()).sum(), z64)[0]
    dz = impl.log_softmax_bwd(c["g"].to(dev), logp.detach().float().to(dev))
    assert dz.dtype == dtype
    return {"dz": (_cpu(dz), t, (1,))}, [dz], c["g"]


@functools.lru_cache(maxsize=None)
def colsum_case(M, C):
    gen = _gen(1000 * M + C + 1)
    return dict(x=(torch.randn(M, C, generator=gen) + 0.25).to(BF), out0=torch.randn(C, generator=gen))


def run_colsum(impl, M, C, dev="cpu"):
    """The bf16 colsum written into a NaN-filled vector and accumulated onto a non-zero one."""
    d = colsum_case(M, C)
    x = d["x"].to(dev)
    out = torch.full((C,), float("nan"), device=dev)
    impl.colsum(x, out, False)
    acc = d["out0"].clone().to(dev)
    impl.colsum(x, acc, True)
    t = d["x"].double().sum(0)
    return {"sum": (_cpu(out), t, (0,)), "sum_acc": (_cpu(acc), t + d["out0"].double(), (0,))}, [out, acc]


# ------------------------------------------------------------------------------ comparators
def worst(res, fn):
    return {n: max([float(fn(a, t, s).max()) for a, t, s in chunks(v) if a.numel()], default=0.0) for n, v in res.items()}


def check(bounds, op, res, what=""):
    """bounds[(op, output)] = (floor, bound, criterion): ``seg_rel < bound`` or ``norm_err <= bound``; the
    figures are printed first."""
    for n, v in res.items():
        _, bound, crit = bounds[(op, n)]
        w = worst({n: v}, seg_rel if crit == "seg_rel" else norm_err)[n]
        print(crit, op, n, what, float("%.3g" % w))
        assert (w < bound) if crit == "seg_rel" else (w <= bound), f"{op} {n} {what}: {crit} {w:.3g} against {bound:g}"


def xent_variants(B):
    """(kind0, grad_scale, label kind, want_logp, want_grad) of one (B, V, dtype): every row kind at B = 1,
    every grad_scale, label kind and output combination."""
    out = []
    for k0 in (ROW_KINDS_B1 if B == 1 else ROW_KINDS[:1]):
        for gs in GRAD_SCALES:
            out.append((k0, gs, "mixed", True, True))
        out += [(k0, 0.5, lk, wl, wg) for lk in LABEL_KINDS for wl in (True, False) for wg in (True, False)
                if not (lk == "mixed" and wl and wg)]
    return out


def xent_op(dtype):
    return "softmax_xent" if dtype == F32 else "softmax_xent_bf16"
