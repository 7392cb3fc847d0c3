"""The bits of the flat optimizer ops as data: a sha256 of every output buffer of ``sgd_flat``,
``adam_flat``, ``sgd_flat_groups`` and ``adam_flat_groups`` over a fixed list of cases
(tests/test_optim_flat_bits_gpu.py recomputes every digest and compares).  The recorded file is the
anchor of a change that must not move a bit of the optimizer arithmetic: record it before the change,
replay it after.

Inputs come from a seeded CPU ``torch.Generator`` and are moved to the device.  Sizes: the arenas of
``pcmp.ops.truth_optim_groups`` (``edge``, ``r300``, ``wrap``: the grid of 2048 workgroups wraps) and,
for the ungrouped ops, 16 elements and 2048*256*4 + 1200 (the grid wraps and the tail is ragged).  The
small sizes (``n16``, ``edge``) take the whole product of the settings; ``r300`` and the ``edge``
sub-ranges take every optimizer variant at gscale 0.5 with the shadow; the three 2 M-element sizes take
a handful of cases that still reach every variant, so that hashing stays at a few seconds.

    python tools/optim_flat_bits.py [--out tests/data/optim_flat_bits_mi355x.txt]
"""
import argparse
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "data", "optim_flat_bits_mi355x.txt")
LR, WD = 0.05, 0.01
BETAS, EPS = (0.9, 0.999), 1e-8
# (tag, momentum, dampening, nesterov)
SGD_VARIANTS = [("nesterov", 0.9, 0.0, True), ("damp0.1", 0.9, 0.1, False), ("mom0", 0.0, 0.0, False)]
ADAM_STEPS = (1.0, 3.0, 10000.0)
BIG = 2048 * 256 * 4 + 1200


def _G():
    from pcmp.ops import truth_optim_groups
    return truth_optim_groups


def sizes():
    """name -> elements: the ungrouped ops run over all of them, the grouped ops over the arenas."""
    G = _G()
    return {"n16": 16, "edge": G.layout("edge")[1], "r300": G.layout("r300")[1], "wrap": G.layout("wrap")[1],
            "big": BIG}


_inputs = {}


def inputs(name, dev):
    """fp32 w, g, m1, m2 (positive) and a uint8 mask with about half the elements off, made once per
    size on the CPU from a seed of their own and never written."""
    import torch
    if (name, str(dev)) not in _inputs:
        n = sizes()[name]
        gen = torch.Generator().manual_seed(4200 + sorted(sizes()).index(name))
        w, g, m1 = (torch.randn(n, generator=gen) for _ in range(3))
        m2 = torch.rand(n, generator=gen) * 0.01 + 1e-4
        mask = (torch.rand(n, generator=gen) < 0.5).to(torch.uint8)
        _inputs[name, str(dev)] = tuple(t.to(dev) for t in (w, g, m1 * 0.1, m2, mask))
    return _inputs[name, str(dev)]


def _settings(name, sub_range=False):
    """(gscale, shadow) pairs of a size."""
    if name in ("n16", "edge") and not sub_range:
        return list(itertools.product((None, 0.5), (True, False)))
    return [(0.5, True)]


def _large(name):
    return name in ("wrap", "big")


def sgd_cases(name, grouped, sub_range=False):
    """(tag, variant, first_step, gscale, shadow, masked)"""
    if _large(name):
        picks = [(0, True, False), (0, False, True), (1, False, False), (2, False, False)]
    else:
        picks = [(v, f, m) for v in range(3) for f in (True, False) for m in (False, True)]
    for v, first, masked in picks:
        if masked and grouped:
            continue
        for gs, shadow in _settings(name, sub_range):
            tag = (f"{SGD_VARIANTS[v][0]}/first{int(first)}/gs{gs}/sh{int(shadow)}"
                   + ("" if grouped else f"/mask{int(masked)}"))
            yield tag, SGD_VARIANTS[v], first, gs, shadow, masked


def adam_cases(name, grouped, sub_range=False):
    """(tag, decoupled, step, gscale, shadow, masked)"""
    if _large(name):
        picks = [(False, 3.0, False), (True, 1.0, True), (True, 10000.0, False)]
    else:
        picks = [(d, s, m) for d in (False, True) for s in ADAM_STEPS for m in (False, True)]
    for decoupled, step, masked in picks:
        if masked and grouped:
            continue
        for gs, shadow in _settings(name, sub_range):
            tag = (f"{'adamw' if decoupled else 'adam'}/step{int(step)}/gs{gs}/sh{int(shadow)}"
                   + ("" if grouped else f"/mask{int(masked)}"))
            yield tag, decoupled, step, gs, shadow, masked


def _table(name, dev):
    import torch
    G = _G()
    runs = G.runs(name)
    return (torch.tensor([e for _, e, _ in runs], dtype=torch.int64, device=dev),
            torch.tensor([G.GROUP_SETTINGS[g][0] for _, _, g in runs], dtype=torch.float32, device=dev),
            torch.tensor([G.GROUP_SETTINGS[g][1] for _, _, g in runs], dtype=torch.float32, device=dev))


def run_cases(dev, op):
    """Runs every case of ``op``; yields (case, {buffer: tensor}) with the whole buffers, so what lies
    outside a sub-range is part of the digest."""
    import torch
    ops, G = torch.ops.pcmp, _G()
    grouped = op.endswith("_groups")
    lr = torch.tensor([LR], device=dev)
    for name, total in sizes().items():
        if grouped and name not in G.ARENAS:
            continue
        w0, g, m10, m20, mask = inputs(name, dev)
        table = _table(name, dev) if grouped else None
        ranges = [(0, total)] + (G.EDGE_SLICES if grouped and name == "edge" else [])
        for lo, hi in ranges:
            where = f"{op}/{name}" + (f"[{lo}:{hi}]" if (lo, hi) != (0, total) else "")
            cases = (sgd_cases if op.startswith("sgd") else adam_cases)(name, grouped, (lo, hi) != (0, total))
            for tag, variant, third, gs, shadow, masked in cases:
                gst = torch.tensor([gs], device=dev) if gs is not None else None
                sh = torch.full((total,), 7.0, dtype=torch.bfloat16, device=dev) if shadow else None
                shs = sh[lo:hi] if shadow else None
                mk = mask if masked else None
                w = w0.clone()
                if op.startswith("sgd"):
                    _, momentum, dampening, nesterov = variant
                    mom = m10.clone() if momentum else w0.new_empty(0)
                    moms = mom[lo:hi] if momentum else mom
                    if grouped:
                        ops.sgd_flat_groups(w[lo:hi], g[lo:hi], moms, shs, lr, gst, *table, lo, total, momentum,
                                            dampening, nesterov, third)
                    else:
                        ops.sgd_flat(w, g, moms, shs, mk, lr, gst, momentum, dampening, WD, nesterov, third)
                    out = {"w": w, **({"mom": mom} if momentum else {})}
                else:
                    m1, m2, st = m10.clone(), m20.clone(), torch.tensor([third], device=dev)
                    if grouped:
                        ops.adam_flat_groups(w[lo:hi], g[lo:hi], m1[lo:hi], m2[lo:hi], shs, lr, gst, st, *table, lo,
                                             total, *BETAS, EPS, variant)
                    else:
                        ops.adam_flat(w, g, m1, m2, shs, mk, lr, gst, st, *BETAS, EPS, WD, variant)
                    out = {"w": w, "m1": m1, "m2": m2}
                if shadow:
                    out["shadow"] = sh
                yield f"{where}/{tag}", out


OPS = ("sgd_flat", "adam_flat", "sgd_flat_groups", "adam_flat_groups")


def sha256(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def digests(dev, op):
    """(case, buffer, sha256 of the buffer's bytes) of every case of ``op``."""
    for case, out in run_cases(dev, op):
        for k, v in out.items():
            yield case, k, sha256(v)


def read(path=PATH):
    """{(case, buffer): sha256} of a recorded file."""
    table = {}
    with open(path) as f:
        for line in f.read().splitlines():
            if line and not line.startswith("#"):
                case, buf, h = line.split()
                assert (case, buf) not in table, line
                table[case, buf] = h
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    import torch
    import pcmp  # noqa: F401
    from pcmp.ops import _lib
    assert torch.cuda.is_available(), "the digests are those of the GPU kernels"
    assert _lib.load(), _lib.load_error()
    dev = torch.device("cuda", 0)
    lines = ["# tools/optim_flat_bits.py: <op>/<size>[<sub-range>]/<settings> <buffer> <sha256 of its bytes>"]
    for op in OPS:
        n = len(lines)
        lines += [" ".join(d) for d in digests(dev, op)]
        print(f"{op}: {len(lines) - n} digests", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
