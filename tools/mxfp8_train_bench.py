"""Times of the mxfp8 training matmul mode (``--train-matmul mxfp8``) against the fp8 mode and the bf16 kernels, for
docs/PERF_NOTES.md.  The protocol of tools/fp8_train_bench.py: one process, device events around windows of
back-to-back launches, the variants alternated within every round, median (min .. max) in us.

Per shape (BERT-base's four Linear shapes at M = 4096 tokens): the two-way quantiser, each block-scaled GEMM alone
(WGRAD also under every forced split count of ``--splits``), and the whole forward / backward of one Linear in the
three modes.  Whole step: the BERT-base fine-tune step (B = 32, S = 128, AdamW on the flat arena) under bf16 / fp8 /
mxfp8, interleaved, and the losses from one seed.

Usage: python tools/mxfp8_train_bench.py [--rounds 5] [--iters 30] [--steps 10] [--loss-steps 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp8_train_bench import SHAPES, bert_step, fmt, window  # noqa: E402

import torch  # noqa: E402

from pcmp.ops import _lib  # noqa: E402


def shape_variants(M, K, N, dev, splits):
    o = _lib.ops()
    g = torch.Generator(device=dev).manual_seed(M + K + N)
    x = torch.randn(M, K, device=dev, generator=g).bfloat16()
    dy = torch.randn(M, N, device=dev, generator=g).bfloat16()
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    b = torch.zeros(N, device=dev)
    x4, dy4, w4 = x.view(M, 1, 1, K), dy.view(M, 1, 1, N), w.bfloat16().view(N, 1, 1, K)
    xq, ex, xtq, ext = o.mxfp8_quant_both(x)
    wq, ew, wtq, ewt = o.mxfp8_quant_both(w)
    dyq, edy, dytq, edyt = o.mxfp8_quant_both(dy)
    fq, fs = o.fp8_quant_rows(w, 0)
    ftq, fts = o.fp8_quant_cols(w, 0)
    gw = torch.empty(N, K, device=dev)

    def wgrad_ns(ns):
        def run():
            old = o.set_knob("mxfp8_wgrad_ns", ns)
            o.linear_mxfp8_wgrad(dytq, edyt, xtq, ext, gw, False)
            o.set_knob("mxfp8_wgrad_ns", old)
        return run

    def mx_bwd():
        q = o.mxfp8_quant_both(dy)
        o.linear_mxfp8_fwd(q[0], q[1], wtq, ewt, None, 0, False)
        o.linear_mxfp8_wgrad(q[2], q[3], xtq, ext, gw, False)

    def fp8_bwd():
        q = o.fp8_quant_both(dy, 1)
        t = o.fp8_quant_cols(x, 0)
        o.linear_fp8_dgrad(q[0], q[1], ftq, fts)
        o.linear_fp8_wgrad(q[2], q[3], t[0], t[1], gw, False)

    v = {
        "mxfp8_quant (rows only) x": lambda: o.mxfp8_quant(x),
        "mxfp8_quant_both x": lambda: o.mxfp8_quant_both(x),
        "mxfp8_quant_both dy": lambda: o.mxfp8_quant_both(dy),
        "fp8_quant_both dy (E5M2)": lambda: o.fp8_quant_both(dy, 1),
        "mxfp8_quant_both W fp32 (cached)": lambda: o.mxfp8_quant_both(w),
        "mxfp8 fwd GEMM": lambda: o.linear_mxfp8_fwd(xq, ex, wq, ew, b, 0, False),
        "mxfp8 dgrad GEMM": lambda: o.linear_mxfp8_fwd(dyq, edy, wtq, ewt, None, 0, False),
        "mxfp8 wgrad GEMM (rule)": lambda: o.linear_mxfp8_wgrad(dytq, edyt, xtq, ext, gw, False),
    }
    for ns in splits:
        v[f"mxfp8 wgrad GEMM, {ns} split(s)"] = wgrad_ns(ns)
    v.update({
        "bf16 conv_fwd": lambda: o.conv_fwd(x4, w4, 1, 0, b, None, False, False),
        "fp8 quant + fwd": lambda: o.linear_fp8_fwd(*o.fp8_quant_rows(x, 0), fq, fs, b, 0),
        "mxfp8 quant_both + fwd": lambda: o.linear_mxfp8_fwd(*o.mxfp8_quant_both(x)[:2], wq, ew, b, 0, False),
        "bf16 backward (dgrad + wgrad)": lambda: (o.conv_dgrad(dy4, w4, 1, 1, 1, 0, None, None),
                                                  o.conv_wgrad(dy4, x4, gw, 1, 1, 1, 0, False)),
        "fp8 backward (2 quant + 2 GEMM)": fp8_bwd,
        "mxfp8 backward (1 quant + 2 GEMM)": mx_bwd,
    })
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--loss-steps", type=int, default=30)
    ap.add_argument("--splits", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("M", "K", "N"),
                    help="time this shape (repeatable) instead of BERT-base's four, and skip the whole step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    for M, K, N in args.shape or SHAPES:
        v = shape_variants(M, K, N, dev, args.splits)
        times = {k: [] for k in v}
        for fn in v.values():
            window(fn, 5)
        for r in range(args.rounds):
            for k in (list(v) if r % 2 == 0 else reversed(list(v))):
                times[k].append(window(v[k], args.iters))
        print(f"shape (M, K, N) = ({M}, {K}, {N}): us per call, median (min .. max) over {args.rounds} rounds of {args.iters}", file=out)
        for k, t in times.items():
            print(f"  {k:36s} {fmt(t)}", file=out)
        out.flush()
        del v
        torch.cuda.empty_cache()
    if args.shape:
        return
    # whole step: one model per mode from one seed, the mode switched around each window
    steps = {m: bert_step(dev, 7) for m in ("bf16", "fp8", "mxfp8")}
    times = {m: [] for m in steps}
    losses = {m: [] for m in steps}

    def run(mode, n):
        _lib.set_train_matmul(mode)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ls = [steps[mode]() for _ in range(n)]
            torch.cuda.synchronize()
            losses[mode].extend(float(l) for l in ls)
            return (time.perf_counter() - t0) / n * 1e3
        finally:
            _lib.set_train_matmul("bf16")

    for m in steps:
        run(m, 3)
    for r in range(args.rounds):
        for m in (list(steps) if r % 2 == 0 else reversed(list(steps))):
            times[m].append(run(m, args.steps))
    done = 3 + args.rounds * args.steps
    for m in steps:
        if done < args.loss_steps:
            run(m, args.loss_steps - done)
    print(f"BERT-base fine-tune step, B = 32, S = 128, AdamW: ms per step over {args.rounds} rounds of {args.steps} steps", file=out)
    for m, t in times.items():
        print(f"  train-matmul {m:5s} {statistics.median(t):7.2f} ({min(t):.2f} .. {max(t):.2f})   {32e3 / statistics.median(t):7.0f} samples/s", file=out)
    for m, l in losses.items():
        print(f"  train-matmul {m:5s} loss at steps 1, 10, 20, {len(l)}: {l[0]:.4f} {l[9]:.4f} {l[19]:.4f} {l[-1]:.4f}", file=out)
    out.flush()


if __name__ == "__main__":
    main()
