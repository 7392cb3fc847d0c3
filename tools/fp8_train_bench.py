"""Times of the fp8 training matmul mode (``--train-matmul fp8``) against the bf16 kernels, for docs/PERF_NOTES.md.

Per shape (BERT-base's four Linear shapes at M = 4096 tokens): the quantisers alone, each fp8 GEMM alone, and
quantise + GEMM against the bf16 ``conv_fwd`` / ``conv_dgrad`` / ``conv_wgrad`` calls of ``LinearFn``; device events
around windows of back-to-back launches, the variants alternated within every round, median (min .. max) in us.
Whole step: the BERT-base fine-tune step (B = 32, S = 128, AdamW on the flat arena) with the mode off and on,
alternated, and the loss after a fixed number of steps under both modes from one seed.

Usage: python tools/fp8_train_bench.py [--rounds 5] [--iters 30] [--steps 10] [--loss-steps 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp import optim  # noqa: E402
from pcmp.ops import _lib, cross_entropy  # noqa: E402
from pcmp.utils.flat import FlatParams  # noqa: E402

SHAPES = [(4096, 768, 2304), (4096, 768, 768), (4096, 768, 3072), (4096, 3072, 768)]   # (M, K, N)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def fmt(v):
    return f"{statistics.median(v):7.1f} ({min(v):.1f} .. {max(v):.1f})"


def shape_variants(M, K, N, dev):
    o = _lib.ops()
    g = torch.Generator(device=dev).manual_seed(M + K + N)
    x = torch.randn(M, K, device=dev, generator=g).bfloat16()
    dy = torch.randn(M, N, device=dev, generator=g).bfloat16()
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    b = torch.zeros(N, device=dev)
    wb = w.bfloat16()
    x4, dy4, w4 = x.view(M, 1, 1, K), dy.view(M, 1, 1, N), wb.view(N, 1, 1, K)
    xq, sx = o.fp8_quant_rows(x, 0)
    wq, sw = o.fp8_quant_rows(w, 0)
    wtq, swt = o.fp8_quant_cols(w, 0)
    dyq, sdy, dytq, sn = o.fp8_quant_both(dy, 1)
    xtq, sk = o.fp8_quant_cols(x, 0)
    gw = torch.empty(N, K, device=dev)

    def fp8_bwd():
        q = o.fp8_quant_both(dy, 1)
        t = o.fp8_quant_cols(x, 0)
        o.linear_fp8_dgrad(q[0], q[1], wtq, swt)
        o.linear_fp8_wgrad(q[2], q[3], t[0], t[1], gw, False)

    return {
        "quant_rows x (E4M3)": lambda: o.fp8_quant_rows(x, 0),
        "quant_cols x (E4M3)": lambda: o.fp8_quant_cols(x, 0),
        "quant_rows dy (E5M2)": lambda: o.fp8_quant_rows(dy, 1),
        "quant_cols dy (E5M2)": lambda: o.fp8_quant_cols(dy, 1),
        "quant_both dy (E5M2)": lambda: o.fp8_quant_both(dy, 1),
        "quant_cols W fp32 (cached)": lambda: o.fp8_quant_cols(w, 0),
        "fp8 fwd GEMM": lambda: o.linear_fp8_fwd(xq, sx, wq, sw, b, 0),
        "fp8 dgrad GEMM": lambda: o.linear_fp8_dgrad(dyq, sdy, wtq, swt),
        "fp8 wgrad GEMM": lambda: o.linear_fp8_wgrad(dytq, sn, xtq, sk, gw, False),
        "bf16 conv_fwd": lambda: o.conv_fwd(x4, w4, 1, 0, b, None, False, False),
        "bf16 conv_dgrad": lambda: o.conv_dgrad(dy4, w4, 1, 1, 1, 0, None, None),
        "bf16 conv_wgrad": lambda: o.conv_wgrad(dy4, x4, gw, 1, 1, 1, 0, False),
        "fp8 quant + fwd": lambda: o.linear_fp8_fwd(*o.fp8_quant_rows(x, 0), wq, sw, b, 0),
        "fp8 backward (2 quant + 2 GEMM)": fp8_bwd,
        "bf16 backward (dgrad + wgrad)": lambda: (o.conv_dgrad(dy4, w4, 1, 1, 1, 0, None, None),
                                                  o.conv_wgrad(dy4, x4, gw, 1, 1, 1, 0, False)),
    }


def bert_step(dev, seed):
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(seed)
    model = BertForSequenceClassification(BertConfig()).to(dev).train()
    flat = FlatParams(list(model.parameters()))
    opt = optim.build("adamw", flat, lr=2e-5, weight_decay=0.01)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 30522, (32, 128), generator=g).to(dev)
    labels = torch.randint(0, 2, (32,), generator=g).to(dev)

    def step():
        opt.zero_grad()
        loss = cross_entropy(model.forward_logits(ids), labels)
        loss.backward()
        opt.step()
        return loss.detach()

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--loss-steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    for M, K, N in SHAPES:
        v = shape_variants(M, K, N, dev)
        times = {k: [] for k in v}
        for fn in v.values():
            window(fn, 5)
        for r in range(args.rounds):
            for k in (list(v) if r % 2 == 0 else reversed(list(v))):
                times[k].append(window(v[k], args.iters))
        print(f"shape (M, K, N) = ({M}, {K}, {N}): us per call, median (min .. max) over {args.rounds} rounds of {args.iters}", file=out)
        for k, t in times.items():
            print(f"  {k:34s} {fmt(t)}", file=out)
        out.flush()
        del v
        torch.cuda.empty_cache()
    # whole step: two models from one seed, the mode switched around each window
    steps = {m: bert_step(dev, 7) for m in ("bf16", "fp8")}
    times = {m: [] for m in steps}
    losses = {m: [] for m in steps}

    def run(mode, n):
        _lib.set_train_matmul(mode)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ls = [steps[mode]() for _ in range(n)]
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            losses[mode].extend(float(l) for l in ls)
            return dt * 1e3
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
