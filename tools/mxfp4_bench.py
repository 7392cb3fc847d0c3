"""Times of the mxfp4 inference matmul mode (``--infer-matmul mxfp4``: MXFP4 weights, MXFP8 activations) against the
bf16 and mxfp8 paths of the same build, for docs/PERF_NOTES.md.

Per shape (those of the mxfp8 table): the GEMM alone and activation quantiser + GEMM, bf16 ``conv_fwd`` next to them;
for the two M = 1 shapes the achieved weight bytes/s of the skinny GEMMs, computed from the shapes.  Then the FFN1 ->
FFN2 pair with ``out_mx``, the BERT-base evaluation forward at B = 32, S = 128, and VGG16 / ResNet-50 batch-1 p50
through ``Batch1Predictor``.  Device events around windows of back-to-back launches after warm-up, the variants
alternated within every round, median (min .. max).

Usage: python tools/mxfp4_bench.py [--rounds 5] [--iters 30] [--skip-shapes] [--skip-e2e] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.ops import _lib  # noqa: E402

SHAPES = [(4096, 768, 2304), (4096, 768, 3072), (4096, 3072, 768), (1, 25088, 4096), (1, 2048, 1000)]   # (M, K, N)
MODES = ("bf16", "mxfp8", "mxfp4")


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def fmt(v, spec="7.1f"):
    return f"{statistics.median(v):{spec}} ({min(v):{spec[1:]}} .. {max(v):{spec[1:]}})"


def alternate(variants, rounds, run, warm):
    """{name: [run(fn) per round]}, the order reversed every other round."""
    for fn in variants.values():
        warm(fn)
    times = {k: [] for k in variants}
    for r in range(rounds):
        for k in (list(variants) if r % 2 == 0 else reversed(list(variants))):
            times[k].append(run(variants[k]))
    return times


def shape_variants(M, K, N, dev):
    o = _lib.ops()
    g = torch.Generator(device=dev).manual_seed(M + K + N)
    x = torch.randn(M, K, device=dev, generator=g).bfloat16()
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    b = torch.zeros(N, device=dev)
    x4, w4 = x.view(M, 1, 1, K), w.bfloat16().view(N, 1, 1, K)
    xq, ex = o.mxfp8_quant(x)
    wq8, ew8 = o.mxfp8_quant(w)
    wq4, ew4 = o.mxfp4_quant(w)
    return {
        "bf16 conv_fwd": lambda: o.conv_fwd(x4, w4, 1, 0, b, None, False, False),
        "mxfp8 quant x": lambda: o.mxfp8_quant(x),
        "mxfp8 GEMM": lambda: o.linear_mxfp8_fwd(xq, ex, wq8, ew8, b, 0, False),
        "mxfp4 GEMM": lambda: o.linear_mxfp4_fwd(xq, ex, wq4, ew4, b, 0, False),
        "mxfp8 quant + GEMM": lambda: o.linear_mxfp8_fwd(*o.mxfp8_quant(x), wq8, ew8, b, 0, False),
        "mxfp4 quant + GEMM": lambda: o.linear_mxfp4_fwd(*o.mxfp8_quant(x), wq4, ew4, b, 0, False),
        "mxfp4 quant W fp32 (cached)": lambda: o.mxfp4_quant(w),
    }


def ffn_variants(dev, M=4096, H=768, F=3072):
    o = _lib.ops()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(M, H, device=dev, generator=g).bfloat16()
    w1, w2 = torch.randn(F, H, device=dev, generator=g) * 0.02, torch.randn(H, F, device=dev, generator=g) * 0.02
    b1, b2 = torch.zeros(F, device=dev), torch.zeros(H, device=dev)
    x4, w1b, w2b = x.view(M, 1, 1, H), w1.bfloat16().view(F, 1, 1, H), w2.bfloat16().view(H, 1, 1, F)
    q8, q4 = (o.mxfp8_quant(w1), o.mxfp8_quant(w2)), (o.mxfp4_quant(w1), o.mxfp4_quant(w2))

    def pair(fwd, q, chain):
        if chain:
            return lambda: fwd(*fwd(*o.mxfp8_quant(x), *q[0], b1, 2, True), *q[1], b2, 0, False)
        return lambda: fwd(*o.mxfp8_quant(fwd(*o.mxfp8_quant(x), *q[0], b1, 2, False)[0]), *q[1], b2, 0, False)

    return {
        "bf16 (GEMM, GELU, GEMM)": lambda: o.conv_fwd(o.gelu_fwd(o.conv_fwd(x4, w1b, 1, 0, b1, None, False, False)[0]).view(M, 1, 1, F),
                                                       w2b, 1, 0, b2, None, False, False),
        "mxfp8 without out_mx": pair(o.linear_mxfp8_fwd, q8, False), "mxfp8 with out_mx": pair(o.linear_mxfp8_fwd, q8, True),
        "mxfp4 without out_mx": pair(o.linear_mxfp4_fwd, q4, False), "mxfp4 with out_mx": pair(o.linear_mxfp4_fwd, q4, True),
    }


def in_mode(mode, fn):
    def run():
        _lib.set_infer_matmul(mode)
        try:
            with torch.no_grad():
                return fn()
        finally:
            _lib.set_infer_matmul("bf16")
    return run


def host_window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bert_eval(dev, rounds, out):
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(7)
    model = BertForSequenceClassification(BertConfig()).to(dev).eval()
    ids = torch.randint(1, 30522, (32, 128), generator=torch.Generator().manual_seed(7)).to(dev)
    v = {m: in_mode(m, lambda: model.forward_logits(ids)) for m in MODES}
    times = alternate(v, rounds, lambda fn: 32 / host_window(fn, 10), lambda fn: host_window(fn, 3))
    print(f"BERT-base evaluation forward, B = 32, S = 128: samples/s over {rounds} rounds of 10 forwards", file=out)
    z = {m: v[m]().float() for m in MODES}
    for m in MODES:
        print(f"  {m:6s} {fmt(times[m], '8.0f')}   max |logit - bf16 logit| {float((z[m] - z['bf16']).abs().max()):.4f}"
              f" (largest |bf16 logit| {float(z['bf16'].abs().max()):.3f})", file=out)


def batch1(dev, rounds, out):
    from pcmp.engine.inference import Batch1Predictor
    from pcmp.models.resnet import resnet50
    from pcmp.models.vgg import vgg16
    imgs = torch.rand(50, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(dev)
    for name, ctor in (("VGG16", vgg16), ("ResNet-50", resnet50)):
        torch.manual_seed(11)
        model = ctor().to(dev).eval()
        preds, p50 = {}, {}

        def make(mode):
            pred = in_mode(mode, lambda: Batch1Predictor(model, imgs[:1]))()   # the graph captures the mode's kernels

            def run():
                lat = []
                for i in range(len(imgs)):
                    t0 = time.perf_counter()
                    preds.setdefault(mode, {})[i] = pred(imgs[i:i + 1])
                    lat.append(time.perf_counter() - t0)
                return statistics.median(lat) * 1e3
            return run
        v = {m: make(m) for m in MODES}
        p50 = alternate(v, rounds, lambda fn: fn(), lambda fn: fn())
        print(f"{name} batch-1 p50 through Batch1Predictor, 50 images: ms over {rounds} rounds", file=out)
        for m in MODES:
            same = sum(preds[m][i] == preds["bf16"][i] for i in range(len(imgs)))
            print(f"  {m:6s} {fmt(p50[m], '7.3f')}   top-1 equal to bf16 on {same} of {len(imgs)} random-weight images", file=out)
        del model, v
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    for M, K, N in ([] if args.skip_shapes else SHAPES):
        v = shape_variants(M, K, N, dev)
        times = alternate(v, args.rounds, lambda fn: window(fn, args.iters), lambda fn: window(fn, 5))
        print(f"shape (M, K, N) = ({M}, {K}, {N}): us per call, median (min .. max) over {args.rounds} rounds of {args.iters}", file=out)
        for k, t in times.items():
            print(f"  {k:30s} {fmt(t)}", file=out)
        if M == 1:   # the skinny GEMMs are weight streams: element bytes plus one scale byte per 32 elements
            for k, wbytes in (("mxfp8 GEMM", N * K + N * K // 32), ("mxfp4 GEMM", N * K // 2 + N * K // 32)):
                print(f"  {k}: {wbytes / 1e6:.1f} MB of weights and scales, {wbytes / statistics.median(times[k]) / 1e6:.2f} TB/s", file=out)
        out.flush()
        del v
        torch.cuda.empty_cache()
    times = alternate(ffn_variants(dev), args.rounds, lambda fn: window(fn, args.iters), lambda fn: window(fn, 5))
    print("FFN1 -> FFN2 pair, 4096 rows, 768 -> 3072 -> 768, GELU, per-call quantisers included: us", file=out)
    for k, t in times.items():
        print(f"  {k:30s} {fmt(t)}", file=out)
    out.flush()
    if not args.skip_e2e:
        bert_eval(dev, args.rounds, out)
        out.flush()
        batch1(dev, args.rounds, out)
        out.flush()


if __name__ == "__main__":
    main()
