"""Times of VGG16 in the mxfp8 inference conv mode (``--infer-conv mxfp8``: block-scaled convs, the 2x2 max-pool fused
into the conv epilogue) against the bf16 path of the same build, for docs/PERF_NOTES.md.

Per layer (the twelve convs behind layer 0) at B = 1 and B = 64: bf16 ``conv_fwd`` (+ ``maxpool_fwd`` where a pool
follows) against one ``conv_mxfp8_fwd`` that consumes the pair and emits the (pooled) pair.  Then the whole evaluation
forward at both batch sizes, and the batch-1 p50 through ``Batch1Predictor`` in the four combinations of conv and matmul
mode.  Device events around windows of back-to-back launches after warm-up (host clock around the predictor), the
variants alternated within every round, median (min .. max).

Usage: python tools/mxfp8_vgg_bench.py [--rounds 5] [--iters 20] [--skip-layers] [--skip-e2e] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.models.vgg import CFG16, vgg16  # noqa: E402
from pcmp.ops import _lib  # noqa: E402


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def fmt(v, spec="8.1f"):
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


def layers():
    """(H = W of the input, C, Cout, pooled) of VGG16's convs 2 .. 13 at 224 x 224."""
    out, hw, cin = [], 224, 64
    for v, nxt in zip(CFG16[1:], CFG16[2:] + [None]):
        if v == "M":
            hw //= 2
        else:
            out.append((hw, cin, v, nxt == "M"))
            cin = v
    return out


def layer_variants(B, hw, C, Co, pool, dev):
    o = _lib.ops()
    g = torch.Generator(device=dev).manual_seed(hw + C + Co)
    x = torch.relu(torch.randn(B, hw, hw, C, device=dev, generator=g)).bfloat16()
    w = torch.randn(Co, 3, 3, C, device=dev, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.zeros(Co, device=dev)
    wb = w.bfloat16()
    xq, ex = o.mxfp8_quant(x.view(-1, C))
    xq = xq.view(x.shape)
    wq, ew = o.mxfp8_quant(w.view(-1, C))
    wq = wq.view(w.shape)

    def bf16():
        y = o.conv_fwd(x, wb, 1, 1, b, None, True, False)[0]
        return o.maxpool_fwd(y, 2, 2, 0, False)[0] if pool else y

    return {"bf16": bf16, "mxfp8": lambda: o.conv_mxfp8_fwd(xq, ex, wq, ew, 1, 1, b, None, True, False, True, 2 if pool else 0)}


def in_modes(conv, matmul, fn):
    def run():
        _lib.set_infer_conv(conv)
        _lib.set_infer_matmul(matmul)
        try:
            with torch.no_grad():
                return fn()
        finally:
            _lib.set_infer_conv("bf16")
            _lib.set_infer_matmul("bf16")
    return run


def eval_forward(model, dev, rounds, out):
    for B, n in ((1, 20), (64, 3)):
        x = torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        v = {c: in_modes(c, "bf16", lambda: model(x)) for c in ("bf16", "mxfp8")}
        times = alternate(v, rounds, lambda fn: window(fn, n) / 1e3, lambda fn: window(fn, 2))
        z = {c: v[c]().float() for c in v}
        print(f"VGG16 evaluation forward, B = {B}: ms over {rounds} rounds of {n} forwards (bf16 matmul)", file=out)
        for c in v:
            print(f"  conv {c:6s} {fmt(times[c], '8.3f')}   max |logit - bf16 logit| {float((z[c] - z['bf16']).abs().max()):.4f}"
                  f" (bf16 logit range {float(z['bf16'].max() - z['bf16'].min()):.3f})", file=out)
        out.flush()


def batch1(model, dev, rounds, out):
    from pcmp.engine.inference import Batch1Predictor
    imgs = torch.rand(50, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(dev)
    preds = {}

    def make(mode):
        pred = in_modes(*mode, lambda: Batch1Predictor(model, imgs[:1]))()   # the graph captures the modes' kernels

        def run():
            lat = []
            for i in range(len(imgs)):
                t0 = time.perf_counter()
                preds.setdefault(mode, {})[i] = pred(imgs[i:i + 1])
                lat.append(time.perf_counter() - t0)
            return statistics.median(lat) * 1e3
        return run
    modes = [(c, m) for c in ("bf16", "mxfp8") for m in ("bf16", "mxfp8")]
    p50 = alternate({m: make(m) for m in modes}, rounds, lambda fn: fn(), lambda fn: fn())
    print(f"VGG16 batch-1 p50 through Batch1Predictor (hipGraph), 50 images: ms over {rounds} rounds", file=out)
    for m in modes:
        same = sum(preds[m][i] == preds[modes[0]][i] for i in range(len(imgs)))
        print(f"  conv {m[0]:6s} matmul {m[1]:6s} {fmt(p50[m], '7.3f')}   top-1 equal to bf16 / bf16 on {same} of {len(imgs)}"
              " random-weight images", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    for B in ([] if args.skip_layers else (1, 64)):
        print(f"VGG16 convs 2 .. 13 at B = {B}: us per call, median (min .. max) over {args.rounds} rounds of {args.iters};"
              " bf16 = conv_fwd (+ maxpool_fwd), mxfp8 = one conv_mxfp8_fwd, pair in, (pooled) pair out", file=out)
        total = {"bf16": 0.0, "mxfp8": 0.0}
        for hw, C, Co, pool in layers():
            v = layer_variants(B, hw, C, Co, pool, dev)
            t = alternate(v, args.rounds, lambda fn: window(fn, args.iters), lambda fn: window(fn, 3))
            for k in total:
                total[k] += statistics.median(t[k])
            print(f"  {hw:3d} x {hw:<3d} {C:3d} -> {Co:3d}{' + pool' if pool else '       '}  bf16 {fmt(t['bf16'])}   mxfp8 {fmt(t['mxfp8'])}"
                  f"   ratio {statistics.median(t['mxfp8']) / statistics.median(t['bf16']):.2f}", file=out)
            out.flush()
            del v
            torch.cuda.empty_cache()
        print(f"  sum of medians: bf16 {total['bf16']:.1f}, mxfp8 {total['mxfp8']:.1f}", file=out)
    if not args.skip_e2e:
        torch.manual_seed(11)
        model = vgg16().to(dev).eval()
        eval_forward(model, dev, args.rounds, out)
        batch1(model, dev, args.rounds, out)
        out.flush()


if __name__ == "__main__":
    main()
