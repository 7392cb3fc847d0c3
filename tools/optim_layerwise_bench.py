"""Device time of a LAMB / LARS step against the parent's kernels on the model arenas.

LAMB against ungrouped AdamW on the BERT-base arena, LARS against ungrouped SGD momentum 0.9 on the
ResNet-50 arena, the layer-wise optimizers at several chunk sizes.  Device events around windows of
``step()``, interleaved rounds (order reversed every other round), median (min - max) per variant; the
yardstick is the parent's kernel and the margin the spread of its own rounds.

Usage: python tools/optim_layerwise_bench.py [--rounds 7] [--chunks 4096,8192,16384] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp import optim  # noqa: E402
from pcmp.utils.flat import FlatParams  # noqa: E402

BYTES = {"adamw": 30, "lamb": 42, "sgd": 22, "lars": 30}   # per element with the bf16 shadow


def arena(which, dev):
    if which == "bert":
        from pcmp.models.bert import BertConfig, BertForSequenceClassification
        model = BertForSequenceClassification(BertConfig())
    else:
        from pcmp.models.resnet import resnet50
        model = resnet50(1000)
    flat = FlatParams(list(model.to(dev).parameters()))
    flat.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    return flat


def window(opt, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        opt.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--chunks", default="4096,8192,16384")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    for which, base, kind, steps, kw in (("resnet50", "sgd", "lars", 1000, dict(momentum=0.9)),
                                         ("bert", "adamw", "lamb", 300, {})):
        flat = arena(which, dev)
        variants = {f"a {base} (parent kernel)": (optim.build(base, flat, lr=1e-6, weight_decay=0.01, **kw), base)}
        for i, c in enumerate(int(x) for x in args.chunks.split(",")):   # a chunk size may repeat: other buffers
            optim.CHUNK = c
            opt = optim.build(kind, flat, lr=1e-6, weight_decay=0.01, **kw)
            variants[f"{'bcdefghij'[i]} {kind} chunk {c} ({opt.nchunks} chunks)"] = (opt, kind)
        times = {k: [] for k in variants}
        for opt, _ in variants.values():
            window(opt, 20)
        for r in range(args.rounds):
            for k in (list(variants) if r % 2 == 0 else reversed(list(variants))):
                times[k].append(window(variants[k][0], steps))
        print(f"{which}: arena {flat.numel} elements, {len(flat.params)} parameters, {args.rounds} interleaved rounds "
              f"of {steps} steps, us per step", file=out)
        ref = statistics.median(times[next(iter(times))])
        for k, v in times.items():
            med = statistics.median(v)
            print(f"  {k:38s} median {med:8.2f}  min {min(v):8.2f}  max {max(v):8.2f}  x{med / ref:5.3f} of a  "
                  f"{BYTES[variants[k][1]] * flat.numel / med / 1e6:5.2f} TB/s", file=out)
        a = times[next(iter(times))]
        print(f"  spread of (a) over its rounds: {max(a) - min(a):.2f} us; all rounds: "
              f"{ {k: [round(x, 2) for x in v] for k, v in times.items()} }", file=out)
        del variants, flat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
