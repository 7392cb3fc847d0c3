"""Times of the mxfp8 inference attention mode (``--infer-attn mxfp8``) against the unchained mxfp8 layer of the same
build, for docs/PERF_NOTES.md.

Per call at (B, S) = (32, 128) and (8, 512), H = 12: bf16 ``attention_fwd`` on the bf16 QKV matrix against
``attention_mx_fwd`` on its block-scaled pair (context as bf16 and as a pair), and ``layernorm_fwd`` without and with
``out_mx`` against the ``mxfp8_quant`` launch it replaces.  Then the BERT-base evaluation forward with ``--infer-matmul
mxfp8``, attention mode off against on, at both shapes, with the largest logit deviation from the bf16 forward (12
layers, random weights).  One process, device events around windows of back-to-back launches after warm-up, the variants
alternated within every round, median (min .. max).

Usage: python tools/mx_attn_bench.py [--rounds 5] [--iters 50] [--layers 12] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.models.bert import BertConfig, BertForSequenceClassification  # noqa: E402
from pcmp.ops import _lib  # noqa: E402

SHAPES = ((32, 128), (8, 512))


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


def batch_ids(B, S, dev):
    ids = torch.randint(1, 30522, (B, S), generator=torch.Generator().manual_seed(S))
    for b in range(B):                      # valid lengths S, S - 7, S - 14, ...: a padded evaluation batch
        if b % 8:
            ids[b, S - 7 * (b % 8):] = 0
    return ids.to(dev)


def op_variants(B, S, dev):
    o, H, D = _lib.ops(), 12, 768
    g = torch.Generator(device=dev).manual_seed(B + S)
    qkv = torch.randn(B * S, 3 * D, device=dev, generator=g).bfloat16()
    x, r = (torch.randn(B * S, D, device=dev, generator=g).bfloat16() for _ in range(2))
    gam, bet = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    q, e = o.mxfp8_quant(qkv)
    ids = batch_ids(B, S, dev)
    return {"attention_fwd bf16": lambda: o.attention_fwd(qkv, ids, B, S, H, 0.0, 0, 0),
            "attention_mx_fwd -> bf16": lambda: o.attention_mx_fwd(q, e, ids, B, S, H, False),
            "attention_mx_fwd -> pair": lambda: o.attention_mx_fwd(q, e, ids, B, S, H, True),
            "layernorm_fwd": lambda: o.layernorm_fwd(x, r, gam, bet, 1e-12),
            "layernorm_fwd out_mx": lambda: o.layernorm_fwd(x, r, gam, bet, 1e-12, 0.0, 0, 0, None, True),
            "mxfp8_quant [B*S, 768]": lambda: o.mxfp8_quant(x)}


def in_modes(matmul, attn, fn):
    def run():
        _lib.set_infer_matmul(matmul)
        _lib.set_infer_attn(attn)
        try:
            with torch.no_grad():
                return fn()
        finally:
            _lib.set_infer_matmul("bf16")
            _lib.set_infer_attn("bf16")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    for B, S in SHAPES:
        t = alternate(op_variants(B, S, dev), args.rounds, lambda fn: window(fn, args.iters), lambda fn: window(fn, 3))
        print(f"ops at B = {B}, S = {S}, H = 12: us per call, median (min .. max) over {args.rounds} rounds of {args.iters}", file=out)
        for k, v in t.items():
            print(f"  {k:26s} {fmt(v)}", file=out)
        out.flush()
    torch.manual_seed(11)
    model = BertForSequenceClassification(BertConfig(num_hidden_layers=args.layers)).to(dev).eval()
    for B, S in SHAPES:
        ids = batch_ids(B, S, dev)
        v = {"bf16": in_modes("bf16", "bf16", lambda: model(ids)[0]), "mxfp8, attn off": in_modes("mxfp8", "bf16", lambda: model(ids)[0]),
             "mxfp8, attn on": in_modes("mxfp8", "mxfp8", lambda: model(ids)[0])}
        t = alternate(v, args.rounds, lambda fn: window(fn, 10) / 1e3, lambda fn: window(fn, 2))
        z = {k: fn().float() for k, fn in v.items()}
        print(f"BERT-base evaluation forward, {args.layers} layers, B = {B}, S = {S}: ms over {args.rounds} rounds of 10 forwards", file=out)
        for k in v:
            print(f"  {k:16s} {fmt(t[k], '8.3f')}   {B / statistics.median(t[k]):7.2f} k samples/s   max |logit - bf16 logit| "
                  f"{float((z[k] - z['bf16']).abs().max()):.4f}", file=out)
        out.flush()


if __name__ == "__main__":
    main()
