"""Device time of the bf16 (or fp32) attention ops at a constant 4,096 tokens (H = 12, head dim 64):
(B, S) = (32, 128), (16, 256), (8, 512), p = 0 and p = 0.1, next to
torch.nn.functional.scaled_dot_product_attention forward + backward (p = 0, same key mask) in the
same process order.  5 x 50 calls between HIP events after warm-up (the protocol docs/PARITY.md
quotes for attention_bwd); one JSON line per measurement with the median and the range of the five
per-call means, in microseconds.

    python tools/attn_bench.py              # every shape, default dispatch
    python tools/attn_bench.py --tiled 1    # S = 128 only, through the tiled kernels (knob attn_tiled)
    python tools/attn_bench.py --dtype fp32                  # fp32 inputs, default dispatch (S = 512: tiled)
    python tools/attn_bench.py --dtype fp32 --f32-tiled 1    # S = 128 and 256 through the tiled fp32 kernels

An A/B run alternates whole processes, each under its own time limit, chained so that a failure
ends the run:

    timeout -k 10 120 python tools/attn_bench.py --tag r1 && timeout -k 10 60 python tools/attn_bench.py --tiled 1 --tag r1 && ...

Raw lines of the recorded runs: profiles/attn_long_ab.txt (bf16), profiles/attn_f32_long_ab.txt (fp32);
the tables: docs/PERF_NOTES.md.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.ops import _lib  # noqa: E402

SHAPES = [(32, 128), (16, 256), (8, 512)]
H = 12
REPS, CALLS = 5, 50


def timed(fn):
    """[median, min, max] of REPS means over CALLS back-to-back calls, us per call."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    out.sort()
    return [round(out[REPS // 2], 2), round(out[0], 2), round(out[-1], 2)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tiled", type=int, default=0, choices=[0, 1], help="knob attn_tiled; 1 times S = 128 only")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="input dtype of the ops and of SDPA")
    ap.add_argument("--f32-tiled", type=int, default=0, choices=[0, 1],
                    help="knob attn_f32_tiled (with --dtype fp32); 1 times S = 128 and 256 only")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    fp32 = args.dtype == "fp32"
    if (args.f32_tiled and not fp32) or (args.tiled and fp32):
        ap.error("--tiled goes with --dtype bf16, --f32-tiled with --dtype fp32")
    assert torch.cuda.is_available(), "attn_bench needs a GPU"
    assert _lib.load(), _lib.load_error()
    ops = torch.ops.pcmp
    dev = torch.device("cuda", 0)
    ops.set_knob("attn_tiled", args.tiled)
    ops.set_knob("attn_f32_tiled", args.f32_tiled)
    dt = torch.float32 if fp32 else torch.bfloat16
    knob_on = args.f32_tiled if fp32 else args.tiled
    shapes = SHAPES[:2] if args.f32_tiled else SHAPES[:1] if args.tiled else SHAPES
    gen = torch.Generator(device=dev).manual_seed(0)
    for B, S in shapes:
        qkv = (torch.randn(B * S, 3 * H * 64, device=dev, generator=gen) * 0.5).to(dt)
        ids = torch.randint(1, 30522, (B, S), device=dev, generator=gen)
        for i in range(B):
            ids[i, S - (37 * i) % (S // 2):] = 0
        rec = {"tag": args.tag, "attn_tiled": args.tiled, "B": B, "S": S, "H": H}
        if fp32:
            rec = {"tag": args.tag, "dtype": "fp32", "attn_f32_tiled": args.f32_tiled, "B": B, "S": S, "H": H}
        for p in (0.0, 0.1):
            ctx, lse = ops.attention_fwd(qkv, ids, B, S, H, p, 7, 0)
            dctx = torch.randn(B * S, H * 64, device=dev, generator=gen).to(dt)
            tf = timed(lambda: ops.attention_fwd(qkv, ids, B, S, H, p, 7, 0))
            tb = timed(lambda: ops.attention_bwd(dctx, qkv, ctx, lse, ids, B, S, H, p, 7, 0))
            print(json.dumps(dict(rec, op="pcmp", p=p, fwd_us=tf, bwd_us=tb)), flush=True)
        if knob_on:
            continue
        # the yardstick: torch SDPA on [B, H, S, 64] views of the same values, boolean key mask
        t = qkv.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4).contiguous()
        q, k, v = (t[i].clone().requires_grad_(True) for i in range(3))
        mask = (ids > 0).view(B, 1, 1, S)
        do = dctx.view(B, S, H, 64).transpose(1, 2).contiguous()

        def fb():
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
            q.grad = k.grad = v.grad = None
            o.backward(do)

        with torch.no_grad():
            tf = timed(lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask))
        tfb = timed(fb)
        print(json.dumps(dict(rec, op="sdpa", p=0.0, fwd_us=tf, fwd_bwd_us=tfb)), flush=True)


if __name__ == "__main__":
    main()
