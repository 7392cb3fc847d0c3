"""Write the table of ``torch.ops.pcmp.conv_kernel_choice`` over the production conv shapes
(tests/data/conv_kernel_choice.txt, checked by tests/test_conv_choice_cpu.py): one line per entry,
``knobset mode N H W C K R stride pad flags tag``.  Host code only, no GPU needed.

Shapes: every distinct conv_fwd geometry of one CPU training step of resnet50 and resnet18 (traced
with PCMP_TRACE_OPS at batch 2), each at N = 256, 64 and 1; BERT-base's Linear shapes (traced from
a two-layer model) as 1x1 convs over M = 4096 and 16384 rows.  Knob sets: the defaults, and the
static set gemm_plan = 0, wgrad_wgs = 1024, under which "plan/auto" and "/nsauto" resolve to kernels
and split counts.  Flags: the operand combinations the training and inference steps use, restricted
to the geometries that take them (see fwd_flags / dgrad_flags / wgrad_flags).

To record another build's choices (a behaviour-preserving change is checked against its parent):
    PCMP_LIB=/path/to/libpcmp_hip.so python tools/conv_choice_table.py tests/data/conv_kernel_choice.txt
"""
import os
import sys

os.environ["PCMP_TRACE_OPS"] = "1"   # before pcmp.ops.kernels is imported
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.ops import _lib, cross_entropy, kernels, truth_image as T, truth_image_run as R  # noqa: E402

KNOBSETS = {"default": {}, "static": {"gemm_plan": 0, "wgrad_wgs": 1024}}
BATCHES = (256, 64, 1)
BERT_ROWS = (4096, 16384)


def _traced_fwd(step):
    """Distinct (H, W, C, K, R, stride, pad) of the conv_fwd calls of ``step()``, in call order."""
    del kernels.TRACE[:]
    step()
    seen = []
    for name, a in kernels.TRACE:
        if name in ("conv_fwd", "linear_gelu_fwd"):
            x, w = a[0], a[1]
            if len(x) == 2:    # linear_gelu_fwd: x [M, C], w [N, C]
                g = (1, 1, x[1], w[0], 1, 1, 0)
            else:
                g = (x[1], x[2], x[3], w[0], w[1], a[2], a[3])
            if g not in seen:
                seen.append(g)
    return seen


def resnet_shapes():
    from pcmp.models.resnet import resnet18, resnet50
    out = []
    for ctor in (resnet50, resnet18):
        torch.manual_seed(0)
        m = ctor().train()
        x, y = torch.rand(2, 3, 224, 224), torch.randint(0, 1000, (2,))
        out += [g for g in _traced_fwd(lambda: cross_entropy(m.forward_logits(x), y).backward()) if g not in out]
    return out


def bert_shapes():
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(0)
    m = BertForSequenceClassification(BertConfig(num_hidden_layers=2)).train()
    ids, y = torch.randint(1, 1000, (2, 16)), torch.randint(0, 2, (2,))
    del kernels.TRACE[:]
    m(ids, None, None, y)[0].backward()
    # the encoder's Linear layers (its forward is two fused ops: their weight gradients name them): dy
    # [M, 1, 1, N], x [M, 1, 1, C] over the M = 32 token rows; the pooler and the classifier see one row per sequence
    seen = []
    for name, a in kernels.TRACE:
        if name == "conv_wgrad" and a[0][0] == ids.numel():
            g = (1, 1, a[1][3], a[0][3], 1, 1, 0)
            if g not in seen:
                seen.append(g)
    return seen


def fwd_flags(g):
    H, W, C, K, R, s, p = g
    fl = [0, 1, 8, 2 | 4 | 8, 4 | 8]
    if R == 1 and s == 1 and C % 64 == 0:
        fl.append(1 | 16)
    return fl


def dgrad_flags(g):
    H, W, C, K, R, s, p = g
    fl = [0, 4]
    if R == 1 and s == 2:   # conv_dgrad_bnr refuses the uncovered pixel classes
        return fl
    for f in T.BNR_FORMS.values():
        w = f["flags"]
        if (w & 64) and not (R == 1 and s == 1 and K % 64 == 0):
            continue
        if (w & 128) and s != 1:
            continue
        fl.append(w)
    return fl


def wgrad_flags(g):
    H, W, C, K, R, s, p = g
    if not (R == 1 and s == 1):
        return [0]
    return [0, 1, 2, 3] if K > 64 else [0, 1]


def entries(ops, shapes):
    """[(knobset, mode, N, H, W, C, K, R, stride, pad, flags, tag)]"""
    out = []
    for ks, kn in KNOBSETS.items():
        with R.knobs(ops, kn):
            for N, g in shapes:
                for mode, flags in ((0, fwd_flags(g)), (1, dgrad_flags(g)), (2, wgrad_flags(g))):
                    for fl in flags:
                        out.append((ks, mode, N, *g, fl, ops.conv_kernel_choice(mode, N, *g, fl)))
    return out


def main():
    path = sys.argv[1]
    assert _lib.load(), _lib.load_error()
    shapes = [(N, g) for g in resnet_shapes() for N in BATCHES] + [(M, g) for g in bert_shapes() for M in BERT_ROWS]
    rows = entries(torch.ops.pcmp, shapes)
    with open(path, "w") as f:
        f.write("# knobset mode N H W C K R stride pad flags tag   (tools/conv_choice_table.py)\n")
        for r in rows:
            f.write(" ".join(map(str, r)) + "\n")
    fams = sorted({t.split("/")[0] for r in rows for t in r[-1].split("+")})
    print(f"{len(rows)} entries over {len(shapes)} shapes from {_lib.LIB_PATH}; families: {' '.join(fams)}")


if __name__ == "__main__":
    main()
