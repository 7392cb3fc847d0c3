"""Long-sequence fp32 attention (256 < S <= 512, any length) on the CPU: the floors of ``ops/ref.py``
in fp32 against the fp64 truth on ``truth.attn_case_long(S, p, with_ids, 2, torch.float32)`` over
``truth.ATTN_S_F32_LONG``, judged with ``truth.seg_rel`` as tests/test_text_truth_gpu.py::
test_attention_f32 judges the fp32 kernels, and the exact zeros of the one-key sequence.

``F32_LONG_BOUNDS`` holds, per (op, output), the floor measured here (the worst ``seg_rel`` of
``ref.py`` over ATTN_S_F32_LONG x {(p = 0, ids), (p = 0.1, ids), (p = 0, no ids)}) and the bound of
tests/test_attention_f32_long_gpu.py, which is the project's fp32 attention bound: 1e-5 for ctx and
dqkv, 1e-6 for lse.  A bound must stay at least twice the floor.
"""
import pytest  # noqa: F401
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth as T, truth_run as R

F32_LONG_VARIANTS = ((0.0, True), (0.1, True), (0.0, False))

# (op, output): (floor of ops/ref.py on the CPU, bound of the GPU tests)
F32_LONG_BOUNDS = {
    ("attention_p0", "ctx"): (5.3e-7, 1e-5), ("attention_p0", "lse"): (1.6e-7, 1e-6), ("attention_p0", "dqkv"): (5.4e-7, 1e-5),
    ("attention_drop", "ctx"): (5.1e-7, 1e-5), ("attention_drop", "lse"): (7.1e-8, 1e-6),
    ("attention_drop", "dqkv"): (5.3e-7, 1e-5),
}

_RUNS = {}


def ref_run(S, p, with_ids):
    """run_attention of ops/ref.py on one long fp32 case, computed once per session."""
    key = (S, p, with_ids)
    if key not in _RUNS:
        _RUNS[key] = R.run_attention(ref, T.attn_case_long(S, p, with_ids, 2, torch.float32), S, p)
    return _RUNS[key]


def seg_rel_worst(res):
    """Worst seg_rel per output of one run_attention result; every compared tensor must be fp32."""
    out = {}
    for n, v in res.items():
        for a, t, s in R.chunks(v):
            assert a.dtype == torch.float32, (n, a.dtype)
            out[n] = max(out.get(n, 0.0), float(T.seg_rel(a, t, s).max()) if a.numel() else 0.0)
    return out


def measure_floors():
    fl = {}
    for S in T.ATTN_S_F32_LONG:
        for p, with_ids in F32_LONG_VARIANTS:
            for n, e in seg_rel_worst(ref_run(S, p, with_ids)[0]).items():
                key = (R.attn_op(p), n)
                fl[key] = max(fl.get(key, 0.0), e)
    return fl


def test_f32_long_lengths():
    assert T.ATTN_S_F32_LONG == [257, 300, 320, 384, 509, 512]
    for S in T.ATTN_S_F32_LONG:
        qkv, ids, dctx, B, lens = T.attn_case_long(S, 0.0, True, 2, torch.float32)
        assert qkv.dtype == torch.float32 and dctx.dtype == torch.float32 and B == 5 and lens[3] == 1
        assert not (ids[4, :136] > 0).any() and (ids[4, 136:S - 3] > 0).all()


def test_f32_long_reference_floors():
    fl = measure_floors()
    print({k: "%.3g" % v for k, v in fl.items()})
    assert set(fl) == set(F32_LONG_BOUNDS), set(fl) ^ set(F32_LONG_BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, bound = F32_LONG_BOUNDS[key]
        if f > 1.5 * rec:
            bad.append((key, "floor moved", f, rec))
        if not (2 * f <= bound and 2 * rec <= bound):
            bad.append((key, "floor above half the bound", f, bound))
    assert not bad, bad


def test_f32_long_one_key_sequence_reference():
    """dQ / dK of the one-key sequence are exact zeros in ref.attention_bwd at every long S."""
    for S in T.ATTN_S_F32_LONG:
        _, one_key, _ = ref_run(S, 0.0, True)
        a, t, s = one_key["dqk"]
        assert a.shape[0] == 1 and a.numel() > 0
        assert float(a.abs().max()) == 0.0, f"one-key dQ / dK S={S}"
        T.assert_elementwise(a, t, s, 1.0, f"one-key dQ / dK S={S}")


if __name__ == "__main__":
    for k, v in sorted(measure_floors().items()):
        print(k, "%.3g" % v)
