"""The element-wise comparator of ``pcmp.ops.truth`` and the distance of ``ops/ref.py`` from the fp64
autograd truths, on the CPU.

``BOUNDS`` holds, per (op, output), the worst ``norm_err`` of ``ops/ref.py`` against the truth over
every bf16 case of tests/test_text_truth_gpu.py (the *floor*: what the bf16 roundings of a correct
implementation cost) and the bound ``k`` the GPU tests hold the kernels to.  The kernels make the
same number of bf16 roundings as ``ref.py`` at other places in the sums, so their distance from the
truth is a second draw of the same noise: ``2*floor <= k``; and ``k <= max(1, 4*floor)`` so that a
bound never grows past what the noise explains.  ``test_reference_floors`` recomputes every floor
and checks both, which also pins the hand-derived backward formulas of ``ref.lstm_seq_bwd``,
``ref.attention_bwd`` and ``ref.layernorm_bwd*`` to autograd.

The cases are evaluated by the runners of ``pcmp.ops.truth_run`` (``ops/ref.py`` here,
``torch.ops.pcmp`` in the GPU tests).
"""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth as T, truth_run as R

# (op, output): (floor of ops/ref.py on the CPU, bound k of the GPU tests).
# bf16 outputs: k = 2 * floor rounded up to a multiple of 0.5, and at least 1.  fp32 outputs (statistics, lse,
# fp32 gradient sums; floors of 1e-5 and below): k = 0.01, i.e. |err| <= 1e-4*|t| + 5e-5*max|t| --
# a few hundred fp32 ulps for the fast exp / log / rsqrt and the other summation order of the kernels,
# two orders of magnitude below anything a bf16 slip would leave.
BOUNDS = {
    ("lstm", "hout"): (0.223, 1.0), ("lstm", "gates"): (0.191, 1.0), ("lstm", "c"): (0.124, 1.0),
    ("lstm", "dgates"): (0.234, 1.0),
    ("attention_p0", "ctx"): (0.398, 1.0), ("attention_p0", "lse"): (1.3e-5, 0.01), ("attention_p0", "dqkv"): (0.467, 1.0),
    ("attention_drop", "ctx"): (0.373, 1.0), ("attention_drop", "lse"): (7.7e-6, 0.01),
    ("attention_drop", "dqkv"): (0.425, 1.0),
    ("layernorm", "y"): (0.254, 1.0), ("layernorm", "xs"): (0.0, 1.0), ("layernorm", "mean"): (1.1e-6, 0.01),
    ("layernorm", "rstd"): (8.6e-6, 0.01), ("layernorm", "dx"): (0.255, 1.0), ("layernorm", "dxd"): (0.401, 1.0),
    ("layernorm", "dgamma"): (2.6e-5, 0.01), ("layernorm", "dbeta"): (5.8e-7, 0.01), ("layernorm", "dbias"): (0.514, 1.5),
    ("embed_layernorm", "y"): (0.225, 1.0), ("embed_layernorm", "xs"): (0.0, 1.0),
    ("embed_layernorm", "mean"): (1.8e-6, 0.01), ("embed_layernorm", "rstd"): (5.6e-6, 0.01),
    ("act", "gelu_y"): (0.035, 1.0), ("act", "gelu_dx"): (0.168, 1.0), ("act", "tanh_y"): (0.187, 1.0),
    ("act", "tanh_dx"): (0.675, 1.5), ("act", "add"): (0.162, 1.0),
    ("embedding", "y"): (0.0, 1.0), ("embedding", "dW"): (4.5e-6, 0.01),
    ("masked_mean", "y"): (0.206, 1.0), ("masked_mean", "dx"): (0.169, 1.0),
}

def measure_floors():
    fl = {}

    def upd(op, res):
        for n, e in R.worst(res).items():
            fl[(op, n)] = max(fl.get((op, n), 0.0), e)

    for shp in T.LSTM_SHAPES:
        upd("lstm", R.run_lstm(ref, T.lstm_case(*shp))[0])
    for S in T.ATTN_S:
        for p, with_ids in ((0.0, True), (0.1, True), (0.0, False)):
            upd(R.attn_op(p), R.run_attention(ref, T.attn_case(S, p, with_ids), S, p)[0])
    for M, D in T.LN_SHAPES:
        for v in R.ln_variants(M, D):
            upd("layernorm", R.run_layernorm(ref, T.ln_case(M, D, v[0]), v)[0])
    for shp in T.EMBED_LN_SHAPES:
        upd("embed_layernorm", R.run_embed_layernorm(ref, T.embed_ln_case(*shp)))
    for n in (8, 8 * 257):
        upd("act", R.run_activations(ref, T.act_case(n))[0])
    for E in (8, 136):
        for case in T.embedding_cases(E):
            for acc in (False, True):
                upd("embedding", R.run_embedding(ref, case, acc)[0])
    for D in (8, 264):
        for S in (1, 40):
            upd("masked_mean", R.run_masked_mean(ref, T.masked_mean_case(D, S))[0])
    return fl


# ------------------------------------------------------------------------------ tests
def old_close(a, b, rtol=2e-2, atol=2e-2):
    """The whole-tensor bound of tests/test_text_kernels_gpu.py."""
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() <= atol + rtol * b.abs().max().item()


def _rejects(a, t, seg):
    with pytest.raises(AssertionError):
        T.assert_elementwise(a, t, seg, 1.0)


def test_comparator_rejects_localised_defects():
    """Six synthetic defects on a copy of a truth tensor, each rejected at k = 1.  The whole-tensor
    ``close()`` of test_text_kernels_gpu.py (at the tolerances it is called with there) accepts a
    (3 % on one ctx tile), b (5 % on one head's dQ, judged against max|dqkv|) and f (anything below
    5e-2 * (1 + max|dgates|) at a padded step); it rejects c at this small shape (it would not where
    neighbouring timesteps differ by less than 3e-2 * (1 + max|h|)), d (a zeroed LayerNorm row) and
    e (dgamma is judged there at rtol 1e-3, atol 1e-2)."""
    B, S, H = 4, 128, 2
    qkv, ids, dctx, _, _ = T.attn_case(S, 0.0)
    ctx, lse, dqkv = T.attention(qkv, ids, B, S, H, dctx=dctx)
    T.assert_elementwise(*R.seg_view(ctx.clone(), ctx, lambda x: T.seg_ctx(x, B, S, H)), 1.0)
    # a. one 16-query x 64 tile of one head of ctx scaled by 1.03
    v, seg = T.seg_ctx(ctx.clone(), B, S, H)
    v[1, 32:48, 1, :] *= 1.03
    _rejects(v, T.seg_ctx(ctx, B, S, H)[0], seg)
    assert old_close(v.reshape(ctx.shape), ctx)
    # b. dQ of one head of one sequence scaled by 1.05
    v, seg = T.seg_dqkv(dqkv.clone(), B, S, H)
    v[2, :, 0, 1, :] *= 1.05
    _rejects(v, T.seg_dqkv(dqkv, B, S, H)[0], seg)
    assert old_close(v.reshape(dqkv.shape), dqkv, 3e-2, 3e-2)
    # c. one 16-unit block of hout at one timestep replaced by the previous timestep's values
    gx, whh, lids, dh = T.lstm_case(5, 7, 32)
    hout, gates, c, dgates = T.lstm(gx, whh, lids, dh)
    v = hout.clone()
    v[0, 4, 16:32] = hout[0, 3, 16:32]
    _rejects(T.seg_hout(v, 32)[0], T.seg_hout(hout, 32)[0], T.seg_hout(hout, 32)[1])
    assert not old_close(v, hout, 3e-2, 3e-2)
    # f. a non-zero value written at a padded step of dgates (row 2 is all pad)
    v = dgates.clone()
    assert float(dgates[2].abs().max()) == 0.0
    v[2, 3, 1, 5] = 0.02     # the bound there is 5e-3 * max|segment|; the GPU tests also ask for exact zeros
    _rejects(T.seg_gates(v, 32)[0], T.seg_gates(dgates, 32)[0], T.seg_gates(dgates, 32)[1])
    assert old_close(v, dgates, 5e-2, 5e-2)
    # ... and a segment whose truth is identically zero takes nothing but zeros
    z = torch.zeros(3, 4)
    T.assert_elementwise(z.clone(), z, (1,), 1.0)
    bad = z.clone()
    bad[1, 2] = 1e-30
    _rejects(bad, z, (1,))
    # d. the last row of an LN output zeroed
    x, r, g, b, dy = T.ln_case(2, 768, True)
    t = T.layernorm(T.ln_input(x, r), g, b, 1e-12, dy)
    v = t["y"].clone()
    v[-1] = 0
    _rejects(v, t["y"], (1,))
    assert not old_close(v, t["y"])
    # e. one column of dgamma off by 2 % (the largest one: 2 % of a column below half the maximum
    #    is inside the element-wise bound too)
    x, r, g, b, dy = T.ln_case(13, 768, True)
    t = T.layernorm(T.ln_input(x, r), g, b, 1e-12, dy)
    v = t["dgamma"].clone()
    v[int(t["dgamma"].abs().argmax())] *= 1.02
    _rejects(v, t["dgamma"], (0,))
    assert not old_close(v, t["dgamma"], 1e-3, 1e-2)
    # NaN never passes
    v = t["y"].clone()
    v[0, 0] = float("nan")
    _rejects(v, t["y"], (1,))


def test_reference_floors():
    fl = measure_floors()
    print({k: round(v, 3) for k, v in fl.items()})
    assert set(fl) == set(BOUNDS), set(fl) ^ set(BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, k = BOUNDS[key]
        # the recorded floor is this measurement (summation order of the CPU BLAS may move it a little)
        if abs(f - rec) > 0.1 * rec + 0.02:
            bad.append((key, "floor moved", f, rec))
        if not (2 * f <= k and k <= max(1.0, 4 * f)) or not (2 * rec <= k and k <= max(1.0, 4 * rec)):
            bad.append((key, "2*floor <= k <= max(1, 4*floor) violated", f, k))
    assert not bad, bad


def test_attention_one_key_sequence_reference():
    """ref.attention_bwd forms D = sum_j P_j dP_j like the kernels: dQ and dK of a sequence with one
    valid key are exactly zero."""
    for S in T.ATTN_S:
        _, one_key, _ = R.run_attention(ref, T.attn_case(S, 0.0), S, 0.0)
        T.assert_elementwise(*one_key["dqk"], 1.0, f"one-key dQ / dK S={S}")


def test_attention_all_pad_sequence_is_outside_the_contract():
    """A sequence with no valid key has no softmax.  ``ref.attention_fwd`` (and the kernels' same
    lse construction) return something finite there, not a mean of V by contract; the docstring
    says so, and the other sequences of the batch do not see it."""
    assert "outside the contract" in ref.attention_fwd.__doc__
    S, H = 32, 2
    qkv, ids, dctx, B, _ = T.attn_case(S, 0.0)
    ids3 = torch.stack([ids[0], torch.zeros_like(ids[0]), ids[2]])
    q3, d3 = qkv.view(B, S, -1)[[0, 1, 2]].reshape(3 * S, -1), dctx.view(B, S, -1)[[0, 1, 2]].reshape(3 * S, -1)
    q2, d2 = qkv.view(B, S, -1)[[0, 2]].reshape(2 * S, -1), dctx.view(B, S, -1)[[0, 2]].reshape(2 * S, -1)
    c3, l3 = ref.attention_fwd(q3, ids3, 3, S, H, 0.0, 0, 0)
    g3 = ref.attention_bwd(d3, q3, c3, l3, ids3, 3, S, H, 0.0, 0, 0)
    c2, l2 = ref.attention_fwd(q2, ids3[[0, 2]], 2, S, H, 0.0, 0, 0)
    g2 = ref.attention_bwd(d2, q2, c2, l2, ids3[[0, 2]], 2, S, H, 0.0, 0, 0)
    for a in (c3, l3, g3):
        assert torch.isfinite(a.float()).all()
    assert torch.equal(c3.view(3, S, -1)[[0, 2]], c2.view(2, S, -1))
    assert torch.equal(l3.view(3, H, S)[[0, 2]], l2.view(2, H, S))
    assert torch.equal(g3.view(3, S, -1)[[0, 2]], g2.view(2, S, -1))


if __name__ == "__main__":
    for k, v in sorted(measure_floors().items()):
        print(k, "%.3g" % v)
