"""The loss head's reference on the CPU: the distance of ``ops/ref.py`` from the fp64 truths of
``pcmp.ops.truth_loss`` over every case of tests/test_loss_truth_gpu.py, and the bounds the kernels are
held to.

``BOUNDS_LOSS[(op, output)] = (floor, bound, criterion)``.  fp32 outputs (``loss_rows`` and ``logp`` in
both dtypes, everything of the fp32 ops, the bf16 colsum's fp32 sums) are held to ``seg_rel < 1e-5``, the
project's fp32 criterion, and the reference's floor must be at most a quarter of it.  bf16 outputs follow
the rule of tests/test_image_truth_cpu.py on ``norm_err``: k = 2 * floor rounded up to a multiple of 0.5,
at least 1.  ``test_reference_floors`` recomputes every floor and enforces both rules."""
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth_loss as L

F32, BF = L.F32, L.BF
S, N = "seg_rel", "norm_err"

BOUNDS_LOSS = {
    ("softmax_xent", "loss_rows"): (7.6e-08, 1e-5, S), ("softmax_xent", "logp"): (8.2e-08, 1e-5, S),
    ("softmax_xent", "p"): (8.2e-07, 1e-5, S),
    ("softmax_xent_bf16", "loss_rows"): (4.4e-08, 1e-5, S), ("softmax_xent_bf16", "logp"): (5.2e-08, 1e-5, S),
    ("softmax_xent_bf16", "p"): (0.24, 1.0, N),
    ("loss_mean", "mean"): (1.1e-07, 1e-5, S),
    ("xent_grad_scale", "out"): (8.3e-08, 1e-5, S), ("xent_grad_scale_bf16", "out"): (0.23, 1.0, N),
    ("log_softmax_bwd", "dz"): (1.2e-06, 1e-5, S), ("log_softmax_bwd_bf16", "dz"): (0.23, 1.0, N),
    ("colsum_bf16", "sum"): (1.3e-08, 1e-5, S), ("colsum_bf16", "sum_acc"): (3.4e-08, 1e-5, S),
}


def _sfx(dtype):
    return "" if dtype == F32 else "_bf16"


def collect_results(impl=ref, dev="cpu"):
    """{(op, output): [(got, truth, seg_dims), ...]} over every case; the exact-zero contracts are asserted
    on the way (they hold for any implementation)."""
    out = {}

    def upd(op, res):
        for n, v in res.items():
            out.setdefault((op, n), []).extend(L.chunks(v))

    for dtype in (F32, BF):
        for B in L.XENT_B:
            for V in L.XENT_V:
                for k0, gs, lk, wl, wg in L.xent_variants(B):
                    res, zero, _ = L.run_xent(impl, B, V, dtype, gs, lk, wl, wg, dev, k0)
                    for z in zero:
                        assert float(z.float().abs().max() if z.numel() else 0.0) == 0.0, (B, V, dtype, lk)
                    upd(L.xent_op(dtype), res)
        for n in L.GRAD_SCALE_N:
            for valid in (0, 1, 29):
                upd("xent_grad_scale" + _sfx(dtype), L.run_grad_scale(impl, n, dtype, valid, dev)[0])
        for B, V in L.LSM_BWD_SHAPES:
            upd("log_softmax_bwd" + _sfx(dtype), L.run_lsm_bwd(impl, B, V, dtype, dev)[0])
    for B in L.LOSS_MEAN_B:
        upd("loss_mean", L.run_loss_mean(impl, B, False, dev)[0])
    for M, C in L.COLSUM_SHAPES:
        upd("colsum_bf16", L.run_colsum(impl, M, C, dev)[0])
    return out


def measure_floors():
    return {key: L.worst({key[1]: v}, L.seg_rel if BOUNDS_LOSS[key][2] == S else L.norm_err)[key[1]]
            for key, v in collect_results().items()}


def test_reference_floors():
    fl = measure_floors()
    print({k: float("%.2g" % v) for k, v in fl.items()})
    assert set(fl) == set(BOUNDS_LOSS), set(fl) ^ set(BOUNDS_LOSS)
    bad = []
    for key, f in fl.items():
        rec, bound, crit = BOUNDS_LOSS[key]
        if crit == S:
            if not (rec / 2 - 3e-8 <= f <= 2 * rec + 3e-8):
                bad.append((key, "floor moved", f, rec))
            if bound != 1e-5 or not 4 * f <= bound or not 4 * rec <= bound:
                bad.append((key, "a floor must be at most a quarter of its bound", f, rec, bound))
        else:
            if abs(f - rec) > 0.1 * rec + 0.02:
                bad.append((key, "floor moved", f, rec))
            if bound != max(1.0, math.ceil(4 * rec) / 2) or not 2 * f <= bound:
                bad.append((key, "k must be 2 * floor rounded up to 0.5, at least 1", f, rec, bound))
    assert not bad, bad


def test_cases_are_what_they_claim():
    """The rows the cases are built for: the wide-range row spans 160, the confident row's softmax is 1 at
    its label in fp64 up to 1e-20 (p - onehot has cancelled), the mixed labels hold an ignored row, a label
    >= V and a negative label other than ignore_index, and every row of the truth's softmax sums to 1."""
    for dtype in (F32, BF):
        for V in L.XENT_V:
            c = L.xent_case(37, V, dtype)
            z, lab = c["z"].double(), c["labels"]["mixed"]
            assert float(z[0].max() - z[0].min()) == 160.0 and float(z[1].max() - z[1].min()) == 0.0
            top = z[2].topk(2).values
            assert float(top[0] - top[1]) >= 59.0 and int(lab[2]) == int(z[2].argmax())
            assert int(lab[5]) == L.IGNORE and int(lab[6]) >= V and int(lab[7]) < 0 and int(lab[7]) != L.IGNORE
            t = L.xent_truth(c["z"], lab)
            assert int(t["valid"].sum()) == 34 and float((t["p"].sum(1) - 1).abs().max()) < 1e-12
            assert 0.0 < 1.0 - float(t["p"][2, lab[2]]) < 1e-20 or float(t["p"][2, lab[2]]) == 1.0
            assert float(t["loss_rows"][~t["valid"]].abs().max()) == 0.0 and float(t["dz"][~t["valid"]].abs().max()) == 0.0
            assert not bool(L.xent_truth(c["z"], c["labels"]["all_ignored"])["valid"].any())


def test_loss_mean_contract():
    """The valid count is exact at every B (on both sides of the 256-thread loop); an all-ignored batch
    gives [0, 0]."""
    for B in L.LOSS_MEAN_B:
        _, got, want, _ = L.run_loss_mean(ref, B)
        assert got == want > 0
        res, got, want, raw = L.run_loss_mean(ref, B, all_ignored=True)
        assert got == want == 0.0 and float(raw[0][0]) == 0.0


def test_log_softmax_bwd_zero_sum_rows():
    """fp32, g on a grid with rows summing to exactly zero: dz is g bitwise."""
    for B, V in L.LSM_BWD_SHAPES:
        res, raw, g = L.run_lsm_bwd(ref, B, V, F32, grid=True)
        assert torch.equal(raw[0], g)


def test_comparator_rejects_loss_defects():
    """Defects a whole-tensor tolerance lets through, injected into results of ``ops/ref.py``: a logp row
    shifted by 2e-4 (an lse off by that much), the softmax of the wide-range row renormalised by 1 + 1e-4,
    and a loss left at an invalid row."""
    res, zero, raw = L.run_xent(ref, 37, 1000, F32, 1.0, "mixed", True, True)
    L.check(BOUNDS_LOSS, "softmax_xent", res)
    a, t, s = res["logp"]
    v = a.clone()
    v[3] += 2e-4
    with pytest.raises(AssertionError):
        L.check(BOUNDS_LOSS, "softmax_xent", {"logp": (v, t, s)})
    a, t, s = res["p"]
    v = a.clone()
    v[0] *= 1 + 1e-4
    with pytest.raises(AssertionError):
        L.check(BOUNDS_LOSS, "softmax_xent", {"p": (v, t, s)})
    assert all(float(z.abs().max()) == 0.0 for z in zero)


if __name__ == "__main__":
    for k, v in sorted(measure_floors().items()):
        print(k, "%.2g" % v)
