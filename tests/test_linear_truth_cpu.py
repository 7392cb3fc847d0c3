"""The distance of ``ops/ref.py`` from the fp64 truths of ``pcmp.ops.truth_linear`` (the Linear GEMMs
with the GELU / GELU' epilogues and the planned DGRAD), the input conditions of the committed cases,
the kernels the committed tags cover, and the Linear defects the element-wise comparator must reject,
on the CPU.

``BOUNDS`` holds, per (op, output), the worst ``norm_err`` of ``ops/ref.py`` against the truth over
every case of tests/test_linear_truth_gpu.py (the *floor*) and the bound ``k`` the GPU tests hold the
kernels to, by the rule of tests/test_image_truth_cpu.py: k = 0.01 for a floor <= 1e-4; otherwise
2 * floor rounded up to a multiple of 0.5, at least 1 and never above max(1, 4 * floor).
``test_reference_floors`` recomputes every floor and enforces the rule.  The tails case, judged per row,
goes under the same outputs: its floors (u 0.23, g 0.40, du 0.22) lie within those of the other cases.
"""
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth_linear as T, truth_linear_run as R
from pcmp.ops.truth import ABS_FRAC, REL

# (op, output): (floor of ops/ref.py on the CPU, bound k of the GPU tests)
BOUNDS = {
    ("linear", "u"): (0.256, 1.0), ("linear", "g"): (0.473, 1.0), ("linear", "du"): (0.251, 1.0),
    ("linear", "dx"): (0.232, 1.0), ("linear", "dx_resid"): (0.251, 1.0),
}


def collect_results():
    """{(op, output): [(got, truth, seg_dims), ...]} of ops/ref.py over every case (the planner cases
    share their inputs: ops/ref.py gives each of them the same figures)."""
    out = {}
    for case in T.ALL_CASES.values():
        res = {}
        if "fwd" in case["tags"]:
            res.update(R.run_fwd(ref, case)[0])
        if len(T.forms(case)) > ("fwd" in case["tags"]):
            res.update(R.run_dgrad(ref, case)[0])
        for n, v in res.items():
            out.setdefault(("linear", n), []).extend(R.chunks(v))
    return out


def measure_floors():
    return {key: max(float(T.norm_err(a, t, s).max()) for a, t, s in v) for key, v in collect_results().items()}


@pytest.fixture(scope="module")
def ops():
    from pcmp.ops import _lib
    if not _lib.load():
        pytest.skip(f"native library not built: {_lib.load_error()}")
    return torch.ops.pcmp


# ------------------------------------------------------------------------------ tests
def test_reference_floors():
    fl = measure_floors()
    print({k: float("%.3g" % v) for k, v in fl.items()})
    assert set(fl) == set(BOUNDS), set(fl) ^ set(BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, k = BOUNDS[key]
        # the recorded floor is this measurement (summation order of the CPU BLAS may move it a little)
        if abs(f - rec) > 0.1 * rec + 0.02:
            bad.append((key, "floor moved", f, rec))
        want = 0.01 if rec <= 1e-4 else max(1.0, math.ceil(4 * rec) / 2)
        if k != want or (f <= 1e-4) != (rec <= 1e-4) or (f > 1e-4 and not (2 * f <= k <= max(1.0, 4 * f))):
            bad.append((key, "k must be the rule's value for the floor", f, rec, k, want))
    assert not bad, bad


def test_grid_inputs_are_exact():
    """The precondition of the bitwise comparisons: sum |terms| / (1/8) < 2^24 for every grid output of
    every case, so every fp32 partial sum is exact in any order and under any split -- and ops/ref.py,
    which accumulates in fp32, reproduces the rounded fp64 truth bit for bit."""
    for name, case in T.ALL_CASES.items():
        assert T.grid_terms(case) < 2 ** 24, name
    for name in ("g33", "gsplit", "large_plan_dma128x128_ns3"):
        case = T.ALL_CASES[name]
        pairs = dict(R.run_fwd(ref, case, grid=True)[0])
        if len(T.forms(case)) > 1:
            pairs.update(R.run_dgrad(ref, case, grid=True)[0])
        for n, (a, t) in pairs.items():
            assert torch.equal(a, t), (name, n)


def test_input_conditions():
    """No truth segment is identically zero (per channel; per row in the tails case), and no bias or
    residual add comes near cancellation where it would matter: the fp32 noise of the terms (1e-5 of
    sum |terms|, the generous constant of tests/test_image_truth_cpu.py) stays below a tenth of the
    comparator's allowance 1e-2*|t| + 5e-3*max_seg|t| at every element -- 0.1 in norm_err units, against
    floors of 0.25 and k = 1 -- so an element whose terms cancel is still judged on a scale its rounding
    noise does not reach."""
    for (op, n), chunks in collect_results().items():
        for a, t, seg in chunks:
            assert bool((t.abs().amax(dim=seg) > 0).all()), (op, n, tuple(t.shape))
    seen = set()
    for name, case in T.ALL_CASES.items():
        tails = T.is_tails(case)
        seg = (1,) if tails else (0,)
        todo = []
        if "fwd" in case["tags"] and ("f", case["shape"], tails) not in seen:
            seen.add(("f", case["shape"], tails))
            d = T.fwd_inputs(case["shape"], tails)
            todo.append((T.fwd_truth(case["shape"], tails)["u"],
                         d["x"].double().abs() @ d["w"].double().abs().t() + d["bias"].double().abs()))
        if "dx_resid" in case["tags"] and ("d", case["dshape"], tails) not in seen:
            seen.add(("d", case["dshape"], tails))
            d = T.dgrad_inputs(case["dshape"], tails)
            todo.append((T.dgrad_truth(case["dshape"], tails)["dx_resid"],
                         d["dy"].double().abs() @ d["w"].double().abs() + d["resid"].double().abs()))
        for t, terms in todo:
            allow = REL * t.abs() + ABS_FRAC * t.abs().amax(dim=seg, keepdim=True)
            assert bool((1e-5 * terms <= 0.1 * allow).all()), name


def test_tails_reach_the_saturated_region():
    """The tails case is what it says: the FWD truth u and the DGRAD operand u_in fall below
    -T.TAILS_REACH (exp(-u^2 / 2) below the smallest fp32 denormal: __expf underflows, 1 + erf has
    cancelled completely), and u_in passes it on the positive side too."""
    case = T.TAILS_CASES["gtails"]
    u = T.fwd_truth(case["shape"], True)["u"]
    u_in = T.dgrad_inputs(case["dshape"], True)["u_in"].double()
    assert float(u.min()) < -T.TAILS_REACH and float(u.max()) > 5.55, (float(u.min()), float(u.max()))
    assert float(u_in.min()) < -T.TAILS_REACH and float(u_in.max()) > T.TAILS_REACH, (float(u_in.min()), float(u_in.max()))


def test_committed_tags(ops):
    """Every committed tag is what conv_kernel_choice reports under the case's knobs (it launches
    nothing); none reads plan/auto, except the small-M kind 6 the GELU call has no candidate for, which
    must."""
    rows = R.committed_tags(ops)
    bad = [r for r in rows if r[1] != r[2]]
    assert not bad, bad
    auto = [r[0] for r in rows if "auto" in r[1] and not r[0].startswith("small_refused")]
    assert not auto, auto
    assert [r[2] for r in rows if r[0].startswith("small_refused")] == ["plan/auto"]


def test_gelu_flags_are_exclusive(ops):
    for mode, flags in ((0, 32 | 1), (0, 32 | 8), (0, 32 | 16), (1, 256 | 1 | 32), (1, 256 | 4)):
        with pytest.raises(RuntimeError, match="excludes"):
            ops.conv_kernel_choice(mode, 147, 1, 1, 192, 192, 1, 1, 0, flags)


def test_coverage(ops):
    """The kernels the committed tags reach, read back through conv_kernel_choice."""
    got = {(form != "fwd", now) for what, want, now in R.committed_tags(ops) for form in [what.split()[1]]}
    fwd = {t for d, t in got if not d}
    dgrad = {t for d, t in got if d}
    both = fwd | dgrad
    # register-staged with GELU at row tiles of 32, 64 and 128, and the small-grid tile
    assert {"reg/32x64", "reg/64x128", "reg/128x64", "reg_smallgrid/64x128"} <= both
    # igemm_dma_kernel 128x128 and 128x64, the 8-wave 256x256, each in both modes
    for t in ("dma4/128x128", "dma4/128x64", "dma8/256x256"):
        assert t in fwd and t in dgrad, t
    # the large-M plan kinds with 1 and 3 splits, in both modes; the small-M kinds with 1 and 4
    for n in T.LARGE_KINDS.values():
        for ns in (1, 3):
            assert f"plan/{n}/ns{ns}" in fwd and f"plan/{n}/ns{ns}" in dgrad, (n, ns)
    for n in T.SMALL_KINDS.values():
        for ns in (1, 4):
            assert f"plan/{n}/ns{ns}" in fwd, (n, ns)
    assert "reg/64x128/ns3" in fwd      # FWD_SPLIT
    # every DGRAD form of the large-M cases is committed
    for case in T.LARGE_CASES.values():
        assert T.forms(case) == T.FORMS


def old_close(a, b, rtol=2e-2, atol=2e-2):
    """The whole-tensor bound of test_linear_gelu_epilogues / test_gemm32_linear_forms."""
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() <= atol + rtol * b.abs().max().item()


def _rejects(a, t, k):
    with pytest.raises(AssertionError):
        T.assert_elementwise(a, t, (0,), k)


def test_comparator_rejects_linear_defects():
    """Synthetic defects on copies of the truths of the (1030, 832, 264) case, each rejected at the k
    of its output.  The last of them -- one 4-column group of one row without the last of three
    K-splits -- passes the whole-tensor bound 2e-2 + 2e-2 * max|ref| of the older tests on g.  One
    thing is accepted, and documented as such (docs/PARITY.md): tanh-GELU in place of erf-GELU."""
    case = T.LARGE_CASES["plan_dma128x128_ns3"]
    (M, C, N), (Md, Cd, Nd) = case["shape"], case["dshape"]
    f, d = T.fwd_inputs(case["shape"]), T.dgrad_inputs(case["dshape"])
    tf, td = T.fwd_truth(case["shape"]), T.dgrad_truth(case["dshape"])
    k = {n: BOUNDS[("linear", n)][1] for n in ("u", "g", "du", "dx", "dx_resid")}
    x, w, dy, wd = f["x"].double(), f["w"].double(), d["dy"].double(), d["w"].double()
    tail = slice(128 * (M // 128), M)          # the rows of the last, partial 128-row tile
    for n in ("u", "g"):
        T.assert_elementwise(tf[n].clone(), tf[n], (0,), k[n])
    # a. the last K-tile dropped for the rows of the tail row tile
    v = tf["u"].clone()
    v[tail] -= x[tail, C - 64:] @ w[:, C - 64:].t()
    _rejects(v, tf["u"], k["u"])
    _rejects(T.gelu(v)[0], tf["g"], k["g"])
    v = td["dx"].clone()
    v[tail] -= dy[tail, Nd - 64:] @ wd[Nd - 64:]
    _rejects(v, td["dx"], k["dx"])
    # b. the bias missing in the last 8 columns
    v = tf["u"].clone()
    v[:, -8:] -= f["bias"].double()[-8:]
    _rejects(v, tf["u"], k["u"])
    _rejects(T.gelu(v)[0], tf["g"], k["g"])
    # c. gelu' taken from a column rotated by one within the last 4-column group
    u_rot = d["u_in"].clone()
    u_rot[:, -4:] = torch.roll(d["u_in"][:, -4:], 1, 1)
    _rejects(T.gelu(u_rot, td["dx"])[1], td["du"], k["du"])
    # d. the residual missing on the tail row tile
    v = td["dx_resid"].clone()
    v[tail] -= d["resid"].double()[tail]
    _rejects(v, td["dx_resid"], k["dx_resid"])
    # e. one 4-column group of one row lacking the last of three splits (5 + 5 + 3 K-tiles: the last is
    #    the reduction from 640 on).  Of the groups of the tail tile's rows, the one whose g the old
    #    bound accepts with the largest norm_err: norm_err rejects it on g and on u
    vu_all = tf["u"].clone()
    vu_all[tail] -= x[tail, 640:] @ w[:, 640:].t()
    vg_all = T.gelu(vu_all)[0]
    eg = T.norm_err(vg_all, tf["g"], (0,))      # (per-column maxima of the truth: those of the whole tensor)
    ok = (vg_all - tf["g"]).abs().float() <= 2e-2 + 2e-2 * tf["g"].float().abs().max()
    best = None
    for r in range(tail.start, M):
        for c0 in range(0, N, 4):
            if bool(ok[r, c0:c0 + 4].all()) and (best is None or float(eg[r, c0:c0 + 4].max()) > best[0]):
                best = (float(eg[r, c0:c0 + 4].max()), r, c0)
    assert best is not None
    _, r, c0 = best
    vu, vg = tf["u"].clone(), tf["g"].clone()
    vu[r, c0:c0 + 4], vg[r, c0:c0 + 4] = vu_all[r, c0:c0 + 4], vg_all[r, c0:c0 + 4]
    print("row %d, columns %d..%d without the last split: norm_err g %.3g, u %.3g"
          % (r, c0, c0 + 3, float(T.norm_err(vg, tf["g"], (0,)).max()), float(T.norm_err(vu, tf["u"], (0,)).max())))
    assert old_close(vg, tf["g"]), "the whole-tensor bound accepts it"
    _rejects(vg, tf["g"], k["g"])
    _rejects(vu, tf["u"], k["u"])
    # f. accepted: the tanh approximation of GELU (norm_err about 0.05)
    e = T.assert_elementwise(T.tanh_gelu(tf["u"]), tf["g"], (0,), k["g"])
    print("tanh-GELU against erf-GELU: norm_err %.3g" % e)
    assert e < 0.25 * k["g"]


if __name__ == "__main__":
    import time
    t0 = time.time()
    for key, v in sorted(measure_floors().items()):
        print(key, "%.3g" % v)
    print("seconds", time.time() - t0)
