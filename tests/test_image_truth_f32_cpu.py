"""The fp32 image path on the CPU: the committed launch-plan tags of ``F32_CONV_CASES`` and what they
cover, the precondition of the exact (grid) cases, the distance of ``ops/ref.py`` in fp32 from the fp64
truths (``BOUNDS_F32``), and the defects the comparators of tests/test_image_truth_f32_gpu.py must
reject.

``BOUNDS_F32`` holds, per (op, output), the worst ``seg_rel`` of ``ops/ref.py`` run in fp32 against the
truth over every random case (the *floor*) and the bound the kernels are held to: the project's fp32
criterion 1e-5, and 1e-6 for pure copies / scalings (a max-pool value, a dropout's x / (1 - p), the GAP
backward's dy / HW), as tests/test_text_truth_gpu.py has it for the text kernels.  No bound comes from a
kernel's own figure: ``test_reference_floors`` recomputes every floor and requires it to be at most a
quarter of its bound, so the reference alone shows the headroom.
"""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth_image as T, truth_image_f32 as TF, truth_image_f32_run as RF, truth_image_run as R

from test_image_truth_cpu import BN_VARIANTS

F32 = torch.float32
E5, E6 = 1e-5, 1e-6

# (op, output): (floor of ops/ref.py in fp32 on the CPU, bound of the GPU tests)
BOUNDS_F32 = {
    ("conv_fwd", "y"): (8.2e-07, E5), ("conv_fwd", "stats"): (1.4e-07, E5), ("conv_fwd_fold", "y"): (7.0e-07, E5),
    ("conv_fwd_fold", "stats"): (9.1e-08, E5), ("conv_dgrad", "dx"): (7.8e-07, E5),
    ("conv_dgrad", "dx_resid"): (6.4e-07, E5), ("conv_wgrad", "dw"): (2.6e-07, E5),
    ("conv_wgrad", "dw_acc"): (2.5e-07, E5), ("conv_wgrad_fold", "dw"): (2.3e-07, E5),
    ("conv_wgrad_fold", "dw_acc"): (2.3e-07, E5), ("conv_dgrad_bnr", "g"): (5.4e-07, E5),
    ("conv_dgrad_bnr", "part"): (1.2e-07, E5), ("conv_dgrad_bnr", "part2"): (1.2e-07, E5),
    ("bn", "part"): (7.4e-08, E5), ("bn", "mean"): (8.3e-08, E5), ("bn", "invstd"): (4.5e-08, E5),
    ("bn", "running_mean"): (7.5e-08, E5), ("bn", "running_var"): (4.8e-08, E5), ("bn", "mean2"): (1.6e-07, E5),
    ("bn", "invstd2"): (4.7e-08, E5), ("bn", "running_mean2"): (5.5e-08, E5), ("bn", "running_var2"): (4.6e-08, E5),
    ("bn", "y"): (3.3e-07, E5), ("bn", "bwd_part"): (1.6e-07, E5), ("bn", "bwd_part2"): (1.4e-07, E5),
    ("bn", "dgamma"): (1.7e-07, E5), ("bn", "dbeta"): (1.6e-07, E5), ("bn", "dgamma2"): (1.5e-07, E5),
    ("bn", "dbeta2"): (1.2e-07, E5), ("bn", "dx"): (2.4e-07, E5), ("bn", "dx2"): (1.7e-07, E5),
    ("bn_one_row", "part"): (4.2e-08, E5), ("bn_one_row", "mean"): (0.0, E5),
    ("bn_one_row", "invstd"): (4.2e-08, E5), ("bn_one_row", "running_mean"): (6.3e-08, E5),
    ("bn_one_row", "running_var"): (4.3e-08, E5), ("bn_one_row", "mean2"): (0.0, E5),
    ("bn_one_row", "invstd2"): (4.2e-08, E5), ("bn_one_row", "running_mean2"): (4.2e-08, E5),
    ("bn_one_row", "running_var2"): (3.7e-08, E5), ("bn_one_row", "y"): (5.8e-08, E5),
    ("bn_one_row", "bwd_part"): (0.0, E5), ("bn_one_row", "bwd_part2"): (0.0, E5),
    ("bn_one_row", "dgamma"): (0.0, E5), ("bn_one_row", "dbeta"): (3.8e-08, E5),
    ("bn_one_row", "dgamma2"): (0.0, E5), ("bn_one_row", "dbeta2"): (3.8e-08, E5), ("bn_one_row", "dx2"): (0.0, E5),
    ("pool", "y"): (0.0, E6), ("pool", "dx"): (4.9e-08, E5), ("pool", "y_bn"): (0.0, E5),
    ("pool", "gap_y"): (5.6e-08, E5), ("pool", "gap_dx"): (4.9e-08, E6), ("pool", "g"): (4.9e-08, E5),
    ("pool", "part"): (1.0e-07, E5), ("pool_c6", "dx"): (3.3e-08, E5), ("pool_c6", "dx_bn"): (3.3e-08, E5),
    ("dropout", "y"): (3.7e-08, E6), ("colsum", "sum"): (8.5e-08, E5), ("colsum", "sum_acc"): (9.1e-08, E5),
}


@pytest.fixture(scope="module")
def ops():
    from pcmp.ops import _lib
    if not _lib.load():
        pytest.skip(f"native library not built: {_lib.load_error()}")
    return torch.ops.pcmp


def shapes():
    """The distinct shapes of the table, each with the tag keys some case runs on it."""
    out = {}
    for c in TF.F32_CONV_CASES.values():
        out.setdefault(c["shape"], set()).update(c["tags"])
    return out


# ------------------------------------------------------------------------------ 1. tags and coverage
def test_committed_tags(ops):
    """Every tag F32_CONV_CASES commits, under the case's knobs: the assertion each GPU conv test opens
    with.  The knobs are back at their defaults afterwards."""
    def peek(n):   # set_knob returns the value it replaces
        v = ops.set_knob(n, 0)
        ops.set_knob(n, v)
        return v

    assert {n: peek(n) for n in TF.KNOB_DEFAULTS} == TF.KNOB_DEFAULTS
    assert all(set(c["knobs"]) <= set(TF.KNOB_DEFAULTS) for c in TF.F32_CONV_CASES.values())
    rows = RF.committed_tags(ops)
    bad = [r for r in rows if r[1] != r[2]]
    assert not bad, bad
    assert {n: peek(n) for n in TF.KNOB_DEFAULTS} == TF.KNOB_DEFAULTS, "a case left a knob changed"
    # the tag is host code that needs no tensor: the fold it reports must not depend on the mode's data
    with pytest.raises(RuntimeError, match="no input fold"):
        ops.conv_f32_plan(1, 2, 6, 6, 16, 16, 3, 1, 1, 1)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.conv_f32_plan(0, 2, 6, 6, 6, 16, 3, 1, 1, 0)


def entries():
    """One record per committed tag."""
    out = []
    for name, c in TF.F32_CONV_CASES.items():
        for key, tg in c["tags"].items():
            mode = RF.TAG_MODE[key][0]
            kern, bm, bn, ns, fold = TF.parse_tag(tg)
            gm, gn, gk = TF.gemm_dims(c["shape"], mode)
            out.append(dict(name=name, key=key, mode=mode, kern=kern, bm=bm, bn=bn, ns=ns, fold=fold, gm=gm, gn=gn, gk=gk,
                            nk=-(-gk // 32), shape=c["shape"], knobs=c["knobs"]))
    return out


def test_table_coverage():
    """What the issue asks the committed tags to contain (tests/test_image_truth_f32_gpu.py runs every
    one of them).  plan_f32 has neither the f32_shortk rule nor the wave-quantisation split for WGRAD: for
    that mode the test pins the absence instead (a short WGRAD reduction keeps its 128x128 tile; under the
    QSPLIT knobs the WGRAD does not split)."""
    E = entries()
    plain = [e for e in E if e["fold"] is None]

    def has(what, pred, pool=plain):
        assert any(pred(e) for e in pool), f"no committed case: {what}"

    assert all(TF.elements(c["shape"]) <= TF.MAX_ELEMENTS for c in TF.F32_CONV_CASES.values())
    N_, H_, W_, C_, K_, R_, S_, P_ = range(8)
    for mode, mname in enumerate(("FWD", "DGRAD", "WGRAD")):
        m = [e for e in plain if e["mode"] == mode]
        # igemm_f32_kernel: through f32_big = 0, with ns1 and ns > 1
        has(f"small {mname} through f32_big = 0", lambda e: e["kern"] == "f32_small" and e["knobs"].get("f32_big") == 0, m)
        has(f"small {mname} ns1", lambda e: e["kern"] == "f32_small" and e["ns"] == 1, m)
        has(f"small {mname} ns > 1", lambda e: e["kern"] == "f32_small" and e["ns"] > 1, m)
        # igemm_f32_big_kernel: the four tiles with ns1, a split with a short last part
        for bm in (64, 128):
            for bn in (64, 128):
                has(f"big {mname} {bm}x{bn} ns1",
                    lambda e: e["kern"] == "f32_big" and (e["bm"], e["bn"], e["ns"]) == (bm, bn, 1), m)
        has(f"big {mname} split, last part short",
            lambda e: e["kern"] == "f32_big" and TF.last_split_short(e["gk"], e["ns"]), m)
        wide = lambda e: e["knobs"] == TF.BIG128 and e["gm"] > 64 and e["gn"] > 64 and e["nk"] <= 4  # noqa: E731
        if mode < 2:
            # its natural fallback under the default knobs
            ch = C_ if mode == 0 else K_
            has(f"small {mname} natural fallback",
                lambda e: e["kern"] == "f32_small" and not e["knobs"] and e["shape"][ch] % 16 != 0, m)
            has(f"{mname} f32_shortk rule", lambda e: wide(e) and (e["kern"], e["bm"], e["bn"]) == ("f32_big", 64, 64), m)
            has(f"{mname} wave-quantisation split", lambda e: e["knobs"] == TF.QSPLIT and e["kern"] == "f32_big" and e["ns"] > 1, m)
        else:
            has("WGRAD: no shortk rule", lambda e: wide(e) and (e["bm"], e["bn"]) == (128, 128), m)
            has("WGRAD: no wave-quantisation split", lambda e: e["knobs"] == TF.QSPLIT and e["ns"] == 1, m)
    # reduction tails
    has("gk % 32 == 16 (C = K = 16, 3x3)", lambda e: e["kern"] == "f32_big" and e["gk"] == 144 and e["shape"][C_:R_ + 1] == (16, 16, 3))
    has("small kernel gk % 16 != 0 (C = 20, 3x3)", lambda e: e["kern"] == "f32_small" and e["mode"] == 0 and e["gk"] == 180)
    has("WGRAD with an odd gk", lambda e: e["mode"] == 2 and e["gk"] % 2 == 1)
    # tap walks
    has("C = 16, 4x4 stride 1 (two taps per K-step)",
        lambda e: e["kern"] == "f32_big" and e["mode"] == 0 and (e["shape"][C_], e["shape"][R_], e["shape"][S_]) == (16, 4, 1))
    has("7x7 stride 2 pad 3, C = 8", lambda e: e["mode"] == 0 and e["shape"][C_] == 8 and e["shape"][R_:] == (7, 2, 3))
    for mode in (0, 1, 2):
        has(f"3x3 stride 2 pad 1 on H = W = 15, mode {mode}",
            lambda e: e["mode"] == mode and e["shape"][H_:W_ + 1] == (15, 15) and e["shape"][R_:] == (3, 2, 1))
    has("1x1 stride 2 DGRAD", lambda e: e["mode"] == 1 and e["shape"][R_:] == (1, 2, 0))
    # tile tails
    for gm in (5, 33, 65, 129):
        has(f"gm = {gm}", lambda e: e["gm"] == gm)
    for gn in (12, 72, 136):
        has(f"gn = {gn}", lambda e: e["gn"] == gn)
    has("C = K = 4", lambda e: e["shape"][C_:K_ + 1] == (4, 4))
    # the input fold
    ff = [e for e in E if e["key"] == "fwd_fold"]
    has("FWD /fold, 3x3 pad 1", lambda e: e["fold"] == "fold" and e["shape"][R_:] == (3, 1, 1), ff)
    has("FWD /fold, stride 2", lambda e: e["fold"] == "fold" and e["shape"][S_] == 2, ff)
    has("FWD /apply through the small kernel", lambda e: e["fold"] == "apply" and e["kern"] == "f32_small", ff)
    has("FWD /apply through f32_fold = 0", lambda e: e["fold"] == "apply" and e["kern"] == "f32_big" and e["knobs"] == {"f32_fold": 0}, ff)
    has("WGRAD /apply", lambda e: e["fold"] == "apply", [e for e in E if e["key"] == "wgrad_fold"])
    assert all(e["fold"] for e in E if e["key"] in ("fwd_fold", "wgrad_fold"))
    # a statistics row after a split covers 16 rows, a tile row BM: both occur, with a tail row
    has("statistics rows of 16 with a tail", lambda e: e["mode"] == 0 and e["ns"] > 1 and e["gm"] % 16)
    has("statistics rows of BM with a tail", lambda e: e["mode"] == 0 and e["ns"] == 1 and e["gm"] > e["bm"] and e["gm"] % e["bm"])


# ------------------------------------------------------------------------------ 2. the exact cases
@pytest.mark.parametrize("shape", list(shapes()), ids=str)
def test_exact_precondition(shape):
    """Asserted, not assumed: the worst output element of every exact case sums fewer than 2^24 units of
    the finest grid step (so any order and any split is exact in fp32), and ``ops/ref.py`` in fp32
    reproduces the fp64 truth bit for bit."""
    keys = shapes()[shape]
    C = shape[3]
    units = TF.exact_units(shape)
    print(shape, {k: int(v) for k, v in units.items()})
    assert all(v < 2 ** 24 for v in units.values()), units
    for n, v in TF.conv_inputs(shape).items():   # every grid input is on its grid
        step = {"xq": 0.5, "wq": 0.25, "residq": 0.125, "biasq": 1 / 16, "dyq": 0.5, "dresq": 0.125, "dw0q": 0.125,
                "zq": 0.125, "fsh": 1 / 16}.get(n)
        if step:
            assert torch.equal(v, torch.round(v / step) * step), n
    d = TF.conv_inputs(shape)
    pre = d["zq"].double() * d["fsc"].double() + d["fsh"].double()
    assert float(pre.abs().min()) >= 1 / 16 and float(torch.relu(pre).max()) < 16
    if "fwd" in keys:
        RF.check_exact(RF.run_conv_fwd(ref, shape)[0], shape)
    if "fwd_fold" in keys and C % 8 == 0:
        RF.check_exact(RF.run_conv_fwd_fold(ref, shape)[0], shape)
    if "dgrad" in keys:
        RF.check_exact(RF.run_conv_dgrad(ref, shape)[0], shape)
    if "wgrad" in keys:
        RF.check_exact(RF.run_conv_wgrad(ref, shape)[0], shape)
    if "wgrad_fold" in keys:
        RF.check_exact(RF.run_conv_wgrad(ref, shape, fold=True)[0], shape)
    if shape == TF.F32_CONV_CASES["down"]["shape"]:   # 1x1 stride 2: no tap reaches an odd pixel
        t = TF.conv_truth(shape, "dx_q")
        assert float(t[:, 1::2].abs().max()) == 0.0 and float(t[:, :, 1::2].abs().max()) == 0.0


# ------------------------------------------------------------------------------ 3. floors and bounds
def collect_results():
    """{(op, output): [(got, truth, seg_dims), ...]} of ops/ref.py in fp32 over every random case."""
    out = {}

    def upd(op, res):
        for n, v in res.items():
            out.setdefault((op, n), []).extend(R.chunks(v))

    for shape, keys in shapes().items():
        if "fwd" in keys:
            upd("conv_fwd", RF.run_conv_fwd(ref, shape)[1])
        if "fwd_fold" in keys:
            upd("conv_fwd_fold", RF.run_conv_fwd_fold(ref, shape)[1])
        if "dgrad" in keys:
            upd("conv_dgrad", RF.run_conv_dgrad(ref, shape)[1])
        if "wgrad" in keys:
            upd("conv_wgrad", RF.run_conv_wgrad(ref, shape)[1])
        if "wgrad_fold" in keys:
            upd("conv_wgrad_fold", RF.run_conv_wgrad(ref, shape, fold=True)[1])
    for name in TF.BNR_F32_CASES:
        for form in TF.BNR_F32_FORMS:
            upd("conv_dgrad_bnr", RF.run_conv_dgrad_bnr(ref, TF.F32_CONV_CASES[name]["shape"], form)[0])
    for M, C in T.BN_SHAPES:
        for mode, relu, acc in BN_VARIANTS:
            upd(R.bn_op(M), R.run_bn(ref, M, C, mode, relu, acc, dtype=F32)[0])
    for shape in T.POOL_SHAPES:
        upd("pool", R.run_pool(ref, shape, dtype=F32)[0])
    upd("pool_c6", RF.run_pool_c6(ref)[1])
    for n in TF.EW_SIZES:
        upd("dropout", RF.run_dropout(ref, n)[2])
    for M, C in TF.COLSUM_SHAPES:
        upd("colsum", RF.run_colsum(ref, M, C)[0])
    return out


def measure_floors():
    return {key: max([float(RF.seg_rel(a, t, s).max()) for a, t, s in v if a.numel()], default=0.0)
            for key, v in collect_results().items()}


def test_reference_floors():
    fl = measure_floors()
    print({k: float("%.2g" % v) for k, v in fl.items()})
    assert set(fl) == set(BOUNDS_F32), set(fl) ^ set(BOUNDS_F32)
    bad = []
    for key, f in fl.items():
        rec, bound = BOUNDS_F32[key]
        # the recorded floor is this measurement, as far as the summation order of the CPU's BLAS leaves it
        # (a factor of two and a quarter of an fp32 ulp); 0 is recorded only where the reference is exact
        if not (rec / 2 - 3e-8 <= f <= 2 * rec + 3e-8) or (rec == 0.0) != (f == 0.0):
            bad.append((key, "floor moved", f, rec))
        if bound not in (E5, E6) or not 4 * f <= bound or not 4 * rec <= bound:
            bad.append((key, "a floor must be at most a quarter of its bound", f, rec, bound))
    assert not bad, bad


def test_input_conditions():
    """No recomputed mask, fold or ReLU within fp32 rounding of zero; no pooling window tied at a
    positive maximum; the BatchNorm cases as tests/test_image_truth_cpu.py asserts them for bf16."""
    near = lambda pre, terms: int((pre.abs() < 1e-5 * terms).sum())  # noqa: E731
    for shape in shapes():
        d = TF.conv_inputs(shape)
        # (the random fold relu(asc*z + ash) needs no such margin: the activation is continuous at zero, and
        # nothing is masked by it)
        for x, sc, sh in (("bx", "msc", "msh"), ("zq", "fsc", "fsh")):
            a, b = d[x].double() * d[sc].double(), d[sh].double().expand(d[x].shape)
            assert near(a + b, a.abs() + b.abs()) == 0, (shape, x)
    for M, C in T.BN_SHAPES:
        for mode in T.BN_MODES:
            t = T.bn_case(M, C, mode, True, F32)["truth"]
            assert near(t["pre"], t["terms"]) == 0, (M, C, mode)
    for shape in T.POOL_SHAPES + [TF.POOL_C6]:
        d = T.pool_case(shape, F32)
        assert d["x"].dtype == F32 and T.pool_ties(d["x"]) == 0
        a, b = d["x"].double() * d["scale"].double(), d["shift"].double().expand(d["x"].shape)
        assert T.pool_ties(torch.relu(a + b)) == 0 and near(a + b, a.abs() + b.abs()) == 0, shape
    # random fp32 inputs keep a full mantissa: they are not bf16 values
    d = TF.conv_inputs(TF.F32_CONV_CASES["split"]["shape"])
    for n in ("x", "w", "dy", "wd", "dres", "z"):
        assert not torch.equal(d[n], d[n].to(torch.bfloat16).float()), n
    assert not torch.equal(T.bn_case(50, 8, "none", False, F32)["x"], T.bn_case(50, 8, "none", False)["x"].float())


# ------------------------------------------------------------------------------ 4. the comparators
def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_comparators_reject_f32_defects():
    """Four defects, each injected into a result of ``ops/ref.py`` that passes without it."""
    shape = TF.F32_CONV_CASES["split"]["shape"]      # (2, 7, 7, 48, 48, 3, 1, 1): 98 rows, ns3 of 160 + 160 + 112
    N, H, W, C, K, Rf, s, p = shape
    d = TF.conv_inputs(shape)
    # a. one statistics row zeroed: per-16-row partials of the reference's own y (the layout after a split)
    y = ref.conv_fwd(d["x"], d["w"], s, p)[0]
    yr = y.reshape(-1, K)
    part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in yr.split(16)])
    assert part.shape[0] == RF.expected_part_rows(98, 16) == 7
    ok = {"stats": RF._stats_rows(part, y, 16)}
    RF.check_rel(BOUNDS_F32, "conv_fwd", ok)
    bad = part.clone()
    bad[6] = 0                                      # the tail row: 2 rows of y
    _rejects(lambda: RF.check_rel(BOUNDS_F32, "conv_fwd", {"stats": RF._stats_rows(bad, y, 16)}))
    # b. one padding-ring pixel set to relu(shift): the folded activation padded by hand
    import torch.nn.functional as F

    def folded(z, sc, sh, w, ring):
        a = F.pad(ref.fold_act(z, sc, sh), (0, 0, 1, 1, 1, 1))
        if ring:
            a[0, 0, 3] = torch.relu(sh)
        return ref.conv_fwd(a, w, s, 0)[0]
    tq, t = TF.conv_truth(shape, "y_fold_q"), TF.conv_truth(shape, "y_fold")
    RF.check_exact({"y_fold": (folded(d["zq"], d["fsc"], d["fsh"], d["wq"], False), tq)})
    _rejects(lambda: RF.check_exact({"y_fold": (folded(d["zq"], d["fsc"], d["fsh"], d["wq"], True), tq)}))
    RF.check_rel(BOUNDS_F32, "conv_fwd_fold", {"y": R._ch(folded(d["z"], d["asc"], d["ash"], d["w"], False), t)})
    _rejects(lambda: RF.check_rel(BOUNDS_F32, "conv_fwd_fold", {"y": R._ch(folded(d["z"], d["asc"], d["ash"], d["w"], True), t)}))
    # c. the last split's contribution dropped: reduction indices (r, s, c) >= 2 * 160 of w [K, R, S, C]
    def short(w):
        w = w.clone()
        w.reshape(K, -1)[:, 320:] = 0
        return w
    te = TF.conv_truth(shape, "y_epi")
    yq = lambda w: ref.conv_fwd(d["xq"], w, s, p, d["biasq"], d["residq"], True)[0]  # noqa: E731
    RF.check_exact({"y_epi": (yq(d["wq"]), te)})
    _rejects(lambda: RF.check_exact({"y_epi": (yq(short(d["wq"])), te)}))
    _rejects(lambda: RF.check_rel(BOUNDS_F32, "conv_fwd", {"y": R._ch(ref.conv_fwd(d["x"], short(d["w"]), s, p)[0],
                                                                   TF.conv_truth(shape, "y"))}))
    # d. one element of an exact case off by one ulp
    for n, (a, tt) in RF.run_conv_dgrad(ref, shape)[0].items():
        RF.check_exact({n: (a, tt)})
        v = a.clone()
        i = int(v.abs().reshape(-1).argmax())
        v.reshape(-1)[i] = torch.nextafter(v.reshape(-1)[i], torch.tensor(float("inf")))
        _rejects(lambda: RF.check_exact({n: (v, tt)}))


if __name__ == "__main__":
    import time
    t0 = time.time()
    for k, v in sorted(measure_floors().items()):
        print(k, "%.2g" % v)
    print("seconds", time.time() - t0)
