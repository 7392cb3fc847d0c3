"""The split-bf16 fp32 matmul mode (csrc/f32_bf16x.h, knob ``f32_bf16x`` = 6 / 3, ``--f32-matmul bf16x6 /
bf16x3``) on the CPU: the operand split is exact, the accuracy floors of the emulation
(``pcmp.ops.truth_f32x``) and the bounds ``BOUNDS_X`` that tests/test_f32_bf16x_gpu.py holds the kernels to,
the precondition under which the exact (grid) cases stay bit-exact in the mode, the launch-plan tags under
the knob, and the command-line switch.

``BOUNDS_X[parts][(op, output)] = (floor, bound)``.  The floor is the worst ``seg_rel`` of the emulation --
the kept part products, each one fp32 convolution, added smallest first -- against the fp64 truth over every
case of ``F32_CONV_CASES`` that runs the op; ``test_floors_and_bounds`` recomputes it.  The bound is
4 * floor (rounded down to two digits), the top of the project's 2 * floor .. 4 * floor rule: the kernel
adds the same products in a serial chain over the 16-deep slabs of the reduction, while the CPU
convolution the emulation uses sums in blocks, so the kernel's accumulation error is the larger of the
two.  No bound comes from a kernel figure.
"""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth_f32x as X, truth_image_f32 as TF, truth_image_f32_run as RF

F32 = torch.float32

# parts -> (op, output) -> (floor of the emulation, bound of the GPU tests)
BOUNDS_X = {
    3: {("conv_fwd", "y"): (1.9e-07, 7.6e-07), ("conv_fwd_fold", "y"): (1.7e-07, 6.8e-07),
        ("conv_dgrad", "dx"): (2.2e-07, 8.8e-07), ("conv_dgrad", "dx_resid"): (1.2e-07, 4.8e-07),
        ("conv_wgrad", "dw"): (2.8e-07, 1.1e-06), ("conv_wgrad", "dw_acc"): (2.8e-07, 1.1e-06),
        ("conv_wgrad_fold", "dw"): (3.2e-07, 1.2e-06), ("conv_wgrad_fold", "dw_acc"): (3.2e-07, 1.2e-06)},
    2: {("conv_fwd", "y"): (8.1e-06, 3.2e-05), ("conv_fwd_fold", "y"): (1.8e-05, 7.2e-05),
        ("conv_dgrad", "dx"): (1.0e-05, 4.0e-05), ("conv_dgrad", "dx_resid"): (9.4e-06, 3.7e-05),
        ("conv_wgrad", "dw"): (6.3e-06, 2.5e-05), ("conv_wgrad", "dw_acc"): (6.3e-06, 2.5e-05),
        ("conv_wgrad_fold", "dw"): (8.0e-06, 3.2e-05), ("conv_wgrad_fold", "dw_acc"): (7.9e-06, 3.1e-05)},
}


def bounds_for(parts):
    """The (op, output) -> (floor, bound) table a GPU test checks a run in the mode against: ``BOUNDS_X`` for
    the matmul outputs; the statistics rows are sums of the implementation's own y and keep ``BOUNDS_F32``."""
    from test_image_truth_f32_cpu import BOUNDS_F32
    return {**BOUNDS_F32, **BOUNDS_X[parts]}


@pytest.fixture(scope="module")
def ops():
    from pcmp.ops import _lib
    if not _lib.load():
        pytest.skip(f"native library not built: {_lib.load_error()}")
    return torch.ops.pcmp


def bits(v):
    return torch.tensor(v, dtype=torch.int32).view(F32)


def edge_values():
    """bf16 rounding ties (the 16 dropped bits are 0x8000, on an even and on an odd kept significand), the fp32
    values one ulp either side of each, +-2^k over the whole normal range, and the largest finite value whose
    hi is finite (0x7f7f7fff: one ulp below the tie that rounds to inf).  (The lower parts of a value with
    residual bits reach 2^-16 below it, so the three-part sum is exact for |x| >= 2^-110: the ties stay above.)"""
    ties = [0x3f808000, 0x3f818000, 0x40ff8000, 0x08808000, 0x7e7e8000, 0x3fff8000]
    v = [t + d for t in ties for d in (-1, 0, 1)] + [(k + 127) << 23 for k in range(-126, 128)] + [0x7f7f7fff, 0x7f7f0000]
    x = bits(v)
    return torch.cat([x, -x])


# ------------------------------------------------------------------------------ 1. the split
def test_split_exact():
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(1 << 20, generator=gen)
    for t in (x, x * 2.0 ** 60, x * 2.0 ** -60, edge_values()):
        assert bool(torch.isfinite(t).all())
        hi, mid, lo = X.split_bf16(t, 3)
        for part in (hi, mid, lo):   # every part is a bf16 value
            assert torch.equal(part, part.to(torch.bfloat16).to(F32)) and bool(torch.isfinite(part).all())
        assert torch.equal(hi, t.to(torch.bfloat16).to(F32))
        # the sum is exact: in fp64 (no rounding at all) and as the fp32 sum smallest first
        assert torch.equal(hi.double() + mid.double() + lo.double(), t.double())
        assert torch.equal((lo + mid) + hi, t)
        h2, m2 = X.split_bf16(t, 2)
        assert torch.equal(h2, hi) and torch.equal(m2, mid)
        assert bool(((t.double() - h2.double() - m2.double()).abs() <= 2.0 ** -17 * t.double().abs()).all())
    assert X.products(3) == [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]
    assert X.products(2) == [(1, 0), (0, 1), (0, 0)]


def test_split_non_finite():
    """A non-finite x gives hi = x and zero lower parts; so does a finite x whose hi rounds to inf."""
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([inf, -inf, nan, 1.5])
    for parts in (2, 3):
        p = X.split_bf16(x, parts)
        assert torch.equal(p[0][:2], x[:2]) and bool(torch.isnan(p[0][2])) and float(p[0][3]) == 1.5
        for low in p[1:]:
            assert torch.equal(low, torch.zeros(4))
    over = bits([0x7f7f8000, 0x7f7fffff])   # finite, rounds to +inf
    p = X.split_bf16(over, 3)
    assert torch.equal(p[0], torch.tensor([inf, inf])) and float(p[1].abs().max()) == 0.0 and float(p[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------ 2. floors and bounds
def test_floors_and_bounds():
    from test_image_truth_f32_cpu import BOUNDS_F32
    for parts in (3, 2):
        fl = X.floors(parts)
        print(parts, {k: float("%.3g" % v) for k, v in fl.items()})
        assert set(fl) == set(BOUNDS_X[parts]) == set(X.BOUND_KEYS)
        for key, (floor, bound) in BOUNDS_X[parts].items():
            assert abs(floor - fl[key]) <= 0.1 * fl[key], (parts, key, floor, fl[key])
            assert 2 * floor <= bound <= 4 * floor, (parts, key, floor, bound)
    for key, (_, bound) in BOUNDS_X[3].items():
        assert bound <= 1e-5, (key, bound)                     # the project's fp32 criterion
        assert bound < BOUNDS_X[2][key][0], (key, bound)       # a six-product kernel that drops a term fails
    b = bounds_for(3)
    assert b[("conv_fwd", "stats")] == BOUNDS_F32[("conv_fwd", "stats")]
    assert b[("conv_fwd_fold", "stats")] == BOUNDS_F32[("conv_fwd_fold", "stats")]


# ------------------------------------------------------------------------------ 3. the exact cases in the mode
@pytest.mark.parametrize("shape", sorted({c["shape"] for c in TF.F32_CONV_CASES.values()}), ids=str)
def test_exactness_precondition(shape):
    """On the grid inputs every matmul operand equals its hi part (xq, wq, dyq, and the folded
    relu(fsc * zq + fsh): a multiple of 1/16 below 9, 8 bits), so the lower parts are 0, every kept product
    is the exact-fp32 product or 0, and the exact cases stay ``torch.equal`` to the fp64 truth in the mode."""
    d = TF.conv_inputs(shape)
    fz = X.fold_f32(d["zq"], d["fsc"], d["fsh"])
    assert torch.equal(fz, torch.round(fz * 16) / 16) and 0 <= float(fz.min()) and float(fz.max()) < 9
    for what in X.OUTPUTS:
        for t in X.matmul_operands(shape, what, grid=True):
            for parts in (2, 3):
                p = X.split_bf16(t, parts)
                assert torch.equal(p[0], t) and all(float(q.abs().max()) == 0.0 for q in p[1:]), what


# ------------------------------------------------------------------------------ 4. tags
# The measured exception rule of plan_f32: under f32_bf16x = 6 a FWD / DGRAD of at most f32_shortk (4) K-steps stays
# on the exact big kernel and keeps its f32_big tag.  On the MI355X the three-part kernel did not pay on that class --
# the layer-1 / layer-2 1x1 convs of ResNet-50 at B = 64: 64->256 FWD 112 us against 103 us and 256->64 DGRAD 105
# against 99 us on the exact kernel, the others level (profiles/f32_bf16x_mi355x.txt); with two parts the class gains
# or stays within 10 %, so f32_bf16x = 3 has no such rule.
# The cases it moves (FWD gk = 64; DGRAD gk = 64 or 80):
STAYS_EXACT_X6 = {("lin5", "fwd"), ("lin5", "fwd_fold"), ("gm65", "dgrad"), ("w128x64", "fwd"), ("w128x64", "dgrad"),
                  ("down", "fwd"), ("down", "dgrad")}


def expected_tag(tag, parts, name, key):
    if parts == 3 and (name, key) in STAYS_EXACT_X6:
        return tag
    return tag.replace("f32_big", X.KERNEL[parts])


def test_tags_under_the_knob(ops):
    """Under f32_bf16x = 6 / 3 and the case's own knobs every committed f32_big tag reads f32x6 / f32x3 with the
    same tile, split and fold suffix -- but for STAYS_EXACT_X6, the short reductions that keep the exact big
    kernel at 6 -- and every f32_small tag is unchanged; at 0 the committed tags come back."""
    short = {(n, k) for n, c in TF.F32_CONV_CASES.items() for k, t in c["tags"].items()
             if t.startswith("f32_big") and RF.TAG_MODE[k][0] < 2 and -(-TF.gemm_dims(c["shape"], RF.TAG_MODE[k][0])[2] // 32) <= 4}
    assert short == STAYS_EXACT_X6
    def peek():
        v = ops.set_knob("f32_bf16x", 0)
        ops.set_knob("f32_bf16x", v)
        return v

    assert peek() == 0
    n_big = n_small = 0
    try:
        for parts in (3, 2):
            ops.set_knob("f32_bf16x", X.KNOB[parts])
            for what, want, got in RF.committed_tags(ops):
                name, key = what.split()
                assert got == expected_tag(want, parts, name, key), (parts, what, want, got)
                n_big += want.startswith("f32_big")
                n_small += want.startswith("f32_small")
                assert (want.startswith("f32_small") or (parts == 3 and (name, key) in STAYS_EXACT_X6)) == (got == want)
        assert n_big and n_small
        ops.set_knob("f32_bf16x", 0)
        assert all(want == got for _, want, got in RF.committed_tags(ops))
        ops.set_knob("f32_bf16x", 4)
        with pytest.raises(RuntimeError, match="f32_bf16x must be 0, 3 or 6"):
            ops.conv_f32_plan(0, 2, 6, 6, 16, 16, 3, 1, 1, 0)
    finally:
        ops.set_knob("f32_bf16x", 0)
    assert peek() == 0


def test_set_f32_matmul(ops):
    from pcmp.ops import _lib
    assert _lib.f32_matmul() == "exact"
    try:
        for name, v in (("bf16x6", 6), ("bf16x3", 3), ("exact", 0)):
            _lib.set_f32_matmul(name)
            assert _lib.f32_matmul() == name and ops.set_knob("f32_bf16x", v) == v
        with pytest.raises(ValueError, match="tf32"):
            _lib.set_f32_matmul("tf32")
    finally:
        _lib.set_f32_matmul("exact")


# ------------------------------------------------------------------------------ 5. the command line
def test_cli_flag(tmp_path):
    import another_neural_net as entry
    from pcmp.ops import _lib
    out = tmp_path / "rec.json"
    try:
        assert entry.main(["--preset", "mlp-cpu", "--dtype", "fp32", "--f32-matmul", "bf16x6", "--json", str(out)]) == 0
        rec = json.loads(out.read_text().strip().splitlines()[-1])
        assert rec["f32_matmul"] == "bf16x6"
        with pytest.raises(SystemExit, match="--f32-matmul needs --dtype fp32"):
            entry.main(["--preset", "mlp-cpu", "--f32-matmul", "bf16x6", "--json", str(out)])
        assert len(out.read_text().strip().splitlines()) == 1
    finally:
        _lib.set_f32_matmul("exact")
        _lib.set_precision("bf16")
