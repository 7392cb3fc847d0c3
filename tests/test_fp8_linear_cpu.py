"""The fp8 (E4M3) inference matmul mode on the CPU: the reference quantiser's contract (docs/PARITY.md), the
mode switch and its command-line flag, and the path ``Linear`` takes with the mode on."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, ref

E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
E4M3 = E4M3[~E4M3.isnan()].unique()          # the 253 values of the format, ascending
LAYER_CASES = [(144, 72, 5), (768, 3072, 40)]    # (in, out, M) of the public-path tests: skinny and tiled


def special_rows(K):
    """[3, K] fp32: zeros; one amax element, the rest 2^-12, 2^-16 (subnormal) and 2^-19 (flushed) of it; mixed signs."""
    v = torch.zeros(3, K)
    v[1] = 3.0 * 2.0 ** -12
    v[1, 0], v[1, 3::4], v[1, 5::4] = 3.0, -3.0 * 2.0 ** -16, 3.0 * 2.0 ** -19
    v[2] = torch.randn(K, generator=torch.Generator().manual_seed(K))
    return v


def quant_bound(x, w, b):
    """(fp64 product of the unquantised operands, derived bound on the fp8 path's distance from it):
    |x_hat - x| <= 2^-4 |x| + 2^-10 sx (three mantissa bits; half a subnormal step of 2^-9 in units of the
    scale), the same for w, propagated through the dot product elementwise, plus 2^-8 |y| for the bf16 output."""
    xd, wd = x.double(), w.double()
    ex = 2.0 ** -4 * xd.abs() + 2.0 ** -10 * (xd.abs().amax(1, keepdim=True) / 448)
    ew = 2.0 ** -4 * wd.abs() + 2.0 ** -10 * (wd.abs().amax(1, keepdim=True) / 448)
    y = xd @ wd.t() + b.double()
    return y, xd.abs() @ ew.t() + ex @ wd.abs().t() + ex @ ew.t() + 2.0 ** -8 * y.abs()


def layer_case(fin, fout, M):
    from pcmp.models.layers import Linear
    torch.manual_seed(fin + M)
    return Linear(fin, fout).eval(), torch.randn(M, fin).bfloat16()


@pytest.mark.parametrize("fin,fout,M", LAYER_CASES)
def test_quant_bound_holds_for_ref(fin, fout, M):
    """The bound the GPU test relies on holds for the reference ops on the same seeds."""
    lin, x = layer_case(fin, fout, M)
    with torch.no_grad():
        y = ref.linear_fp8_fwd(*ref.fp8_quant_rows(x), *ref.fp8_quant_rows(lin.weight), lin.bias, 0)
        t, bound = quant_bound(x, lin.weight, lin.bias)
    assert bool(((y.double() - t).abs() <= bound).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ref_quantiser_contract(dtype):
    v = special_rows(16).to(dtype)
    q, s = ref.fp8_quant_rows(v)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    amax, top = v.float().abs().amax(1), torch.full((3,), 448.0)
    want_s = torch.where(amax > 0, amax / top, torch.ones(3))
    assert torch.equal(s.view(torch.int32), want_s.view(torch.int32))
    r = torch.where(amax > 0, top / amax.clamp_min(1e-30), torch.zeros(3))
    t = (v.float() * r[:, None]).double()                    # the value the conversion rounds
    dist = (t[..., None] - E4M3).abs()
    best, got = dist.amin(-1), q.double()
    assert torch.equal((got - t).abs(), best), "decoded q is a nearest e4m3 value"
    tie = (dist == best[..., None]).sum(-1) > 1
    assert bool(((q.view(torch.uint8) & 1) == 0)[tie].all()), "ties go to the even code"
    assert got[0].abs().max() == 0 and got[1, 0] == 448 and got[1, 3] == -2.0 ** -7 and got[1, 5] == 0


def test_switch_and_cli_flag(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    assert _lib.infer_matmul() == "bf16"
    try:
        _lib.set_infer_matmul("fp8")
        with pytest.raises(ValueError, match="int8"):
            _lib.set_infer_matmul("int8")
        assert _lib.infer_matmul() == "fp8"
        _lib.set_infer_matmul("bf16")
        assert entry.main(["--preset", "mlp-cpu", "--infer-matmul", "fp8", "--json", str(out)]) == 0
        assert _lib.infer_matmul() == "fp8"
        assert json.loads(out.read_text().strip().splitlines()[-1])["infer_matmul"] == "fp8"
        with pytest.raises(SystemExit, match="--infer-matmul fp8 needs --dtype bf16"):
            entry.main(["--preset", "mlp-cpu", "--infer-matmul", "fp8", "--dtype", "fp32", "--json", str(out)])
        assert len(out.read_text().strip().splitlines()) == 1
    finally:
        _lib.set_infer_matmul("bf16")
        _lib.set_precision("bf16")


def test_linear_cpu_paths():
    """no_grad + fp8 mode: the two reference ops composed, bitwise.  Grad enabled: the bf16-mode result."""
    lin, x = layer_case(144, 72, 5)
    y_bf16 = lin(x)
    try:
        _lib.set_infer_matmul("fp8")
        with torch.no_grad():
            y = lin(x)
            want = ref.linear_fp8_fwd(*ref.fp8_quant_rows(x), *ref.fp8_quant_rows(lin.weight), lin.bias, 0)
        y_grad = lin(x)
    finally:
        _lib.set_infer_matmul("bf16")
    assert y.dtype == torch.bfloat16 and torch.equal(y, want) and not torch.equal(y, y_bf16)
    assert y_grad.requires_grad and torch.equal(y_grad, y_bf16)
