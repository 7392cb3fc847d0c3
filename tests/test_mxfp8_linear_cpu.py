"""The mxfp8 (block-scaled E4M3) inference matmul mode on the CPU: the reference quantiser's contract (docs/PARITY.md),
the mode switch and its flag, the path ``Linear`` takes, and the conditions the GPU tests put on the cases they share."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, ref
from test_fp8_linear_cpu import E4M3

LAYER_CASES = [(160, 72, 5), (768, 3072, 40)]    # (in, out, M) of the public-path tests: skinny and tiled
# (M, K, N, act, seed) of the out_mx tests: the first seeds that pass test_out_mx_case_conditions
OUT_MX_CASES = [(17, 128, 32, 2, 0), (17, 128, 32, 1, 0), (129, 416, 160, 2, 3), (129, 416, 160, 1, 3)]


def block_scaled(R, K, gen, std=1.0):
    """[R, K] fp32 randn, each 32-block times 2^j, j per block from -6..6: a scale applied to the wrong block shows."""
    j = torch.randint(-6, 7, (R, K // 32, 1), generator=gen)
    return (torch.randn(R, K // 32, 32, generator=gen) * std * 2.0 ** j).view(R, K)


def special_blocks():
    """[7, 32]: zeros; amax 448; 449; mantissa 1.75 and the next fp32; rest at 2^-12, 2^-16, 2^-19 of amax; mixed signs."""
    v = torch.zeros(7, 32)
    v[1, 5], v[2, 5], v[3, 5] = 448.0, -449.0, 14.0
    v[4, 5] = torch.nextafter(torch.tensor(14.0), torch.tensor(16.0))
    v[1:5, 6] = 1.0
    v[5] = 3.0 * 2.0 ** -12
    v[5, 0], v[5, 3::4], v[5, 5::4] = 3.0, -3.0 * 2.0 ** -16, 3.0 * 2.0 ** -19
    v[6] = torch.randn(32, generator=torch.Generator().manual_seed(32))
    return v


def rule_scale(amax):
    """Biased E8M0 byte by the rule's definition, on fp64 amax: the smallest t with amax / 2^t <= 448."""
    f, p = torch.frexp(amax.double() / 448)            # amax / 448 = f * 2^p, 0.5 <= f < 1
    t = torch.where(f == 0.5, p - 1, p).clamp_min(-127)
    return torch.where(amax > 0, t + 127, torch.full_like(t, 127)).to(torch.uint8)


def mx_truth(xq, ex, wq, ew, b, act):
    """The product formula of the contract in fp64."""
    t = ref.mxfp8_dequant(xq, ex, torch.float64) @ ref.mxfp8_dequant(wq, ew, torch.float64).t()
    t = t + b.double() if b is not None else t
    return torch.relu(t) if act == 1 else torch.nn.functional.gelu(t) if act == 2 else t


def out_mx_case(M, K, N, act, seed):
    """Quantised operands, bias, fp64 truth.  x row 3 is zero and block 0's bias negative: ReLU leaves a zero block."""
    gen = torch.Generator().manual_seed(seed)
    x = block_scaled(M, K, gen)
    x[3] = 0
    b = torch.randn(N, generator=gen) * 0.5
    b[:32] = -b[:32].abs()
    xq, ex = ref.mxfp8_quant(x.bfloat16())
    wq, ew = ref.mxfp8_quant(block_scaled(N, K, gen, 0.05))
    return xq, ex, wq, ew, b, mx_truth(xq, ex, wq, ew, b, act)


def quant_bound(x, w, b):
    """(fp64 product of the unquantised operands, bound on the mxfp8 path's distance from it): test_fp8_linear_cpu's
    bound with the block's 2^t where the row's amax / 448 stands, |x_hat - x| <= 2^-4 |x| + 2^-10 2^t, same for w."""
    def err(v):
        s = torch.ldexp(torch.ones((), dtype=torch.float64), rule_scale(v.abs().view(len(v), -1, 32).amax(2)).int() - 127)
        return 2.0 ** -4 * v.abs() + 2.0 ** -10 * s.repeat_interleave(32, 1)
    xd, wd = x.double(), w.double()
    ex, ew = err(xd), err(wd)
    y = xd @ wd.t() + b.double()
    return y, xd.abs() @ ew.t() + ex @ wd.abs().t() + ex @ ew.t() + 2.0 ** -8 * y.abs()


def layer_case(fin, fout, M):
    from pcmp.models.layers import Linear
    gen = torch.Generator().manual_seed(fin + M)
    lin = Linear(fin, fout).eval()
    with torch.no_grad():
        lin.weight.copy_(block_scaled(lin.weight.shape[0], fin, gen, fin ** -0.5))
    return lin, block_scaled(M, fin, gen).bfloat16()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ref_quantiser_contract(dtype):
    v = special_blocks().to(dtype)
    q, e = ref.mxfp8_quant(v)
    assert q.dtype == torch.float8_e4m3fn and e.dtype == torch.uint8 and e.shape == (7, 4)
    assert torch.equal(e[:, 0], rule_scale(v.float().abs().amax(1))) and bool((e[:, 1:] == 127).all())
    t = v.double() * 2.0 ** (127 - e[:, :1].double())           # the value the conversion rounds
    dist = (t[..., None] - E4M3).abs()
    best, got = dist.amin(-1), q.double()
    assert torch.equal((got - t).abs(), best), "decoded q is a nearest e4m3 value"
    tie = (dist == best[..., None]).sum(-1) > 1
    assert bool(((q.view(torch.uint8) & 1) == 0)[tie].all()), "ties go to the even code"
    assert got[0].abs().max() == 0 and got[5, 0] == 384 and got[5, 3] == -3 * 2.0 ** -9 and got[5, 5] == 0
    if dtype == torch.float32:   # t = 0, 1 | E - 8, E - 7 around the mantissa 1.75
        assert e[:5, 0].tolist() == [127, 127, 128, 122, 123] and got[1, 5] == 448 and got[2, 5] == -224
    e = ref.mxfp8_quant(block_scaled(3, 160, torch.Generator().manual_seed(0)).to(dtype))[1]
    assert e.shape == (3, 8) and bool((e[:, 5:] == 127).all()) and e[:, :5].unique().numel() > 2, "K = 160: three pad bytes"


@pytest.mark.parametrize("M,K,N,act,seed", OUT_MX_CASES)
def test_out_mx_case_conditions(M, K, N, act, seed):
    """No block amax of the truth within relative 2^-10 of a threshold 1.75 * 2^j; ReLU leaves an all-zero block."""
    amax = out_mx_case(M, K, N, act, seed)[-1].abs().view(M, N // 32, 32).amax(2)
    f = torch.frexp(amax[amax > 0])[0]                           # threshold: mantissa 1.75 = 0.875 * 2
    assert bool(((f - 0.875).abs() > 0.875 * 2.0 ** -10).all())
    assert act != 1 or bool((amax == 0).any())


def test_switch_and_cli_flag(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    assert _lib.infer_matmul() == "bf16"
    try:
        _lib.set_infer_matmul("mxfp8")
        assert _lib.infer_matmul() == "mxfp8"
        _lib.set_infer_matmul("bf16")
        assert entry.main(["--preset", "mlp-cpu", "--infer-matmul", "mxfp8", "--json", str(out)]) == 0
        assert _lib.infer_matmul() == "mxfp8"
        assert json.loads(out.read_text().strip().splitlines()[-1])["infer_matmul"] == "mxfp8"
        with pytest.raises(SystemExit, match="--infer-matmul mxfp8 needs --dtype bf16"):
            entry.main(["--preset", "mlp-cpu", "--infer-matmul", "mxfp8", "--dtype", "fp32", "--json", str(out)])
        assert len(out.read_text().strip().splitlines()) == 1
    finally:
        _lib.set_infer_matmul("bf16")
        _lib.set_precision("bf16")


@pytest.mark.parametrize("fin,fout,M", LAYER_CASES)
def test_linear_cpu_paths(fin, fout, M):
    """no_grad + mxfp8 mode: the two reference ops composed, bitwise, inside the bound the GPU test uses on the same
    seeds.  Grad enabled: the bf16-mode result."""
    lin, x = layer_case(fin, fout, M)
    y_bf16 = lin(x)
    try:
        _lib.set_infer_matmul("mxfp8")
        with torch.no_grad():
            y = lin(x)
            want = ref.linear_mxfp8_fwd(*ref.mxfp8_quant(x), *ref.mxfp8_quant(lin.weight), lin.bias, 0)[0]
            t, bound = quant_bound(x, lin.weight, lin.bias)
        y_grad = lin(x)
    finally:
        _lib.set_infer_matmul("bf16")
    assert y.dtype == torch.bfloat16 and torch.equal(y, want) and not torch.equal(y, y_bf16)
    assert bool(((y.double() - t).abs() <= bound).all())
    assert y_grad.requires_grad and torch.equal(y_grad, y_bf16)
