"""The mxfp4 (MXFP4 weights, MXFP8 activations) inference matmul mode on the CPU: the reference weight quantiser's contract
(docs/PARITY.md), its per-weight error bound, the mode switch and its flag, the path ``Linear`` takes, and the conditions
the GPU tests put on the cases they share."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, ref
from test_mxfp8_linear_cpu import LAYER_CASES, block_scaled, layer_case, rule_scale

GRID = torch.tensor(ref.E2M1_GRID, dtype=torch.float64)
TIES = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
# (M, K, N, act, seed) of the out_mx tests: the first seeds that pass test_out_mx_case_conditions
OUT_MX_CASES = [(17, 128, 32, 2, 0), (17, 128, 32, 1, 0), (129, 416, 160, 2, 12), (129, 416, 160, 1, 12)]


def special_blocks():
    """[7, 32]: zeros; amax 6 and the next fp32; mantissa 1.5 (12) and the next fp32; the seven ties times 2^-2 with
    alternating signs under an amax of 6 * 2^-2; mixed signs."""
    v = torch.zeros(7, 32)
    v[1, 5], v[2, 5], v[3, 5] = 6.0, -torch.nextafter(torch.tensor(6.0), torch.tensor(8.0)), 12.0
    v[4, 5] = torch.nextafter(torch.tensor(12.0), torch.tensor(16.0))
    v[1:5, 6] = 1.0
    v[5, :7], v[5, 7] = TIES * 0.25 * torch.tensor([1, -1, 1, -1, 1, -1, 1]), -1.5
    v[6] = torch.randn(32, generator=torch.Generator().manual_seed(32))
    return v


def rule_scale4(amax):
    """Biased E8M0 byte by the rule's definition, on fp64 amax: the smallest t with amax / 2^t <= 6."""
    f, p = torch.frexp(amax.double() / 6)              # amax / 6 = f * 2^p, 0.5 <= f < 1
    t = torch.where(f == 0.5, p - 1, p).clamp_min(-127)
    return torch.where(amax > 0, t + 127, torch.full_like(t, 127)).to(torch.uint8)


def mx4_truth(xq, ex, wq4, ew, b, act):
    """The product formula of the contract in fp64."""
    t = ref.mxfp8_dequant(xq, ex, torch.float64) @ ref.mxfp4_dequant(wq4, ew, torch.float64).t()
    t = t + b.double() if b is not None else t
    return torch.relu(t) if act == 1 else torch.nn.functional.gelu(t) if act == 2 else t


def out_mx_case(M, K, N, act, seed):
    """test_mxfp8_linear_cpu.out_mx_case with MXFP4 weights: x row 3 zero and block 0's bias negative."""
    gen = torch.Generator().manual_seed(seed)
    x = block_scaled(M, K, gen)
    x[3] = 0
    b = torch.randn(N, generator=gen) * 0.5
    b[:32] = -b[:32].abs()
    xq, ex = ref.mxfp8_quant(x.bfloat16())
    wq4, ew = ref.mxfp4_quant(block_scaled(N, K, gen, 0.05))
    return xq, ex, wq4, ew, b, mx4_truth(xq, ex, wq4, ew, b, act)


def weight_err(w):
    """The rule's per-weight bound max(|w| / 5, 2^(t-2)) in fp64: a fifth of the value where the grid's steps are relative
    (worst between 4 and 6: 1 / 5), half the smallest step 2^(t-1) below it."""
    s = torch.ldexp(torch.ones((), dtype=torch.float64), rule_scale4(w.abs().view(len(w), -1, 32).amax(2)).int() - 127)
    return torch.maximum(w.abs() / 5, s.repeat_interleave(32, 1) / 4)


def quant_bound(x, w, b):
    """test_mxfp8_linear_cpu.quant_bound with the MXFP4 error of the weight: |x_hat - x| <= 2^-4 |x| + 2^-10 2^t for x."""
    xd, wd = x.double(), w.double()
    sx = torch.ldexp(torch.ones((), dtype=torch.float64), rule_scale(xd.abs().view(len(xd), -1, 32).amax(2)).int() - 127)
    ex, ew = 2.0 ** -4 * xd.abs() + 2.0 ** -10 * sx.repeat_interleave(32, 1), weight_err(wd)
    y = xd @ wd.t() + b.double()
    return y, xd.abs() @ ew.t() + ex @ wd.abs().t() + ex @ ew.t() + 2.0 ** -8 * y.abs()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ref_quantiser_contract(dtype):
    v = special_blocks().to(dtype)
    q, e = ref.mxfp4_quant(v)
    assert q.dtype == torch.uint8 and q.shape == (7, 16) and e.dtype == torch.uint8 and e.shape == (7, 4)
    assert torch.equal(e[:, 0], rule_scale4(v.float().abs().amax(1))) and bool((e[:, 1:] == 127).all())
    code = torch.stack((q & 15, q >> 4), 2).view(7, 32)            # element k: byte k / 2, even k in the low nibble
    got = GRID[(code & 7).long()] * (1 - 2 * (code >> 3).double())
    assert torch.equal(ref.mxfp4_dequant(q, e, torch.float64), got * 2.0 ** (e[:, :1].double() - 127))
    t = v.double() * 2.0 ** (127 - e[:, :1].double())              # the value the conversion rounds
    dist = (t.abs()[..., None] - GRID).abs()
    best = dist.amin(-1)
    assert torch.equal((got - t).abs(), best), "decoded q is a nearest grid value"
    tie = (dist == best[..., None]).sum(-1) > 1
    assert bool(((code & 1) == 0)[tie].all()), "ties go to the even code"
    assert torch.equal(code >> 3, (v < 0).to(torch.uint8)), "sign << 3, also where the magnitude rounds to zero"
    assert got[0].abs().max() == 0 and e[5, 0] == 125 and got[5, :8].tolist() == [0, -1, 1, -2, 2, -4, 4, -6]
    if dtype == torch.float32:   # t = 0, 1 | E - 2, E - 1 around the mantissa 1.5
        assert e[:5, 0].tolist() == [127, 127, 128, 128, 129] and got[1, 5] == 6 and got[2, 5] == -3 and got[1, 6] == 1
    e = ref.mxfp4_quant(block_scaled(3, 160, torch.Generator().manual_seed(0)).to(dtype))[1]
    assert e.shape == (3, 8) and bool((e[:, 5:] == 127).all()) and e[:, :5].unique().numel() > 2, "K = 160: three pad bytes"


def test_weight_error_bound():
    w = block_scaled(64, 768, torch.Generator().manual_seed(4), 0.05)
    q, e = ref.mxfp4_quant(w)
    ratio = (ref.mxfp4_dequant(q, e, torch.float64) - w.double()).abs() / weight_err(w.double())
    scaled = w.view(64, -1, 32).abs().amax(2) * 2.0 ** (127 - e[:, :24].float())
    assert bool((ratio <= 1).all()) and float(ratio.max()) > 0.9, "the bound holds and is nearly met"
    assert bool((scaled > 3).all() and (scaled <= 6).all()), "the scaled amax lies in (3, 6]"


@pytest.mark.parametrize("M,K,N,act,seed", OUT_MX_CASES)
def test_out_mx_case_conditions(M, K, N, act, seed):
    """test_mxfp8_linear_cpu's condition on this mode's truth (the pair emitted is MXFP8: thresholds at 1.75 * 2^j)."""
    amax = out_mx_case(M, K, N, act, seed)[-1].abs().view(M, N // 32, 32).amax(2)
    f = torch.frexp(amax[amax > 0])[0]
    assert bool(((f - 0.875).abs() > 0.875 * 2.0 ** -10).all())
    assert act != 1 or bool((amax == 0).any())


def test_switch_and_cli_flag(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    assert _lib.infer_matmul() == "bf16" and "mxfp4" in _lib.INFER_MATMUL_MODES
    try:
        assert entry.main(["--preset", "mlp-cpu", "--infer-matmul", "mxfp4", "--json", str(out)]) == 0
        assert _lib.infer_matmul() == "mxfp4"
        assert json.loads(out.read_text().strip().splitlines()[-1])["infer_matmul"] == "mxfp4"
        with pytest.raises(SystemExit, match="--infer-matmul mxfp4 needs --dtype bf16"):
            entry.main(["--preset", "mlp-cpu", "--infer-matmul", "mxfp4", "--dtype", "fp32", "--json", str(out)])
        assert len(out.read_text().strip().splitlines()) == 1
    finally:
        _lib.set_infer_matmul("bf16")
        _lib.set_precision("bf16")


@pytest.mark.parametrize("fin,fout,M", LAYER_CASES)
def test_linear_cpu_paths(fin, fout, M):
    """no_grad + mxfp4 mode: the reference ops composed, bitwise, inside the bound the GPU test uses on the same seeds.
    Grad enabled: the bf16-mode result."""
    lin, x = layer_case(fin, fout, M)
    y_bf16 = lin(x)
    try:
        _lib.set_infer_matmul("mxfp4")
        with torch.no_grad():
            y = lin(x)
            want = ref.linear_mxfp4_fwd(*ref.mxfp8_quant(x), *ref.mxfp4_quant(lin.weight), lin.bias, 0)[0]
            t, bound = quant_bound(x, lin.weight, lin.bias)
        y_grad = lin(x)
    finally:
        _lib.set_infer_matmul("bf16")
    assert y.dtype == torch.bfloat16 and torch.equal(y, want) and not torch.equal(y, y_bf16)
    assert bool(((y.double() - t).abs() <= bound).all())
    assert y_grad.requires_grad and torch.equal(y_grad, y_bf16)
