"""The pooled variant of ``conv_mxfp8_fwd`` (csrc/mxfp8_conv.hip, ``pool=2``) and VGG16's mxfp8 chain on the GPU.  Cases,
truth, conditions and the path check: tests/test_mxfp8_vgg_cpu.py."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import pcmp  # noqa: F401
from pcmp.ops import _lib, truth as T
from pcmp.ops._lib import ops
from test_mxfp8_conv_cpu import K_FWD, check_out_mx
from test_mxfp8_linear_gpu import with_knobs
from test_mxfp8_vgg_cpu import POOL_CASES, POOL_MX_CASES, check_vgg_paths, pool_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pooled_conv_against_fp64(gpu, name, tile):
    """fp64 truth; two runs bitwise equal; bitwise ``max_pool2d`` of the unpooled op's bf16 output (rounding to bf16 is
    monotone, and an element's fp32 sum does not depend on the tile row it sits in)."""
    args, t = pool_case(name, dev=gpu)
    (y,), (y2,), (full,) = with_knobs({"fp8_tile": tile}, lambda: [
        ops().conv_mxfp8_fwd(*args, True, False, pool) for pool in (2, 2, 0)])
    assert y.dtype == torch.bfloat16 and y.shape == t.shape and torch.equal(y, y2), "two runs are bitwise equal"
    worst = T.assert_elementwise(y.cpu().view(-1, y.shape[-1]), t.view(-1, y.shape[-1]), (1,), K_FWD, f"{name} tile {tile}")
    print(f"mxfp8 pooled conv {name} tile {tile}: worst norm_err {worst:.4f}")
    assert torch.equal(y, F.max_pool2d(full.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)), "pool of the unpooled output"


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("name,seed", POOL_MX_CASES)
def test_pooled_pair(gpu, name, seed, tile):
    args, t = pool_case(name, seed, True, gpu)
    (yq, ye), (y,), (y3, yq3, ye3) = with_knobs({"fp8_tile": tile}, lambda: [
        ops().conv_mxfp8_fwd(*args, b, m, 2) for b, m in ((False, True), (True, False), (True, True))])
    assert yq.shape == t.shape
    worst = check_out_mx(yq.cpu(), ye.cpu(), t)
    print(f"mxfp8 pooled conv pair {name} tile {tile}: worst err / bound {worst:.4f}")
    for a, b in ((yq, yq3), (ye, ye3), (y, y3)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_vgg_public_path(gpu):
    out, y_off = check_vgg_paths(gpu, ops())
    lo, hi = y_off.float().aminmax()
    print(f"mxfp8 VGG16 logits vs bf16: max |delta| {float((out.float() - y_off.float()).abs().max()):.4f} over range {float(hi - lo):.4f}")


def test_vgg16_entrypoint(gpu, tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    try:
        rc = entry.main(["--model", "vgg16", "--infer-conv", "mxfp8", "--train-size", "10", "--batch-size", "2", "--epochs", "1",
                         "--num-images", "2", "--json", str(out)])
    finally:
        _lib.set_infer_conv("bf16")
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    h = rec["history"]   # the evaluation pass and the captured batch-1 predictor ran the chain
    assert rc == 0 and rec["infer_conv"] == "mxfp8" and rec["batch1_latency"]["graph"] is True
    assert len(h["test_loss"]) >= 1 and all(math.isfinite(l) for l in h["train_loss"] + h["test_loss"])
