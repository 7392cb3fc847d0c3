"""The mxfp8 inference conv mode on the GPU (csrc/mxfp8_conv.hip): ``conv_mxfp8_fwd`` against fp64, the ``out_mx`` epilogue,
the residual blocks' chain, one entry-point run.  Cases, truth and conditions: tests/test_mxfp8_conv_cpu.py."""
import json
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, truth as T
from pcmp.ops._lib import ops
from test_mxfp8_conv_cpu import CONV_CASES, K_FWD, OUT_MX_CASES, check_block_paths, check_out_mx, conv_case
from test_mxfp8_linear_gpu import with_knobs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_against_fp64(gpu, name, tile):
    args, t = conv_case(name, dev=gpu)
    (y,), (y2,) = with_knobs({"fp8_tile": tile}, lambda: [ops().conv_mxfp8_fwd(*args, True, False) for _ in range(2)])
    assert y.dtype == torch.bfloat16 and y.shape == t.shape and torch.equal(y, y2), "two runs are bitwise equal"
    worst = T.assert_elementwise(y.cpu().view(-1, y.shape[-1]), t.view(-1, y.shape[-1]), (1,), K_FWD, f"{name} tile {tile}")
    print(f"mxfp8 conv {name} tile {tile}: worst norm_err {worst:.4f}")


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("name,cout,seed", OUT_MX_CASES)
def test_out_mx_epilogue(gpu, name, cout, seed, tile):
    args, t = conv_case(name, cout, seed, True, gpu)
    (yq, ye), (y,), (y3, yq3, ye3), (yq2, ye2) = with_knobs({"fp8_tile": tile}, lambda: [
        ops().conv_mxfp8_fwd(*args, b, m) for b, m in ((False, True), (True, False), (True, True), (False, True))])
    assert yq.shape == t.shape and bool((t.abs().view(-1, cout // 32, 32).amax(2) == 0).any())
    worst = check_out_mx(yq.cpu(), ye.cpu(), t)
    print(f"mxfp8 conv out_mx {name} tile {tile}: worst err / bound {worst:.4f}")
    for a, b in ((yq, yq2), (ye, ye2), (yq, yq3), (ye, ye3), (y, y3)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_block_public_path(gpu, kind):
    check_block_paths(kind, gpu, ops())


def test_resnet18_entrypoint(gpu, tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    try:
        rc = entry.main(["--model", "resnet18", "--full-train", "--infer-conv", "mxfp8", "--image-size", "64", "--train-size",
                         "40", "--batch-size", "8", "--epochs", "1", "--lr", "0.01", "--num-images", "4", "--json", str(out)])
    finally:
        _lib.set_infer_conv("bf16")
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    h = rec["history"]   # the evaluation pass and the captured batch-1 predictor ran the chain
    assert rc == 0 and rec["infer_conv"] == "mxfp8" and rec["batch1_latency"]["graph"] is True
    assert len(h["test_loss"]) >= 1 and all(math.isfinite(l) for l in h["train_loss"] + h["test_loss"])
