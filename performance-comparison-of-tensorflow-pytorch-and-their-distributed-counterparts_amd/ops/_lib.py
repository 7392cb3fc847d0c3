"""Native library loading and backend selection.

Rule: an op on a GPU tensor runs the hand-written HIP kernel from ``_native/libpcmp_hip.so``
and raises loudly if that library is missing or failed to load (no silent eager fallback);
an op on a CPU tensor runs the PyTorch reference implementation in :mod:`pcmp.ops.ref`
(CPU plumbing config + numerics tests).  ``PCMP_KERNELS=torch`` (or
:func:`set_backend`) forces the reference path on GPU too — used only for A/B parity runs.
"""
from __future__ import annotations

import os
import pathlib
import threading

import torch

_PKG = pathlib.Path(__file__).resolve().parent.parent
# PCMP_LIB: load another build of the library (same-box A/B of compile-time variants, tools/build_variant.py)
LIB_PATH = pathlib.Path(os.environ["PCMP_LIB"]) if os.environ.get("PCMP_LIB") else _PKG / "_native" / "libpcmp_hip.so"

_lock = threading.Lock()
_loaded = False
_load_error: str | None = None
_backend = os.environ.get("PCMP_KERNELS", "hip").lower()
_compute_dtype: torch.dtype | None = None   # None: bf16 on the GPU, fp32 on the CPU
_f32_matmul = "exact"                       # set_f32_matmul
_infer_matmul = "bf16"                      # set_infer_matmul
_infer_conv = "bf16"                        # set_infer_conv
_infer_attn = "bf16"                        # set_infer_attn
_train_matmul = "bf16"                      # set_train_matmul


def load(build_if_missing: bool = False) -> bool:
    """Load the native op library into ``torch.ops.pcmp``.  Returns True on success."""
    global _loaded, _load_error
    if _loaded:
        return True
    with _lock:
        if _loaded:
            return True
        if not LIB_PATH.exists() and build_if_missing:
            from .. import _build
            _build.build(verbose=False)
        if not LIB_PATH.exists():
            _load_error = f"{LIB_PATH} not built (run __graft_entry__.build() or pcmp._build.build())"
            return False
        try:
            torch.ops.load_library(str(LIB_PATH))
            _loaded = True
            _load_error = None
        except Exception as e:  # pragma: no cover - depends on the environment
            _load_error = f"failed to load {LIB_PATH}: {e}"
        if _loaded:
            if _f32_matmul != "exact":   # chosen before the library was loaded
                torch.ops.pcmp.set_knob("f32_bf16x", F32_MATMUL_MODES[_f32_matmul])
            _apply_env_knobs()
        return _loaded


def _apply_env_knobs() -> None:
    """``PCMP_KNOBS="name=value,..."``: kernel-variant knobs (torch.ops.pcmp.set_knob) for whole-
    program A/B runs; the defaults are the measured-best variants."""
    spec = os.environ.get("PCMP_KNOBS", "")
    for item in filter(None, (t.strip() for t in spec.split(","))):
        name, _, val = item.partition("=")
        torch.ops.pcmp.set_knob(name.strip(), int(val))


def available() -> bool:
    return load()


def load_error() -> str | None:
    return _load_error


def set_backend(name: str) -> None:
    """'hip' (default) or 'torch' (reference ops on every device)."""
    global _backend
    assert name in ("hip", "torch"), name
    _backend = name


def backend() -> str:
    return _backend


def set_precision(name: str) -> None:
    """``--dtype``: 'bf16' (default; bf16 storage with fp32 accumulation) or 'fp32' (the
    reference's precision, SURVEY §0.1 / §5.6: another_neural_net.py:95-115 and nb :655-702 run
    fp32 everywhere).  Both stay on the HIP kernels: fp32 activations select the fp32 kernels of
    ``csrc/f32.hip`` (convolutions / Linear on v_mfma_f32_16x16x4_f32, BatchNorm, pooling, dropout,
    losses) and ``csrc/text_f32.hip`` (LayerNorm, attention, GELU / tanh, embedding, masked mean,
    the BiLSTM recurrence, Linear+GELU): no op falls back to PyTorch (``kernels.FP32_REF_OPS`` is
    empty)."""
    global _compute_dtype
    assert name in ("bf16", "fp32"), name
    _compute_dtype = torch.float32 if name == "fp32" else None


def precision() -> str:
    return "fp32" if _compute_dtype == torch.float32 else "bf16"


F32_MATMUL_MODES = {"exact": 0, "bf16x6": 6, "bf16x3": 3}   # name -> knob f32_bf16x


def set_f32_matmul(name: str) -> None:
    """``--f32-matmul``: how the fp32 convolutions and Linear layers form their products on the GPU.
    'exact' (default): the f32 MFMA kernels, an exact fp32 fma chain.  'bf16x6' / 'bf16x3': each fp32
    operand is split into three / two bf16 parts and the product is the sum of six / three bf16 MFMA
    products accumulated in fp32 (``csrc/f32_bf16x.h``; fp32-level and 2^-17-class accuracy,
    docs/PARITY.md).  Shapes the split kernel does not take, the fp32 attention and every other fp32
    kernel stay exact.  The mode is a knob of the native library (``f32_bf16x``), set here when the
    library is loaded and otherwise when it loads; on the CPU reference path it is only recorded:
    ``ops/ref.py`` stays exact fp32."""
    global _f32_matmul
    if name not in F32_MATMUL_MODES:
        raise ValueError(f"f32 matmul mode {name!r}: one of {sorted(F32_MATMUL_MODES)}")
    _f32_matmul = name
    if _loaded:
        torch.ops.pcmp.set_knob("f32_bf16x", F32_MATMUL_MODES[name])


def f32_matmul() -> str:
    return _f32_matmul


INFER_MATMUL_MODES = ("bf16", "fp8", "mxfp8", "mxfp4")


def set_infer_matmul(name: str) -> None:
    """``--infer-matmul``: how bf16 ``Linear`` layers multiply under ``torch.no_grad()``.  'bf16' (default):
    the bf16 MFMA kernels, as in training.  'fp8': activations are quantised per token and the fp32 master
    weights per output channel to OCP E4M3 (``fp8_quant_rows``) and the product runs on the fp8 MFMA
    (``linear_fp8_fwd``, ``csrc/fp8.hip``; contract and errors in docs/PARITY.md).  Training (grad enabled),
    convolutions, the fp32 precision and layers whose shape the fp8 kernels do not take (K % 16 != 0 or
    N % 8 != 0) are untouched.  'mxfp8': E4M3 elements with one power-of-two scale per 32 consecutive K
    elements (``mxfp8_quant``), multiplied on the block-scaled MFMA (``linear_mxfp8_fwd``, ``csrc/mxfp8.hip``);
    same scope, layers with K % 32 != 0 or N % 8 != 0 stay on bf16.  'mxfp4': the mxfp8 mode with the weights in
    OCP MXFP4 (E2M1 elements, two per byte, one power-of-two scale per 32; ``mxfp4_quant``) against the same
    MXFP8 activations (``linear_mxfp4_fwd``, ``csrc/mxfp4.hip``): half the weight bytes, a relative rms weight
    error of about 0.12.  The mode lives in Python (``ops/functions.py: linear`` reads it); the CPU
    reference path honours it through ``ops/ref.py``."""
    global _infer_matmul
    if name not in INFER_MATMUL_MODES:
        raise ValueError(f"inference matmul mode {name!r}: one of {sorted(INFER_MATMUL_MODES)}")
    _infer_matmul = name


def infer_matmul() -> str:
    return _infer_matmul


TRAIN_MATMUL_MODES = ("bf16", "fp8", "mxfp8")


def set_train_matmul(name: str) -> None:
    """``--train-matmul``: how bf16 ``Linear`` layers multiply when grad is enabled.  'bf16' (default): the bf16
    MFMA kernels.  'fp8': all three GEMMs of a layer run on the fp8 MFMA (``ops/functions.py: LinearFp8TrainFn``;
    ``csrc/fp8.hip``, ``csrc/fp8_train.hip``; contract and errors in docs/PARITY.md): the forward on E4M3 ``x`` (one
    scale per token) and E4M3 ``W`` (one per output channel), DGRAD on E5M2 ``dy`` (per token) and E4M3 ``W^T``
    (per input channel), WGRAD on E5M2 ``dy^T`` and E4M3 ``x^T`` (per column of ``dy`` and of ``x``) into the fp32
    gradient.  A call takes the path when ``x`` is 2-D bf16 and M, K and N are multiples of 16 above 16; every
    other call, the fp32 precision and the convolutions are untouched.  'mxfp8': all three GEMMs run on the
    block-scaled MFMA with E4M3 elements and one E8M0 scale per 32 elements of the reduction, gradients included
    (``LinearMxfp8TrainFn``; ``csrc/mxfp8_train.hip``, ``csrc/mxfp8.hip``): ``mxfp8_quant_both`` writes the row and
    the transposed column image of ``x`` and of ``dy`` in one launch each, the forward and DGRAD are
    ``linear_mxfp8_fwd`` and WGRAD is ``linear_mxfp8_wgrad``; a call takes the path when ``x`` is 2-D bf16 and M, K
    and N are multiples of 32.  Independent of :func:`set_infer_matmul`, which governs calls under
    ``torch.no_grad()``."""
    global _train_matmul
    if name not in TRAIN_MATMUL_MODES:
        raise ValueError(f"training matmul mode {name!r}: one of {sorted(TRAIN_MATMUL_MODES)}")
    _train_matmul = name


def train_matmul() -> str:
    return _train_matmul


INFER_CONV_MODES = ("bf16", "mxfp8")


def set_infer_conv(name: str) -> None:
    """``--infer-conv``: how the convolutions of bf16 residual blocks run in eval mode under ``torch.no_grad()``.
    'bf16' (default): the bf16 implicit-GEMM kernels.  'mxfp8': every block conv with ``C % 32 == 0`` runs
    ``conv_mxfp8_fwd`` (``csrc/mxfp8_conv.hip``) on block-scaled E4M3 operands; the activation is quantised once,
    behind the stem, and from then on each conv's epilogue emits the next conv's operand, so no quantiser runs
    inside or between blocks (``ops/conv_blocks.py: _block_eval_mx``; contract and errors in docs/PARITY.md).
    VGG16's features take the same chain behind layer 0, the ``MaxPool2d(2, 2)`` behind a conv fused into that conv's
    epilogue (``models/vgg.py: VGG._features_mx``).  Independent of :func:`set_infer_matmul`, which governs the head.
    Training, grad-enabled calls, the stems and the fp32 precision are untouched."""
    global _infer_conv
    if name not in INFER_CONV_MODES:
        raise ValueError(f"inference conv mode {name!r}: one of {sorted(INFER_CONV_MODES)}")
    _infer_conv = name


def infer_conv() -> str:
    return _infer_conv


INFER_ATTN_MODES = ("bf16", "mxfp8")


def set_infer_attn(name: str) -> None:
    """``--infer-attn``: how a BERT layer runs its attention under ``torch.no_grad()`` next to a block-scaled
    :func:`set_infer_matmul` mode ('mxfp8' or 'mxfp4').  'bf16' (default): the QKV GEMM writes bf16, the bf16 attention
    kernels run on it, and a quantiser runs before ``attn_out``, ``ffn1`` and the next layer's ``qkv``.  'mxfp8': the
    layer never leaves the format (``models/bert.py: BertLayer.forward_mx``): the QKV GEMM emits the ``(e4m3, E8M0)``
    pair, ``attention_mx_fwd`` (``csrc/attn_mx.hip``) consumes it and emits the context as a pair, and both LayerNorms
    emit the pair of their bf16 row (``layernorm_fwd`` with ``out_mx``), so one ``mxfp8_quant`` runs per forward
    (contract and errors in docs/PARITY.md).  Padded batches with ``S % 32 == 0``, ``S <= 512`` and more than 16 rows;
    every other call, packed batches and the other matmul modes keep today's layer."""
    global _infer_attn
    if name not in INFER_ATTN_MODES:
        raise ValueError(f"inference attention mode {name!r}: one of {sorted(INFER_ATTN_MODES)}")
    _infer_attn = name


def infer_attn() -> str:
    return _infer_attn


def default_compute_dtype(device: torch.device) -> torch.dtype:
    """Activation dtype of a model on ``device`` unless the model was given one explicitly."""
    if _compute_dtype is not None:
        return _compute_dtype
    return torch.bfloat16 if device.type == "cuda" else torch.float32


def use_native(t: torch.Tensor) -> bool:
    """True if ops on ``t`` must run the HIP kernels.  Raises if they are required but absent."""
    if not t.is_cuda or _backend == "torch":
        return False
    if not load():
        raise RuntimeError(
            "pcmp: GPU tensor given but the native HIP library is unavailable: "
            f"{_load_error}.  Refusing to fall back silently (set PCMP_KERNELS=torch to use the "
            "PyTorch reference path deliberately).")
    return True


def ops():
    load()
    return torch.ops.pcmp
