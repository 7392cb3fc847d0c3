"""Autograd Functions for the dense / loss / regularisation ops (Linear as a 1x1 implicit-GEMM
conv, Dropout with a counter-based RNG, fused softmax cross-entropy, log-softmax).

Reference parity: the transfer heads ``Linear(2048,512)-ReLU-Dropout(0.2)-Linear(512,10)-
LogSoftmax`` / ``Linear(4096,256)-ReLU-Dropout(0.4)-Linear(256,10)-LogSoftmax`` with
``NLLLoss`` (another_neural_net.py:108-113,250-257), VGG16 classifier FCs with Dropout(0.5)
and the BERT pooler/classifier (pytorch_on_language_distr.py:151-161).
"""
from __future__ import annotations

import itertools

import torch

from . import _lib
from .kernels import K
from .params import (compute_weight, compute_weight_t, emit_grad, fp8_weight, fp8_weight_t, mxfp4_weight, mxfp8_weight,
                     mxfp8_weight_t)


class _RNG:
    """Dropout seed/offset stream: deterministic given ``torch.initial_seed()``.

    ``salt`` (set by :class:`pcmp.engine.graph.GraphedStep` while it captures a training step) is
    a device int64 counter that the dropout / attention kernels mix into the seed; the captured step
    increments it, so every replay of the graph draws new masks although the kernels' arguments
    are frozen at capture time.  Eager steps leave it None."""

    def __init__(self):
        self.seed = None
        self.counter = itertools.count()
        self.salt = None

    def next(self, n: int):
        if self.seed is None:
            self.seed = int(torch.initial_seed()) & ((1 << 62) - 1)
        off = next(self.counter) << 32
        return self.seed, off

    def reseed(self, seed: int):
        self.seed = int(seed) & ((1 << 62) - 1)
        self.counter = itertools.count()


dropout_rng = _RNG()


class LinearFn(torch.autograd.Function):
    """y = act(x @ W^T + b), x [M, Cin] (compute dtype), W [Nout, Cin] fp32 master."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        M, Cin = x.shape
        Nout = weight.shape[0]
        w = compute_weight(weight, x.dtype)
        b = bias.detach().float() if bias is not None else None

        # a plain GEMM on the MFMA kernels: torch.ops.pcmp.conv_fwd plans the kernel / K-split per
        # shape (csrc/igemm.hip plan_gemm); bias and ReLU are fused into the epilogue
        y = K.conv_fwd(x.reshape(M, 1, 1, Cin), w.reshape(Nout, 1, 1, Cin), 1, 0, b, None, relu,
                       False)[0].reshape(M, Nout)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, y)
            ctx.weight, ctx.bias, ctx.relu = weight, bias, relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        if ctx.relu:
            dy = K.relu_bwd(dy, y)
        M, Cin = x.shape
        Nout = weight.shape[0]
        dy4 = dy.reshape(M, 1, 1, Nout)
        x4 = x.reshape(M, 1, 1, Cin)
        gw = emit_grad(weight, lambda out, acc: K.conv_wgrad(dy4, x4, out, 1, 1, 1, 0, acc))
        gb = emit_grad(bias, lambda out, acc: K.colsum(dy, out, acc)) if bias is not None else None
        dx = None
        if ctx.needs_input_grad[0]:
            w = compute_weight(weight, dy.dtype)
            dx = K.conv_dgrad(dy4, w.reshape(Nout, 1, 1, Cin), 1, 1, 1, 0, None,
                              compute_weight_t(weight, dy.dtype)).reshape(M, Cin)
        return dx, gw, gb, None


class LinearFp8TrainFn(torch.autograd.Function):
    """``LinearFn`` with its three GEMMs on the fp8 MFMA (``set_train_matmul("fp8")``; contract in docs/PARITY.md):
    forward on E4M3 ``x`` (a scale per token) and the cached E4M3 ``W`` (per output channel); DGRAD on E5M2 ``dy``
    (per token) and the cached E4M3 ``W^T`` (per input channel); WGRAD on E5M2 ``dy^T`` and E4M3 ``x^T`` (per
    column of ``dy`` and of ``x``) into the fp32 gradient or its ``main_grad`` sink.  ``x`` is saved in bf16 and
    quantised by columns in the backward; ``dy`` is read twice, by one amax sweep and one convert sweep that
    write both of its images.  The bias gradient and the ReLU mask are the bf16 ops of ``LinearFn``."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        x = x.contiguous()
        xq, sx = K.fp8_quant_rows(x)
        wq, sw = fp8_weight(weight)
        b = bias.detach().float() if bias is not None else None
        y = K.linear_fp8_fwd(xq, sx, wq, sw, b, 1 if relu else 0)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, y if relu else None)
            ctx.weight, ctx.bias, ctx.relu = weight, bias, relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        if ctx.relu:
            dy = K.relu_bwd(dy, y)
        dyq, sdy, dytq, sn = K.fp8_quant_both(dy, 1)
        gw = None
        if weight.requires_grad:
            xtq, sk = K.fp8_quant_cols(x, 0)
            gw = emit_grad(weight, lambda out, acc: K.linear_fp8_wgrad(dytq, sn, xtq, sk, out, acc))
        gb = emit_grad(bias, lambda out, acc: K.colsum(dy, out, acc)) if bias is not None else None
        dx = K.linear_fp8_dgrad(dyq, sdy, *fp8_weight_t(weight)) if ctx.needs_input_grad[0] else None
        return dx, gw, gb, None


class LinearMxfp8TrainFn(torch.autograd.Function):
    """``LinearFn`` with its three GEMMs on the block-scaled MFMA (``set_train_matmul("mxfp8")``; contract in
    docs/PARITY.md): E4M3 elements with one E8M0 scale per 32 elements of each GEMM's reduction, the output gradient
    included.  ``mxfp8_quant_both`` makes the row image and the transposed column image of a tensor in one launch:
    of ``x`` in the forward (the row image feeds ``linear_mxfp8_fwd``, the column image is saved for WGRAD in place
    of bf16 ``x``) and of ``dy`` in the backward (rows for DGRAD, which is ``linear_mxfp8_fwd`` on the cached ``W^T``
    image, columns for ``linear_mxfp8_wgrad``).  The bias gradient and the ReLU mask are the bf16 ops of ``LinearFn``."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        xq, ex, xtq, ext = K.mxfp8_quant_both(x.contiguous())
        mxfp8_weight_t(weight)                      # a cache miss quantises W once, into this and mxfp8_weight's cache
        wq, ew = mxfp8_weight(weight)
        b = bias.detach().float() if bias is not None else None
        y = K.linear_mxfp8_fwd(xq, ex, wq, ew, b, 1 if relu else 0, False)[0]
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xtq, ext, y if relu else None)
            ctx.weight, ctx.bias, ctx.relu = weight, bias, relu
        return y

    @staticmethod
    def backward(ctx, dy):
        xtq, ext, y = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy = dy.contiguous()
        if dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        if ctx.relu:
            dy = K.relu_bwd(dy, y)
        dyq, edy, dytq, edyt = K.mxfp8_quant_both(dy)
        gw = emit_grad(weight, lambda out, acc: K.linear_mxfp8_wgrad(dytq, edyt, xtq, ext, out, acc))
        gb = emit_grad(bias, lambda out, acc: K.colsum(dy, out, acc)) if bias is not None else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.linear_mxfp8_fwd(dyq, edy, *mxfp8_weight_t(weight), None, 0, False)[0]
        return dx, gw, gb, None


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        seed, off = dropout_rng.next(x.numel())
        ctx.cfg = (p, seed, off, dropout_rng.salt)
        return K.dropout(x.contiguous(), p, seed, off, dropout_rng.salt)

    @staticmethod
    def backward(ctx, dy):
        p, seed, off, salt = ctx.cfg
        return K.dropout(dy.contiguous(), p, seed, off, salt), None


class SoftmaxXentFn(torch.autograd.Function):
    """mean over valid rows of -log_softmax(z)[y]  (== LogSoftmax + NLLLoss)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        need = ctx.needs_input_grad[0]
        logits = logits.contiguous()
        r = K.softmax_xent(logits, labels, False, need, 1.0, ignore_index)
        lm = K.loss_mean(r[0], labels.contiguous(), logits.shape[1], ignore_index)   # [mean, valid rows]
        if need:
            ctx.save_for_backward(r[1], lm)
        return lm[0]

    @staticmethod
    def backward(ctx, gout):
        dl, lm = ctx.saved_tensors
        return K.xent_grad_scale(dl, gout.reshape(1).to(torch.float32).contiguous(), lm[1:2]), None, None


class LogSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        r = K.softmax_xent(z.contiguous(), None, True, False, 1.0, -100)
        logp = r[1]
        ctx.save_for_backward(logp)
        ctx.dtype = z.dtype
        return logp

    @staticmethod
    def backward(ctx, g):
        (logp,) = ctx.saved_tensors
        # the g - exp(logp) * sum(g) math runs at g's precision (fp32 from an fp32 NLL); only the
        # result is cast to the activation dtype
        if g.dtype != ctx.dtype and g.dtype != torch.float32:
            g = g.float()
        dz = K.log_softmax_bwd(g.contiguous(), logp)
        return dz if dz.dtype == ctx.dtype else dz.to(ctx.dtype)


def fp8_infer(x, weight) -> bool:
    """True when ``linear`` takes the fp8 inference path for this call: ``set_infer_matmul("fp8")``, grad
    disabled, bf16 activations, and a shape the fp8 kernels take (K % 16 == 0, N % 8 == 0)."""
    return (_lib.infer_matmul() == "fp8" and not torch.is_grad_enabled() and x.dtype == torch.bfloat16
            and x.dim() == 2 and x.shape[1] % 16 == 0 and weight.shape[0] % 8 == 0)


def linear_fp8(x, weight, bias, act):
    """act(x @ W^T + b) on the fp8 MFMA (act 0 none, 1 ReLU, 2 erf-GELU): x quantised per token, the cached
    per-channel quantisation of the fp32 master weight, one GEMM with the scales, bias and act in its
    epilogue.  No host synchronisation: capturable once the weight cache is warm."""
    xq, sx = K.fp8_quant_rows(x.contiguous())
    wq, sw = fp8_weight(weight)
    b = bias.detach().float() if bias is not None else None
    return K.linear_fp8_fwd(xq, sx, wq, sw, b, act)


def fp8_train(x, weight) -> bool:
    """True when ``linear`` takes the fp8 training path for this call: ``set_train_matmul("fp8")``, grad enabled,
    2-D bf16 activations, and M, K, N all multiples of 16 above 16 (each is the reduction of one of the three
    GEMMs, and the tiled kernel takes more than 16 rows)."""
    return (_lib.train_matmul() == "fp8" and torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 2
            and all(d % 16 == 0 and d > 16 for d in (x.shape[0], x.shape[1], weight.shape[0])))


def mxfp8_train(x, weight) -> bool:
    """True when ``linear`` takes the mxfp8 training path for this call: ``set_train_matmul("mxfp8")``, grad
    enabled, 2-D bf16 activations, and M, K, N all multiples of 32 (each is the reduction of one of the three GEMMs,
    cut into blocks of 32)."""
    return (_lib.train_matmul() == "mxfp8" and torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 2
            and all(d > 0 and d % 32 == 0 for d in (x.shape[0], x.shape[1], weight.shape[0])))


def mxfp8_infer(x, weight) -> bool:
    """True when ``linear`` takes a block-scaled inference path for this call: ``set_infer_matmul("mxfp8")`` or
    ``("mxfp4")`` (the same MXFP8 activations against MXFP4 weights), grad disabled, bf16 activations, and a shape
    the kernels take (K % 32 == 0, N % 8 == 0)."""
    return (_lib.infer_matmul() in ("mxfp8", "mxfp4") and not torch.is_grad_enabled() and x.dtype == torch.bfloat16
            and x.dim() == 2 and x.shape[1] % 32 == 0 and weight.shape[0] % 8 == 0)


def mxfp8_chain(M, w1, w2) -> bool:
    """True when the Linear ``w1`` on M rows can hand its output to the Linear ``w2`` as a quantised pair
    (``out_mx``): the tiled kernel (M > 16), whole 32-channel blocks, no padded channels in between."""
    return M > 16 and w1.shape[0] % 32 == 0 and w2.shape[1] == w1.shape[0] and w2.shape[0] % 8 == 0


def linear_mxfp8(x, weight, bias, act, out_mx=False):
    """act(x @ W^T + b) on the block-scaled fp8 MFMA (act 0 none, 1 ReLU, 2 erf-GELU).  ``x`` is a bf16 tensor,
    quantised here, or an already quantised ``(q, e)`` pair.  ``out_mx``: the result stays in the format, a
    ``(yq, ye)`` pair quantised from the fp32 epilogue value, for the next ``linear_mxfp8`` to consume.  In the
    mxfp4 mode the weight operand is MXFP4 (``linear_mxfp4_fwd``); the activation format, and so the pair handed
    on, is the same."""
    xq, ex = x if isinstance(x, tuple) else K.mxfp8_quant(x.contiguous())
    b = bias.detach().float() if bias is not None else None
    if _lib.infer_matmul() == "mxfp4":
        r = K.linear_mxfp4_fwd(xq, ex, *mxfp4_weight(weight), b, act, out_mx)
    else:
        r = K.linear_mxfp8_fwd(xq, ex, *mxfp8_weight(weight), b, act, out_mx)
    return (r[0], r[1]) if out_mx else r[0]


def linear(x, weight, bias=None, relu=False):
    mode = _lib.infer_matmul()
    if mode != "bf16":   # mode test first: the default path pays one compare
        if mode == "fp8" and fp8_infer(x, weight):
            return linear_fp8(x, weight, bias, 1 if relu else 0)
        if mode in ("mxfp8", "mxfp4") and mxfp8_infer(x, weight):
            return linear_mxfp8(x, weight, bias, 1 if relu else 0)
    if _lib.train_matmul() != "bf16":
        if fp8_train(x, weight):
            return LinearFp8TrainFn.apply(x, weight, bias, relu)
        if mxfp8_train(x, weight):
            return LinearMxfp8TrainFn.apply(x, weight, bias, relu)
    return LinearFn.apply(x, weight, bias, relu)


def dropout(x, p, training=True):
    if not training or p == 0.0:
        return x
    return DropoutFn.apply(x, p)


def cross_entropy(logits, labels, ignore_index=-100):
    return SoftmaxXentFn.apply(logits, labels, ignore_index)


def log_softmax(z):
    return LogSoftmaxFn.apply(z)
