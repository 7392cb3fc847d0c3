"""Parameter plumbing shared by every autograd Function of the framework.

* **Compute weights.**  Parameters are fp32 masters.  Kernels consume a compute-dtype copy
  (bf16 on the GPU).  When the model's parameters are flattened (:class:`pcmp.utils.flat.FlatParams`),
  ``p._shadow`` is a view into one contiguous bf16 buffer that the fused optimizer kernel
  rewrites in the same pass as the fp32 update; otherwise the copy is cached per ``p._version``.

* **Gradient sinks.**  With flattened parameters each parameter carries ``p.main_grad``, an fp32
  view into the flat gradient buffer (whose slices are the DDP all-reduce buckets).  Backward
  kernels write weight gradients straight into that view (overwrite on the first write of a
  step, accumulate afterwards) and then fire ``p._grad_ready_hook`` so the data-parallel
  engine can launch the bucket's all-reduce while the rest of backward runs.  Without a sink
  the gradient is returned to autograd as usual.
"""
from __future__ import annotations

import os
from typing import Callable

import torch

# Global weight generation: bumped whenever parameters or BN running statistics change through a
# path that does not touch the tensors' version counters (fused optimizer kernels, BN-statistics
# updates inside training forwards).  Derived caches (inference BN folding) key on it.
WEIGHT_GEN = [0]


def bump_weight_gen():
    WEIGHT_GEN[0] += 1


def compute_weight(p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    sh = getattr(p, "_shadow", None)
    if sh is not None and sh.dtype == dtype:
        return sh
    if p.dtype == dtype:
        return p.detach()
    cache = getattr(p, "_shadow_cache", None)
    if cache is None or cache[0] != p._version or cache[1].dtype != dtype or cache[1].device != p.device:
        cache = (p._version, p.detach().to(dtype).contiguous())
        p._shadow_cache = cache
    return cache[1]


def fp8_weight(p: torch.Tensor):
    """``(wq, sw)``: the E4M3 rows and per-output-channel scales of a Linear weight for the fp8 inference
    mode, quantised from the fp32 master (not the bf16 shadow) and cached on the parameter.  The key holds
    the tensor version and ``WEIGHT_GEN``: the fused optimizers rewrite weights without touching version
    counters."""
    key = (p._version, WEIGHT_GEN[0], p.device)
    cache = getattr(p, "_fp8_cache", None)
    if cache is None or cache[0] != key:
        from .kernels import K
        q, s = K.fp8_quant_rows(p.detach().contiguous())
        cache = p._fp8_cache = (key, q, s)
    return cache[1], cache[2]


def fp8_weight_t(p: torch.Tensor):
    """``(wtq, swt)``: the transposed E4M3 image ``[K, N]`` of a Linear weight with one scale per input channel
    k (``fp8_quant_cols``), the DGRAD operand of the fp8 training mode; from the fp32 master, cached on the
    parameter under the key of :func:`fp8_weight`."""
    key = (p._version, WEIGHT_GEN[0], p.device)
    cache = getattr(p, "_fp8_t_cache", None)
    if cache is None or cache[0] != key:
        from .kernels import K
        q, s = K.fp8_quant_cols(p.detach().contiguous())
        cache = p._fp8_t_cache = (key, q, s)
    return cache[1], cache[2]


def mxfp8_weight(p: torch.Tensor):
    """``(wq, ew)``: the block-scaled E4M3 form of a Linear weight for the mxfp8 inference mode, quantised from
    the fp32 master and cached on the parameter under the key of :func:`fp8_weight`."""
    key = (p._version, WEIGHT_GEN[0], p.device)
    cache = getattr(p, "_mxfp8_cache", None)
    if cache is None or cache[0] != key:
        from .kernels import K
        q, e = K.mxfp8_quant(p.detach().contiguous())
        cache = p._mxfp8_cache = (key, q, e)
    return cache[1], cache[2]


def mxfp8_weight_t(p: torch.Tensor):
    """``(wtq, ewt)``: the transposed block-scaled E4M3 image ``[K, N]`` of a Linear weight, blocks of 32 output
    channels of one input channel, the DGRAD operand of the mxfp8 training mode; from the fp32 master, cached on the
    parameter under the key of :func:`fp8_weight`.  One ``mxfp8_quant_both`` call makes it together with the row
    image, which is ``mxfp8_quant``'s bit for bit and goes into :func:`mxfp8_weight`'s cache."""
    key = (p._version, WEIGHT_GEN[0], p.device)
    cache = getattr(p, "_mxfp8_t_cache", None)
    if cache is None or cache[0] != key:
        from .kernels import K
        q, e, qt, et = K.mxfp8_quant_both(p.detach().contiguous())
        p._mxfp8_cache = (key, q, e)
        cache = p._mxfp8_t_cache = (key, qt, et)
    return cache[1], cache[2]


def mxfp4_weight(p: torch.Tensor):
    """``(wq4, ew)``: the MXFP4 form (E2M1 nibbles ``[N, K / 2]``, E8M0 block scales) of a Linear weight for the
    mxfp4 inference mode, quantised from the fp32 master and cached on the parameter under the key of
    :func:`fp8_weight`."""
    key = (p._version, WEIGHT_GEN[0], p.device)
    cache = getattr(p, "_mxfp4_cache", None)
    if cache is None or cache[0] != key:
        from .kernels import K
        q, e = K.mxfp4_quant(p.detach().contiguous())
        cache = p._mxfp4_cache = (key, q, e)
    return cache[1], cache[2]


def mxfp8_conv_weight(L):
    """``(wq, ew, bias)`` of a conv + BN layer for the mxfp8 inference conv mode: the BN-folded fp32 weight
    ``weight * scale`` (never rounded to bf16) as ``wq [Cout, R, S, C]`` E4M3 with ``ew [Cout*R*S, 4*ceil(C/128)]``,
    one MX row per (output channel, tap), and the fp32 shift as the bias.  Cached on the layer under the key of the
    bf16 fold (``conv_blocks._folded``): ``WEIGHT_GEN`` and the version counters of the weight and the BN tensors.
    A ``layers.Conv2d`` (VGG: bias, no BN) has nothing to fold: its fp32 master weight in the same form and its fp32
    bias (None without one), cached under ``WEIGHT_GEN`` and the versions of the two tensors."""
    f = getattr(L, "_fold_mx", None)
    if not hasattr(L, "gamma"):
        b = L.bias
        key = (WEIGHT_GEN[0], L.weight._version, None if b is None else b._version, L.weight.device)
        if f is None or f[0] != key:
            from .kernels import K
            w = L.weight.detach().float().contiguous()
            q, e = K.mxfp8_quant(w.view(-1, w.shape[-1]))
            f = L._fold_mx = (key, q.view(w.shape), e, None if b is None else b.detach().float().contiguous())
        return f[1], f[2], f[3]
    key = (WEIGHT_GEN[0], L.weight._version, L.gamma._version, L.beta._version, L.running_mean._version,
           L.running_var._version, L.weight.device)
    if f is None or f[0] != key:
        from .kernels import K
        scale, shift = K.bn_eval_coeff(L.gamma.detach(), L.beta.detach(), L.running_mean, L.running_var, L.eps)
        w = (L.weight.detach().float() * scale.view(-1, 1, 1, 1)).contiguous()
        q, e = K.mxfp8_quant(w.view(-1, w.shape[-1]))
        f = L._fold_mx = (key, q.view(w.shape), e, shift.float().contiguous())
    return f[1], f[2], f[3]


def compute_weight_t(p: torch.Tensor, dtype: torch.dtype):
    """Transposed [C,R,S,K] compute weight for DGRAD from the flat arena, or None (the kernel
    then transposes per call)."""
    owner = getattr(p, "_flat_owner", None)
    if owner is None or dtype != torch.bfloat16:
        return None
    from . import _lib
    if _lib.backend() == "torch":
        return None    # the reference backend computes DGRAD from w; the arena's class-blocked form is HIP-only
    return owner.transposed(p)


def emit_grad(p: torch.Tensor | None, compute: Callable[[torch.Tensor, bool], None]):
    """Produce the gradient of ``p``.  ``compute(out, accumulate)`` fills an fp32 tensor.

    Returns the tensor to hand back to autograd, or None when it went into a sink.
    """
    if p is None or not p.requires_grad:
        return None
    mg = getattr(p, "main_grad", None)
    if mg is not None:
        fresh = getattr(p, "_grad_fresh", True)
        compute(mg, not fresh)
        p._grad_fresh = False
        hook = getattr(p, "_grad_ready_hook", None)
        if hook is not None:
            hook(p)
        return None
    out = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    compute(out, False)
    return out if p.dtype == torch.float32 else out.to(p.dtype)


def needs_grad(p) -> bool:
    return p is not None and isinstance(p, torch.Tensor) and p.requires_grad


def sink_or_temp(p: torch.Tensor | None):
    """For kernels that write a small gradient (BN gamma/beta) directly: returns
    (out_tensor_or_None, accumulate, finish) where ``finish()`` returns the autograd value."""
    if p is None or not p.requires_grad:
        return None, False, (lambda: None)
    mg = getattr(p, "main_grad", None)
    if mg is not None:
        acc = not getattr(p, "_grad_fresh", True)

        def finish():
            p._grad_fresh = False
            hook = getattr(p, "_grad_ready_hook", None)
            if hook is not None:
                hook(p)
            return None
        return mg, acc, finish
    tmp = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    return tmp, False, (lambda: tmp)


# ------------------------------------------------------------------------------------------------
# Weight-gradient side stream.  Within a block's backward, WGRAD(L) and DGRAD(L) both depend only on
# the layer's output gradient, so WGRAD runs on a second HIP stream and fills the CUs that the
# DGRAD chain leaves idle (small grids, tile tails, the latency-bound BN finalize launches).  The
# compute stream joins the side stream at the end of every backward pass (autograd engine
# callback), and the data-parallel bucket launch orders the all-reduce after both streams.
# PCMP_WGRAD_STREAM=0 keeps everything on one stream.
_SIDE: dict = {}
_JOIN_QUEUED = [False]
_ENV: dict = {}


def refresh_env() -> None:
    """Re-read the side-stream switches (PCMP_WGRAD_STREAM, PCMP_SIDE_WGRAD_WGS,
    PCMP_SIDE_WGRAD_WGS_LINEAR); they are cached because run_on_side is on the per-kernel host path
    (A/B tools call this after editing os.environ)."""
    _ENV["side"] = os.environ.get("PCMP_WGRAD_STREAM", "1") != "0"
    for key, var, dflt in (("wgs", "PCMP_SIDE_WGRAD_WGS", 384), ("wgs_linear", "PCMP_SIDE_WGRAD_WGS_LINEAR", 160)):
        try:
            _ENV[key] = max(0, int(os.environ.get(var, str(dflt))))
        except ValueError:
            _ENV[key] = dflt


refresh_env()


def side_stream_enabled() -> bool:
    return _ENV["side"]


def active_streams(device):
    """(compute stream, wgrad stream) pair in use on ``device`` this backward, or ()."""
    return _SIDE.get(("active", torch.device(device).index), ())


def _join(main, side, key):
    main.wait_stream(side)
    _SIDE.pop(key, None)
    _JOIN_QUEUED[0] = False


def fork_side(fn: Callable[[], object], keep_alive):
    """Run ``fn`` on the device's side stream, ordered after the compute stream's work so far, and
    return ``(result, event)``: the compute stream must ``wait_event(event)`` (``join_side``) before
    it consumes the result.  For independent branches inside one autograd node (a residual block's
    downsample conv next to its main branch)."""
    dev = keep_alive[0].device
    main = torch.cuda.current_stream(dev)
    side = _SIDE.get(dev.index)
    if side is None:
        side = _SIDE[dev.index] = torch.cuda.Stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    for t in keep_alive:
        if t is not None:
            t.record_stream(side)
    ev = torch.cuda.Event()
    ev.record(side)
    return out, ev


def join_side(result, ev):
    """Make the compute stream wait for a ``fork_side`` result and register its tensors with it."""
    ts = [t for t in (result if isinstance(result, (tuple, list)) else (result,)) if isinstance(t, torch.Tensor)]
    main = torch.cuda.current_stream(ts[0].device)
    main.wait_event(ev)
    for t in ts:
        t.record_stream(main)
    return result


def _side_wgrad_wgs() -> int:
    """Split-K workgroup target of side-stream WGRADs (``PCMP_SIDE_WGRAD_WGS``, default 384; 0 keeps
    the per-shape autotune, which times each WGRAD alone)."""
    return _ENV["wgs"]


# per device: [side stream, ring of fork events, ring position].  run_on_side runs ~50 times per
# training step, so its host cost counts (BERT-base's eager step is launch-bound on a slow host,
# profiles/r4_bert_host_prof.txt): raw current-stream get / set instead of Stream objects and the
# stream context manager, and recycled events instead of one new Event per fork.  A recycled
# event is re-recorded only after 256 later forks -- the wait enqueued on it long since resolved.
_SIDE_CTX: dict = {}
_NEV = 256


def _side_ctx(idx: int):
    c = _SIDE_CTX.get(idx)
    if c is None:
        side = _SIDE.get(idx)
        if side is None:
            side = _SIDE[idx] = torch.cuda.Stream(idx)
        c = _SIDE_CTX[idx] = [side, [torch.cuda.Event() for _ in range(_NEV)], 0]
    return c


def run_on_side(fn: Callable[[], None], keep_alive, linear: bool = False) -> None:
    """Run ``fn`` (kernel launches) on the device's WGRAD stream, ordered after the compute stream's
    work so far; ``keep_alive`` tensors are recorded on the side stream for the caching allocator.
    ``linear``: Linear-layer WGRADs (BERT's M = 4096-token reductions) take the split-K workgroup
    target PCMP_SIDE_WGRAD_WGS_LINEAR (160: fewer splits and reduce launches -- +1.8 % BERT-base
    step vs 384, profiles/r5_bert_wgs_ab.txt) instead of the conv target."""
    idx = keep_alive[0].get_device()
    c = _side_ctx(idx)
    side = c[0]
    cur = torch._C._cuda_getCurrentStream(idx)   # (stream id, device index, device type)
    ev = c[1][c[2]]
    c[2] = (c[2] + 1) % _NEV
    ev.record()                                   # on the compute stream (current)
    side.wait_event(ev)
    if not _JOIN_QUEUED[0]:
        main = torch.cuda.Stream(stream_id=cur[0], device_index=cur[1], device_type=cur[2])
        key = ("active", idx)
        _SIDE[key] = (main, side)
        _JOIN_QUEUED[0] = True
        torch.autograd.Variable._execution_engine.queue_callback(lambda: _join(main, side, key))
    wgs = _ENV["wgs_linear" if linear else "wgs"]
    torch._C._cuda_setStream(stream_id=side.stream_id, device_index=idx, device_type=side.device_type)
    try:
        if wgs:
            prev = torch.ops.pcmp.set_knob("wgrad_wgs", wgs)
            try:
                fn()
            finally:
                torch.ops.pcmp.set_knob("wgrad_wgs", prev)   # keep a PCMP_KNOBS=wgrad_wgs=N setting
        else:
            fn()
    finally:
        torch._C._cuda_setStream(stream_id=cur[0], device_index=cur[1], device_type=cur[2])
    for t in keep_alive:
        t.record_stream(side)
