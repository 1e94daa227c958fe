"""Global gradient norm and the clip coefficient on the device.

``tf.clip_by_global_norm`` / ``tf.global_norm`` over the flat fp32 gradient
buffers.  The fused update kernels (:mod:`mdtf.ops.optim`) read
``[lr, lr_t, grad_scale]`` from a device tensor ``dyn``; clipping multiplies
``grad_scale`` by ``coef = clip_norm / max(norm, clip_norm)``, so it is two
small launches in front of the unchanged updates and no host read of the norm:

* :func:`grad_sumsq_` — one launch over the gradient of every update target,
  one fp32 partial per block (``csrc/gradnorm.hip``; no atomics, bitwise
  repeatable);
* :func:`clip_finalize_` — partials summed in a fixed order in fp64, then
  ``norm = grad_scale * sqrt(sumsq)`` (the norm of the AVERAGED gradient the
  optimizer applies), ``eff = [lr, lr_t, grad_scale * coef]`` and
  ``stats = [norm, coef]``.

Semantics (TF): ``norm <= clip_norm`` gives ``coef == 1`` exactly and an
effective scale bitwise equal to the input; a zero norm gives ``coef == 1``; a
non-finite norm gives ``coef = NaN`` (every update turns NaN, so the failure is
loud); ``clip_norm <= 0`` computes the norm only.

GPU tensors run the HIP kernels; CPU tensors (and ``MDTF_KERNELS=torch``) use the
vectorised PyTorch reference below, the same math with one fp64 partial per
segment.
"""
import ctypes
import math

import torch

from . import _native

_native.register("mdtf_grad_sumsq_blocks", [_native.P, _native.I], _native.L)
_native.register("mdtf_grad_sumsq", [_native.P, _native.P, _native.I, _native.P, _native.L, _native.P])
_native.register("mdtf_clip_finalize", [_native.P, _native.I, _native.P, _native.F, _native.F, _native.F, _native.F,
                                        _native.P, _native.P, _native.P, _native.I, _native.P])

MAX_SEGMENTS = 8
FULL, REDUCE, COEF = 0, 1, 2      # clip_finalize_ modes: both halves | partials -> sumsq | sumsq -> coefficient


def _native_ok(t):
    return t.is_cuda and _native.mode() != "torch" and _native.use_native(t)


def _check_segments(grads):
    if not 1 <= len(grads) <= MAX_SEGMENTS:
        raise ValueError("grad_sumsq takes 1..%d gradient buffers, got %d" % (MAX_SEGMENTS, len(grads)))
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() % 4:
            raise ValueError("grad_sumsq needs contiguous fp32 buffers of a multiple of 4 elements (flat groups and "
                             "shards are 64-aligned), got %s x %d" % (g.dtype, g.numel()))


def num_partials(grads):
    """Partials one :func:`grad_sumsq_` launch over ``grads`` writes."""
    _check_segments(grads)
    if not _native_ok(grads[0]):
        return len(grads)
    ns = (ctypes.c_longlong * len(grads))(*[g.numel() for g in grads])
    n = _native.fn("mdtf_grad_sumsq_blocks")(ctypes.cast(ns, ctypes.c_void_p), len(grads))
    if n < 0:
        raise RuntimeError("mdtf_grad_sumsq_blocks: invalid argument")
    return int(n)


class NormBuffers(object):
    """Persistent buffers of one clipped train op: block partials (fp32 on the GPU, one fp64 per segment on the
    reference path), ``sumsq`` (fp64[1], what the sharded path all-reduces), ``eff`` = ``[lr, lr_t, grad_scale *
    coef]`` (the ``dyn`` of the update kernels) and ``stats`` = ``[norm, coef]``.  Allocated once, outside any
    hipGraph capture."""

    def __init__(self, grads):
        dev = grads[0].device
        self.n = num_partials(grads)
        self.native = _native_ok(grads[0])
        self.partials = torch.zeros(self.n, dtype=torch.float32 if self.native else torch.float64, device=dev)
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.eff = torch.zeros(3, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(2, dtype=torch.float32, device=dev)


def grad_sumsq_(grads, buf):
    """Sum of squares of every buffer of ``grads`` into ``buf.partials`` (one launch)."""
    _check_segments(grads)
    if buf.native:
        k = len(grads)
        ps = (ctypes.c_void_p * k)(*[g.data_ptr() for g in grads])
        ns = (ctypes.c_longlong * k)(*[g.numel() for g in grads])
        _native.check(_native.fn("mdtf_grad_sumsq")(
            ctypes.cast(ps, ctypes.c_void_p), ctypes.cast(ns, ctypes.c_void_p), k, _native.ptr(buf.partials),
            buf.partials.numel(), _native.stream_ptr()), "grad_sumsq")
        return
    if len(grads) != buf.partials.numel():
        raise ValueError("grad_sumsq: %d segments, buffers for %d" % (len(grads), buf.partials.numel()))
    for i, g in enumerate(grads):
        buf.partials[i] = g.double().pow(2).sum()


def clip_finalize_(buf, clip_norm, lr, lr_t, grad_scale, dyn=None, mode=FULL):
    """``buf.partials`` -> ``buf.sumsq`` -> ``buf.eff`` / ``buf.stats`` (see the module docstring).  ``dyn``
    (optional device ``[lr, lr_t, grad_scale]``) overrides the scalars, as in the update kernels."""
    if buf.native:
        _native.check(_native.fn("mdtf_clip_finalize")(
            _native.ptr(buf.partials), buf.partials.numel(), _native.ptr(buf.sumsq), float(clip_norm), float(lr),
            float(lr_t), float(grad_scale), _native.ptr(dyn), _native.ptr(buf.eff), _native.ptr(buf.stats), int(mode),
            _native.stream_ptr()), "clip_finalize")
        return
    if mode != COEF:
        ss = buf.partials.sum(dtype=torch.float64)      # fixed order
        if mode == REDUCE:
            buf.sumsq[0] = ss
            return
    else:
        ss = buf.sumsq[0]
    f32 = torch.float32
    if dyn is not None:
        d = dyn.to(f32)
        lr, lr_t, gs = d[0], d[1], d[2]
    else:
        lr, lr_t, gs = (torch.tensor(float(x), dtype=f32) for x in (lr, lr_t, grad_scale))
    gs = gs.to(ss.device)
    norm = (gs.double() * ss.sqrt()).to(f32)
    clip = torch.tensor(float(clip_norm), dtype=f32, device=norm.device)
    coef = torch.ones((), dtype=f32, device=norm.device)
    if float(clip_norm) > 0:
        if not math.isfinite(float(norm)):
            coef = torch.full((), float("nan"), dtype=f32, device=norm.device)
        elif bool(norm > clip):
            coef = clip / norm
    buf.eff[0] = lr
    buf.eff[1] = lr_t
    buf.eff[2] = gs if bool(coef == 1) else gs * coef
    buf.stats[0] = norm
    buf.stats[1] = coef
