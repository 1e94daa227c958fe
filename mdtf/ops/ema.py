"""Exponential moving average of the weights over a flat fp32 buffer.

``ema -= (1 - decay) * (ema - w)`` (``tf.train.ExponentialMovingAverage``), one launch per update target, beside
the fused optimizer launches of :mod:`mdtf.ops.optim`.  GPU tensors run ``mdtf_ema_update`` (``csrc/ema.hip``);
CPU tensors, and ``MDTF_KERNELS=torch``, use the PyTorch form below (the same formula).

``omd`` is ``1 - decay``, formed by the caller in double and rounded to fp32 once (:func:`one_minus_decay`); the
kernel never forms it.  ``omd_dev`` (optional) is a 1-float device tensor the kernel reads instead of the scalar, so
a hipGraph-captured step (:mod:`mdtf.train.graph`) picks up the per-step decay without re-capture.
"""
import ctypes

from . import _native

_native.register("mdtf_ema_update", [_native.L, _native.P, _native.P, _native.P, _native.F, _native.P])

# csrc/ema.hip: kThreads, kEmaVpt; one block owns CHUNK consecutive elements (the launch does not cap its grid)
THREADS = 256
VPT = 4
CHUNK = 4 * THREADS * VPT


def one_minus_decay(decay):
    """``1 - decay`` in double, rounded to fp32 once (what the kernel's float argument / device buffer holds)."""
    return ctypes.c_float(1.0 - float(decay)).value


def _native_ok(t):
    return t.is_cuda and _native.mode() != "torch" and _native.use_native(t)


def ema_update_(ema, master, omd, omd_dev=None):
    """``ema -= omd * (ema - master)`` in place; ``omd_dev[0]`` overrides ``omd`` when given."""
    if _native_ok(ema):
        _native.check(_native.fn("mdtf_ema_update")(
            ema.numel(), _native.ptr(ema), _native.ptr(master), _native.ptr(omd_dev), float(omd),
            _native.stream_ptr()), "ema_update")
        return
    if omd_dev is not None:
        omd = omd_dev.tolist()[0]
    ema.sub_((ema - master).mul_(float(omd)))
