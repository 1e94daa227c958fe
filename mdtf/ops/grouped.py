"""Grouped 3x3 convolution (``conv2d(..., groups=G)``, the conv2 of ResNeXt) on the kernels of ``csrc/conv_group.hip``.

The op, for an NHWC ``x`` [N, H, W, C] and a filter ``w`` [kh, kw, C / G, Cout] (HWIO with the per-group input count, as
TF 2 / Keras ``Conv2D(groups=G)``)::

    y[n, oh, ow, co] = sum_{i, j, k} x[n, oh * s + i - pt, ow * s + j - pl, g * C / G + k] * w[i, j, k, co]

with ``g = co // (Cout / G)`` and taps outside the image contributing 0.  The HIP kernels run for GPU tensors in bf16
with ``C == Cout``, ``C % 32 == 0``, ``C / G`` in {4, 8, 16, 32}, a 3x3 filter, stride 1 or 2 (the same on both axes),
dilation 1 and pads of at most 2: forward and data gradient accumulate in fp32 on the MFMA units and round once to
bf16; the weight gradient is a two-phase, atomic-free reduction (per-chunk fp32 partials, then an fp64 sum in chunk
order) that lands in the variable's fp32 gradient slot when there is one, and is bitwise repeatable.

Every other case runs the PyTorch expression (a grouped ``F.conv2d``): CPU tensors, ``MDTF_KERNELS=torch`` (the
comparator), fp32 activations, ``C / G`` of 1, 2, 64 or more, ``C != Cout``, ``C % 32 != 0``, filters other than 3x3,
dilation, unequal or larger strides, a pad above 2 and an image of 2 GiB or more.  Not here: BN statistics in the
epilogue, NCHW.
"""
import torch

from . import _native as N
from ..train import variables as V

# the 15 ints: N, H, W, C, Cg, OH, OW, KH, KW, S, D, PT, PB, PL, PR
N.register("mdtf_gconv_fwd", [N.P, N.P, N.P] + [N.I] * 15 + [N.P])
N.register("mdtf_gconv_dgrad", [N.P, N.P, N.P] + [N.I] * 15 + [N.P])
N.register("mdtf_gconv_wgrad", [N.P, N.P, N.P] + [N.I] * 15 + [N.P])
# the 8 ints of the plan: N, H, W, C, Cg, OH, OW, S
N.register("mdtf_gconv_wgrad_finalize", [N.P, N.P] + [N.I] * 9 + [N.P])
N.register("mdtf_gconv_wgrad_ws", [N.I] * 8, restype=N.L)
N.register("mdtf_gconv_wgrad_chunk", [N.I] * 8, restype=N.L)
N.register("mdtf_gconv_band", [N.I] * 8, restype=N.L)

GROUP_WIDTHS = (4, 8, 16, 32)
MAX_PAD = 2


def native_ok(x, w, groups, stride, dil, pads=(0, 0, 0, 0)):
    """Whether the HIP kernels take this call (else the PyTorch expression runs)."""
    kh, kw, cg, co = w.shape
    c = x.shape[-1]
    return (N.use_native(x) and x.dtype == torch.bfloat16 and co == c and c % 32 == 0 and cg in GROUP_WIDTHS
            and cg * groups == c and (kh, kw) == (3, 3) and stride[0] == stride[1] and stride[0] in (1, 2)
            and tuple(dil) == (1, 1) and max(pads) <= MAX_PAD and x.shape[1] * x.shape[2] * c < (1 << 30)
            and x.shape[0] * x.shape[1] * x.shape[2] < (1 << 31))


def _plan_ints(geo):
    return geo[:7] + [geo[9]]


def band(geo):
    """Output rows per block of the forward kernel for the 15 ints ``geo``."""
    return int(N.fn("mdtf_gconv_band")(*_plan_ints(geo)))


def wgrad_chunk(geo):
    """Output pixels per chunk (one partial each, at most) of the weight gradient."""
    return int(N.fn("mdtf_gconv_wgrad_chunk")(*_plan_ints(geo)))


def wgrad_workspace(geo, device):
    """The partials buffer of the weight gradient: fp32 ``[chunks, 9, C, Cg]`` flattened."""
    floats = N.fn("mdtf_gconv_wgrad_ws")(*_plan_ints(geo))
    return torch.empty(max(int(floats), 1), dtype=torch.float32, device=device)


def dgrad_nhwc(dy, w, geo):
    """The data gradient for ``dy`` [N, OH, OW, C] (``geo``: the 15 ints of the entry points)."""
    dx = torch.empty((geo[0], geo[1], geo[2], geo[3]), dtype=dy.dtype, device=dy.device)   # every element is stored
    N.check(N.fn("mdtf_gconv_dgrad")(N.ptr(dy), N.ptr(w), N.ptr(dx), *geo, N.stream_ptr()), "gconv_dgrad")
    return dx


def wgrad_into(x, dy, geo, out, accumulate):
    """``out`` (fp32 [3, 3, Cg, C]) = or += the weight gradient; both phases on the current stream."""
    ws = wgrad_workspace(geo, x.device)
    N.check(N.fn("mdtf_gconv_wgrad")(N.ptr(x), N.ptr(dy), N.ptr(ws), *geo, N.stream_ptr()), "gconv_wgrad")
    N.check(N.fn("mdtf_gconv_wgrad_finalize")(N.ptr(ws), N.ptr(out), *_plan_ints(geo), int(bool(accumulate)),
                                              N.stream_ptr()), "gconv_wgrad_finalize")
    return out


class _Grouped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pads, out_hw):
        x = x.contiguous()
        w = w.contiguous()
        n, h, wd, c = x.shape
        oh, ow = out_hw
        geo = [n, h, wd, c, w.shape[2], oh, ow, 3, 3, stride, 1, pads[0], pads[1], pads[2], pads[3]]
        y = torch.empty((n, oh, ow, c), dtype=x.dtype, device=x.device)
        N.check(N.fn("mdtf_gconv_fwd")(N.ptr(x), N.ptr(w), N.ptr(y), *geo, N.stream_ptr()), "gconv_fwd")
        ctx.save_for_backward(x, w)
        ctx.geo = geo
        ctx.w_dtype = w.dtype
        ctx.sink = V.grad_sink(w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        geo = ctx.geo
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = dgrad_nhwc(dy, w, geo)
        if ctx.needs_input_grad[1]:
            sink = ctx.sink
            if sink is not None:                            # straight into the fp32 grad slot
                wgrad_into(x, dy, geo, V.accumulate_slot(sink), True)
                dw = V.grad_marker(w)
            else:
                dw = wgrad_into(x, dy, geo, torch.empty(w.shape, dtype=torch.float32, device=w.device), False)
                dw = dw.to(ctx.w_dtype)
        return dx, dw, None, None, None


def grouped_nhwc(x, w, stride, pads, out_hw):
    """The kernels' path (:func:`native_ok` holds): bf16 ``x``, ``w`` [3, 3, Cg, C], one stride for both axes."""
    if w.dtype != x.dtype:
        w = w.to(x.dtype)
    return _Grouped.apply(x, w, int(stride), tuple(pads), tuple(out_hw))
