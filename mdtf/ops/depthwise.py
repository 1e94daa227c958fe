"""``tf.nn.depthwise_conv2d`` on the direct NHWC kernels of ``csrc/depthwise.hip``.

The op, for an NHWC ``x`` [N, H, W, C] and a filter ``w`` [kh, kw, C, mult]::

    y[n, oh, ow, c * mult + m] = sum_{i, j} x[n, oh * sh + i * dh - pt, ow * sw + j * dw - pl, c] * w[i, j, c, m]

with taps outside the image contributing 0.  The HIP kernels run for GPU tensors in bf16 with ``C % 8 == 0``, channel
multiplier 1 and ``kh * kw <= 49``: forward and data gradient sum the taps in fp32 in ``(i, j)`` order and round once
to bf16; the weight gradient is a two-phase, atomic-free reduction (per-chunk fp32 partials, then an fp64 sum in chunk
order) that lands in the variable's fp32 gradient slot when there is one, and is bitwise repeatable.

Every other case runs the PyTorch expression (a grouped ``F.conv2d`` with ``groups = C``): CPU tensors,
``MDTF_KERNELS=torch`` (the comparator), fp32 activations, ``C % 8 != 0``, a channel multiplier above 1 and filters of
more than 49 taps.  Not here: BN statistics in the epilogue, relu6, NCHW.
"""
import torch

from . import _native as N
from ..train import variables as V

# the 16 ints: N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PB, PL, PR
N.register("mdtf_dwconv_fwd", [N.P, N.P, N.P] + [N.I] * 16 + [N.P])
N.register("mdtf_dwconv_dgrad", [N.P, N.P, N.P] + [N.I] * 16 + [N.P])
N.register("mdtf_dwconv_wgrad", [N.P, N.P, N.P] + [N.I] * 16 + [N.P])
N.register("mdtf_dwconv_wgrad_finalize", [N.P, N.P] + [N.I] * 7 + [N.P])
N.register("mdtf_dwconv_wgrad_ws", [N.I] * 6, restype=N.L)
N.register("mdtf_dwconv_wgrad_chunk", [N.I] * 6, restype=N.L)

MAX_TAPS = 49


def native_ok(x, w):
    """Whether the HIP kernels take this call (else the PyTorch expression runs)."""
    kh, kw, c, mult = w.shape
    return (N.use_native(x) and x.dtype == torch.bfloat16 and c % 8 == 0 and c >= 8 and mult == 1
            and kh * kw <= MAX_TAPS)


def wgrad_workspace(n, oh, ow, c, kh, kw, device):
    """The partials buffer of the weight gradient: fp32 ``[chunks, kh * kw, c]`` flattened."""
    floats = N.fn("mdtf_dwconv_wgrad_ws")(n, oh, ow, c, kh, kw)
    return torch.empty(max(int(floats), 1), dtype=torch.float32, device=device)


def wgrad_chunk(n, oh, ow, c, kh, kw):
    """Output pixels per chunk (one partial each) of the weight gradient for these sizes."""
    return int(N.fn("mdtf_dwconv_wgrad_chunk")(n, oh, ow, c, kh, kw))


def dgrad_nhwc(dy, w, geo):
    """The data gradient for ``dy`` [N, OH, OW, C] (``geo``: the 16 ints of the entry points)."""
    dx = torch.empty((geo[0], geo[1], geo[2], geo[3]), dtype=dy.dtype, device=dy.device)   # every element is stored
    N.check(N.fn("mdtf_dwconv_dgrad")(N.ptr(dy), N.ptr(w), N.ptr(dx), *geo, N.stream_ptr()), "dwconv_dgrad")
    return dx


def wgrad_into(x, dy, geo, out, accumulate):
    """``out`` (fp32 [kh, kw, C, 1]) = or += the weight gradient; both phases on the current stream."""
    n, _, _, c, oh, ow, kh, kw = geo[:8]
    ws = wgrad_workspace(n, oh, ow, c, kh, kw, x.device)
    N.check(N.fn("mdtf_dwconv_wgrad")(N.ptr(x), N.ptr(dy), N.ptr(ws), *geo, N.stream_ptr()), "dwconv_wgrad")
    N.check(N.fn("mdtf_dwconv_wgrad_finalize")(N.ptr(ws), N.ptr(out), n, oh, ow, c, kh, kw, int(bool(accumulate)),
                                               N.stream_ptr()), "dwconv_wgrad_finalize")
    return out


class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pads, dil, out_hw):
        x = x.contiguous()
        w = w.contiguous()
        n, h, wd, c = x.shape
        kh, kw = w.shape[0], w.shape[1]
        oh, ow = out_hw
        geo = [n, h, wd, c, oh, ow, kh, kw, stride[0], stride[1], dil[0], dil[1], pads[0], pads[1], pads[2], pads[3]]
        y = torch.empty((n, oh, ow, c), dtype=x.dtype, device=x.device)
        N.check(N.fn("mdtf_dwconv_fwd")(N.ptr(x), N.ptr(w), N.ptr(y), *geo, N.stream_ptr()), "dwconv_fwd")
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
        return dx, dw, None, None, None, None


def depthwise_nhwc(x, w, stride, pads, dil, out_hw):
    """The kernels' path (:func:`native_ok` holds): bf16 ``x``, ``w`` [kh, kw, C, 1]."""
    if w.dtype != x.dtype:
        w = w.to(x.dtype)
    return _Depthwise.apply(x, w, tuple(stride), tuple(pads), tuple(dil), tuple(out_hw))
