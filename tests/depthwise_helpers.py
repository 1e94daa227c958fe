"""Shared pieces of ``tests/test_depthwise.py``: the SAME / VALID geometry of ``tf.nn.depthwise_conv2d`` restated
from TF's definition and fp64 oracles of y, dx and dw as explicit tap loops (nothing here imports ``mdtf.ops``).

The op, for NHWC ``x`` [N, H, W, C] and a filter ``w`` [kh, kw, C, mult]::

    y[n, oh, ow, c * mult + m] = sum_{i, j} x[n, oh * sh + i * dh - pt, ow * sw + j * dw - pl, c] * w[i, j, c, m]

with a tap outside the image contributing 0.  Every oracle also returns ``sum |terms|`` and the number of terms of
each output element, which is what the bounds are made of:

* y and dx: products of two bf16 values are exact in fp32, so the error is that of the additions of the ``T`` taps
  inside the image: ``gamma(T) * sum_t |x_t w_t|``, plus the final rounding when the output is bf16
  (``nhwc_helpers.out_bound``).  With a channel multiplier the dx of one input channel sums ``T * mult`` terms.
* dw: any order of summing ``K = N * OH * OW`` fp32 terms is within ``gamma(K) * sum |terms|``; ``gamma(K + 2)`` allows
  the final rounding and the add into a gradient slot.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import gamma  # noqa: E402


def axis_geometry(n, k, s, d, padding):
    """One axis: (out, pad_before, pad_after) of TF's SAME / VALID with an effective filter (k - 1) * d + 1."""
    ke = (k - 1) * d + 1
    if padding == "SAME":
        out = -(-n // s)
        total = max((out - 1) * s + ke - n, 0)
        return out, total // 2, total - total // 2
    assert padding == "VALID"
    return (n - ke) // s + 1, 0, 0


class Geo(object):
    """The geometry of one case: sizes, strides, dilations, pads and output size."""

    def __init__(self, shape, k, s, d, padding):
        self.n, self.h, self.w, self.c = shape
        self.kh, self.kw = k
        self.sh, self.sw = (s, s) if isinstance(s, int) else s
        self.dh, self.dw = (d, d) if isinstance(d, int) else d
        self.padding = padding
        self.oh, self.pt, self.pb = axis_geometry(self.h, self.kh, self.sh, self.dh, padding)
        self.ow, self.pl, self.pr = axis_geometry(self.w, self.kw, self.sw, self.dw, padding)

    def ints(self):
        """The 16 ints of the entry points."""
        return [self.n, self.h, self.w, self.c, self.oh, self.ow, self.kh, self.kw, self.sh, self.sw, self.dh,
                self.dw, self.pt, self.pb, self.pl, self.pr]

    def taps(self):
        """Every tap (i, j) with the output range [o0, o1) x [q0, q1) whose source pixel lies inside the image, as
        (i, j, out rows slice, out cols slice, in rows slice, in cols slice)."""
        for i in range(self.kh):
            rows = _axis_range(self.oh, self.h, i, self.sh, self.dh, self.pt)
            if rows is None:
                continue
            for j in range(self.kw):
                cols = _axis_range(self.ow, self.w, j, self.sw, self.dw, self.pl)
                if cols is None:
                    continue
                yield i, j, rows[0], cols[0], rows[1], cols[1]


def _axis_range(n_out, n_in, t, s, d, pad):
    """The outputs o with 0 <= o * s + t * d - pad < n_in as a slice, and the slice of their source coordinates."""
    off = t * d - pad
    o0 = max(0, -(off // s)) if off < 0 else 0               # smallest o with o * s + off >= 0
    o1 = min(n_out, (n_in - 1 - off) // s + 1) if n_in - 1 - off >= 0 else 0
    if o1 <= o0:
        return None
    return slice(o0, o1), slice(o0 * s + off, (o1 - 1) * s + off + 1, s)


def fwd_ref(x, w, geo):
    """x fp64 [N, H, W, C], w fp64 [kh, kw, C, mult] -> y [N, OH, OW, C * mult], sum |terms| and the number of taps
    inside the image per output pixel ([OH, OW])."""
    n, c, mult = geo.n, geo.c, w.shape[3]
    y = torch.zeros((n, geo.oh, geo.ow, c, mult), dtype=torch.float64)
    sabs = torch.zeros_like(y)
    cnt = torch.zeros((geo.oh, geo.ow), dtype=torch.float64)
    for i, j, ro, co, ri, ci in geo.taps():
        t = x[:, ri, ci, :, None] * w[i, j]
        y[:, ro, co] += t
        sabs[:, ro, co] += t.abs()
        cnt[ro, co] += 1
    shape = (n, geo.oh, geo.ow, c * mult)
    return y.reshape(shape), sabs.reshape(shape), cnt


def dgrad_ref(dy, w, geo):
    """dy fp64 [N, OH, OW, C * mult] -> dx [N, H, W, C], sum |terms| and the number of terms per input pixel."""
    n, c, mult = geo.n, geo.c, w.shape[3]
    dy = dy.reshape(n, geo.oh, geo.ow, c, mult)
    dx = torch.zeros((n, geo.h, geo.w, c), dtype=torch.float64)
    sabs = torch.zeros_like(dx)
    cnt = torch.zeros((geo.h, geo.w), dtype=torch.float64)
    for i, j, ro, co, ri, ci in geo.taps():
        t = dy[:, ro, co] * w[i, j]
        dx[:, ri, ci] += t.sum(-1)
        sabs[:, ri, ci] += t.abs().sum(-1)
        cnt[ri, ci] += mult
    return dx, sabs, cnt


def wgrad_ref(x, dy, geo, mult=1):
    """dw [kh, kw, C, mult] and sum |terms|; every element sums at most K = N * OH * OW terms."""
    n, c = geo.n, geo.c
    dy = dy.reshape(n, geo.oh, geo.ow, c, mult)
    dw = torch.zeros((geo.kh, geo.kw, c, mult), dtype=torch.float64)
    sabs = torch.zeros_like(dw)
    for i, j, ro, co, ri, ci in geo.taps():
        t = x[:, ri, ci, :, None] * dy[:, ro, co]
        dw[i, j] = t.sum((0, 1, 2))
        sabs[i, j] = t.abs().sum((0, 1, 2))
    return dw, sabs


def y_bound(ref, sabs, cnt, bf16_out):
    """The bound of y or dx: gamma(T) * sum |terms| with T the element's own number of terms ([rows, cols])."""
    acc = gamma(cnt)[None, :, :, None] * sabs
    return NH.out_bound(ref, acc, bf16_out)


def dw_bound(sabs, geo):
    return gamma(geo.n * geo.oh * geo.ow + 2) * sabs + NH.TINY


def brute_fwd(x, w, geo):
    """The definition, one output element at a time (tiny shapes only): checks the sliced tap loops above."""
    mult = w.shape[3]
    y = torch.zeros((geo.n, geo.oh, geo.ow, geo.c * mult), dtype=torch.float64)
    for oh in range(geo.oh):
        for ow in range(geo.ow):
            for i in range(geo.kh):
                ih = oh * geo.sh + i * geo.dh - geo.pt
                if not 0 <= ih < geo.h:
                    continue
                for j in range(geo.kw):
                    iw = ow * geo.sw + j * geo.dw - geo.pl
                    if 0 <= iw < geo.w:
                        y[:, oh, ow] += (x[:, ih, iw, :, None] * w[i, j]).reshape(geo.n, -1)
    return y
