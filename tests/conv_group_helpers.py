"""The fp64 oracle of ``tests/test_conv_group.py``: a grouped convolution as a direct loop over taps and groups, written
from the definition (nothing here imports ``mdtf.ops`` or calls ``F.conv2d``).

For NHWC ``x`` [N, H, W, C] and ``w`` [kh, kw, C / G, Cout], output channel ``co`` belongs to group ``co // (Cout / G)``
and reads input channels ``g * C / G .. (g + 1) * C / G - 1``; a tap outside the image contributes 0.  Besides y, dx and
dw the oracle returns ``sum |terms|`` of every element and the number of taps behind every y and dx pixel, which is what
the bounds are made of (products of two bf16 values are exact in fp32, zero-padded MFMA entries add exact zeros):

* y, dx: ``gamma(T * Cg) * sum |terms|`` for the T taps inside the image, plus the rounding of a bf16 result;
* dw: ``gamma(N * OH * OW + 2) * sum |terms|`` (any summation order, the final rounding, the add into a slot).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import gamma  # noqa: E402


def _axis(n_out, n_in, t, s, pad):
    """The outputs o with 0 <= o * s + t - pad < n_in as a slice, and the slice of their sources (None: none)."""
    off = t - pad
    o0 = max(0, -(off // s))
    o1 = min(n_out, (n_in - 1 - off) // s + 1) if n_in - 1 - off >= 0 else 0
    if o1 <= o0:
        return None
    return slice(o0, o1), slice(o0 * s + off, (o1 - 1) * s + off + 1, s)


class Oracle(object):
    def __init__(self, x, w, dy, groups, s, pads):
        n, h, wd, c = x.shape
        kh, kw, cg, cout = w.shape
        _, oh, ow, _ = dy.shape
        cog = cout // groups
        x, w, dy = x.double(), w.double(), dy.double()
        self.y, self.y_abs = torch.zeros_like(dy), torch.zeros_like(dy)
        self.dx, self.dx_abs = torch.zeros_like(x), torch.zeros_like(x)
        self.dw, self.dw_abs = torch.zeros_like(w), torch.zeros_like(w)
        self.y_taps, self.dx_taps = torch.zeros(oh, ow, dtype=torch.float64), torch.zeros(h, wd, dtype=torch.float64)
        self.cg, self.k = cg, n * oh * ow
        for i in range(kh):
            rows = _axis(oh, h, i, s, pads[0])
            for j in range(kw):
                cols = _axis(ow, wd, j, s, pads[2])
                if rows is None or cols is None:
                    continue
                (ro, ri), (co, ci) = rows, cols
                self.y_taps[ro, co] += 1
                self.dx_taps[ri, ci] += 1
                for g in range(groups):
                    gi, go = slice(g * cg, (g + 1) * cg), slice(g * cog, (g + 1) * cog)
                    xs, ds, wt = x[:, ri, ci, gi, None], dy[:, ro, co, None, go], w[i, j, :, go]
                    t = xs * wt                                     # [N, rows, cols, Cg, Cout / G]
                    self.y[:, ro, co, go] += t.sum(3)
                    self.y_abs[:, ro, co, go] += t.abs().sum(3)
                    t = ds * wt
                    self.dx[:, ri, ci, gi] += t.sum(4)
                    self.dx_abs[:, ri, ci, gi] += t.abs().sum(4)
                    t = xs * ds
                    self.dw[i, j, :, go] += t.sum((0, 1, 2))
                    self.dw_abs[i, j, :, go] += t.abs().sum((0, 1, 2))

    def check(self, what, y, dx, dw, bf16, slot0=None):
        """y / dx (None: not checked) and dw against the oracle; ``slot0``: what the fp32 slot held before."""
        for name, got, ref, sabs, taps in (("y", y, self.y, self.y_abs, self.y_taps),
                                           ("dx", dx, self.dx, self.dx_abs, self.dx_taps)):
            if got is not None:
                acc = gamma(taps * self.cg)[None, :, :, None] * sabs
                NH.check_bound(got, ref, NH.out_bound(ref, acc, bf16), "%s %s" % (what, name))
        if dw is not None:
            ref, sabs = self.dw, self.dw_abs
            if slot0 is not None:
                ref, sabs = ref + slot0.double(), sabs + slot0.double().abs()
            NH.check_bound(dw, ref, gamma(self.k + 2) * sabs + NH.TINY, what + " dw")
