"""Shared pieces of ``tests/test_nhwc_kernels.py``: fp64 oracles of the memory-bound NHWC ops written from the TF
definitions (nothing here imports ``mdtf.ops``: padding geometry, the valid-tap average, the LRN window and the
first-maximum rule are restated, not shared), the elementwise comparisons, seeded inputs and sentinel-guarded buffers.

The comparisons.  ``U = 2^-24`` is the fp32 unit roundoff.  bf16 keeps 8 significant bits, so half a bf16 ulp of v is
``2^(e-9)`` for ``2^(e-1) <= |v| < 2^e`` (``half_ulp_bf16``): between ``2^-9 |v|`` and ``2^-8 |v|``.  A flat
``2^-9 |v|`` is NOT half an ulp: a correctly rounded result misses it for half of all values.

* ``check_bound``: ``|got - ref| <= bound`` element by element.  For an accumulation of k fp32 operations the bound is
  ``gamma(k) * sum|terms|``; ``out_bound`` adds the final rounding to bf16 (half an ulp) when the output is bf16.
* ``check_neighbour``: for kernels built on fast intrinsics with a bf16 output.  Each element is the bf16 rounding of
  the fp64 result or the bf16 value next to it, and at most 1 % of the elements are the neighbour.  An error of e
  relative to the value moves an element to the neighbour with probability about ``e / 2^-8``, so fp32 arithmetic
  with errors of a few U passes with a margin of three orders of magnitude, while anything computed from a
  bf16-rounded intermediate does not.

Measured constants (CPU, PyTorch fp32 against the fp64 oracle, over every input ``test_nhwc_kernels.py`` builds with
``xent_case``):

* ``torch.logsumexp`` in fp32: at most 1.59 units of ``U * max(|lse|, 1)``;
* ``F.cross_entropy`` in fp32: at most 1.58 units of ``U * (|lse| + |x_label|)``.

(Both maxima come from the 513-row case; the rows with masked classes reach 1.34 and 1.26, the other three-row cases
stay under 0.95 and 0.37.)  ``LSE_UNITS_CPU`` = ``LOSS_UNITS_CPU`` = 2 is these figures rounded up to whole units, so
that the tests on ``cpu``, which assert them again, do not hinge on the summation order of one PyTorch build.  The
device's ``__expf`` / ``__logf`` are specified to a few ulp where the CPU's are below one, so ``lse_bound`` allows 8
times the constants on top of what can be derived (the sum's roundings and the roundings of ``m + log s`` and
``lse - x_label``).
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from optim_helpers import U, TINY, gamma, bits_equal  # noqa: E402,F401

TINY16 = 2.0 ** -133            # one bf16 denormal
LSE_UNITS_CPU = 2.0
LOSS_UNITS_CPU = 2.0
INTRINSIC_FACTOR = 8.0


# ------------------------------------------------------------------------------------------------------ inputs
def bf16_exact(t):
    """fp32 tensor whose values are bf16-representable."""
    return t.float().bfloat16().float()


def randn(shape, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return bf16_exact(torch.randn(shape, generator=gen) * scale)


def put(t, device):
    """cpu: an fp32 copy; cuda: the same values as bf16 (exact: the values are bf16-representable)."""
    if t is None:
        return None
    if device == "cpu":
        return t.clone()
    return t.to(device).bfloat16() if t.dtype == torch.float32 else t.to(device)


# ------------------------------------------------------------------------------------------------- comparisons
def round_bf16(ref):
    """fp64 -> the nearest bf16 value (ties to even), as fp64; one rounding, not double -> float -> bf16."""
    _, e = torch.frexp(ref)
    e = e.clamp(min=-125)
    q = torch.ldexp(torch.ones_like(ref), e - 8)
    return torch.round(ref / q) * q


def half_ulp_bf16(v):
    """Half the spacing of bf16 values around v (fp64): the most a rounding to nearest moves v."""
    _, e = torch.frexp(v.abs())
    h = torch.ldexp(torch.ones_like(v), e.clamp(min=-125) - 9)
    return torch.where(v == 0, torch.full_like(v, TINY16), h)


def _ordered(t):
    """bf16 -> integers in value order, +0 and -0 both 0: neighbours differ by one."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7fff))


def check_bound(got, ref, bound, what):
    got, ref = got.detach().cpu().double(), ref.detach()
    bound = bound.detach() if torch.is_tensor(bound) else bound
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), "%s: non-finite elements differ from the reference's" % what
    assert torch.equal(got[~fin].nan_to_num(1.5, 2.5, 3.5), ref[~fin].nan_to_num(1.5, 2.5, 3.5)), what
    err = (got - ref).abs()[fin]
    bnd = bound.expand_as(ref)[fin] if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = float((err / bnd.clamp(min=TINY)).max()) if err.numel() else 0.0
    print("NHWC_ERR %-58s max %.3f of its bound" % (what, ratio))
    bad = ~(err <= bnd)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements off; first (finite #%d): err %.6g bound %.6g" % (
            what, int(bad.sum()), err.numel(), i, float(err[i]), float(bnd[i])))
    return ratio


def out_bound(ref, acc, bf16_out):
    """The bound of an output whose fp32 value is within ``acc`` of ``ref``, stored as bf16 or kept in fp32."""
    if bf16_out:
        return half_ulp_bf16(ref.abs() + acc) + acc         # the value that is rounded lies within acc of ref
    return acc + TINY


def check_neighbour(got, ref, what, cap=0.01):
    """``got`` (bf16, or fp32 rounded to bf16 here) is round_bf16(ref) or the bf16 value next to it; at most ``cap``
    of the elements are the neighbour."""
    got, ref = got.detach().cpu(), ref.detach()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    got = got.bfloat16()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN positions" % what
    want = round_bf16(ref.masked_fill(nan, 0.0)).bfloat16()
    d = (_ordered(got.masked_fill(nan, 0.0)) - _ordered(want)).abs()
    far = d > 1
    n_nb = int((d == 1).sum())
    print("NHWC_NB  %-58s %d of %d elements are the neighbour (cap %d)" % (what, n_nb, d.numel(),
                                                                          int(cap * d.numel())))
    if far.any():
        i = int(far.flatten().nonzero()[0])
        raise AssertionError("%s: %d of %d elements are neither the rounded fp64 result nor its neighbour; first at "
                             "%d: got %r want %r" % (what, int(far.sum()), d.numel(), i, float(got.flatten()[i]),
                                                      float(want.flatten()[i])))
    assert n_nb <= cap * d.numel(), "%s: %d of %d elements are the neighbour, more than %g" % (what, n_nb, d.numel(),
                                                                                              cap)
    return n_nb


# ------------------------------------------------------------------------------------- sentinel-guarded buffers
GUARD_BYTES = 16                # keeps the 16-byte vector accesses of the kernels aligned
_SENTINEL = {torch.float32: (torch.int32, -842150451), torch.bfloat16: (torch.int16, -12851),
             torch.uint8: (torch.uint8, 0xCD), torch.int64: (torch.int64, -3617008641903833651)}      # 0xCDCD...


class Guarded(object):
    """A tensor of ``shape`` placed GUARD_BYTES into a sentinel-filled buffer with GUARD_BYTES after it.  ``t`` None:
    an output, left full of sentinels (``all_written`` then tells whether a kernel stored every element)."""

    def __init__(self, t, device, dtype=None, shape=None):
        dtype = dtype or t.dtype
        shape = tuple(t.shape) if shape is None else tuple(shape)
        n = 1
        for s in shape:
            n *= s
        self.bits, self.pattern = _SENTINEL[dtype]
        self.pad = GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(n + 2 * self.pad, dtype=dtype, device=device)
        self.buf.view(self.bits).fill_(self.pattern)
        self.t = self.buf[self.pad:self.pad + n].view(shape)
        assert self.t.data_ptr() % 16 == 0
        if t is not None:
            self.t.copy_(t)
        self.before = self.buf.clone()

    def guards_intact(self):
        b = self.buf.view(self.bits)
        return bool((b[:self.pad] == self.pattern).all()) and bool((b[-self.pad:] == self.pattern).all())

    def unchanged(self):
        return torch.equal(self.buf.view(self.bits), self.before.view(self.bits))

    def all_written(self):
        return not bool((self.t.reshape(-1).view(self.bits) == self.pattern).any())


def assert_contained(what, inputs, outputs):
    for i, g in enumerate(inputs):
        assert g.unchanged(), "%s: input %d modified" % (what, i)
    for i, g in enumerate(outputs):
        assert g.guards_intact(), "%s: wrote outside output %d" % (what, i)
        assert g.all_written(), "%s: output %d has elements no thread stored" % (what, i)


# ------------------------------------------------------------------------------------------- pooling (tf.nn.*_pool)
def same_pad(n, k, s):
    """TF SAME along one axis: (out, pad_before)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def pool_geometry(h, w, k, s, padding):
    """(OH, OW, pad_top, pad_left)"""
    if padding == "SAME":
        (oh, pt), (ow, pl) = same_pad(h, k[0], s[0]), same_pad(w, k[1], s[1])
        return oh, ow, pt, pl
    assert padding == "VALID"
    return (h - k[0]) // s[0] + 1, (w - k[1]) // s[1] + 1, 0, 0


def _taps(geo, h, w, k, s):
    """Every (oh, ow, kh, kw, ih, iw) whose tap lies inside the image, in (kh, kw) scan order per window."""
    oh_n, ow_n, pt, pl = geo
    for oh in range(oh_n):
        for ow in range(ow_n):
            for kh in range(k[0]):
                ih = oh * s[0] - pt + kh
                if ih < 0 or ih >= h:
                    continue
                for kw in range(k[1]):
                    iw = ow * s[1] - pl + kw
                    if 0 <= iw < w:
                        yield oh, ow, kh, kw, ih, iw


taps = _taps                     # public name: bn_helpers walks the windows in the same scan order


def pool_ref(x, k, s, padding, is_max):
    """x: fp64 NHWC.  Returns y, the argmax tap kh*KW + kw (first maximum in scan order), the valid-tap count per
    window and sum|x| over each window."""
    n, h, w, c = x.shape
    geo = pool_geometry(h, w, k, s, padding)
    oh_n, ow_n = geo[0], geo[1]
    y = torch.full((n, oh_n, ow_n, c), float("-inf") if is_max else 0.0, dtype=torch.float64)
    arg = torch.zeros((n, oh_n, ow_n, c), dtype=torch.int64)
    cnt = torch.zeros((oh_n, ow_n), dtype=torch.float64)
    sabs = torch.zeros_like(y)
    for oh, ow, kh, kw, ih, iw in _taps(geo, h, w, k, s):
        v = x[:, ih, iw, :]
        cnt[oh, ow] += 1
        if is_max:
            take = v > y[:, oh, ow, :]
            y[:, oh, ow, :] = torch.where(take, v, y[:, oh, ow, :])
            arg[:, oh, ow, :] = torch.where(take, torch.full_like(arg[:, oh, ow, :], kh * k[1] + kw),
                                            arg[:, oh, ow, :])
        else:
            y[:, oh, ow, :] += v
            sabs[:, oh, ow, :] += v.abs()
    assert bool((cnt > 0).all())
    if not is_max:
        y = y / cnt[None, :, :, None]
        sabs = sabs / cnt[None, :, :, None]
    return dict(y=y, arg=arg, cnt=cnt, sabs=sabs, geo=geo)


def pool_bwd_ref(dy, fwd, x_shape, k, s, is_max):
    """dx, sum|terms| and the number of windows over each input pixel.  max: the whole dy goes to the first maximum
    of its window; avg: dy / (valid taps) to every valid tap."""
    n, h, w, c = x_shape
    dx = torch.zeros(x_shape, dtype=torch.float64)
    sabs = torch.zeros_like(dx)
    nwin = torch.zeros((h, w), dtype=torch.float64)
    for oh, ow, kh, kw, ih, iw in _taps(fwd["geo"], h, w, k, s):
        if is_max:
            t = dy[:, oh, ow, :] * (fwd["arg"][:, oh, ow, :] == kh * k[1] + kw)
        else:
            t = dy[:, oh, ow, :] / fwd["cnt"][oh, ow]
        dx[:, ih, iw, :] += t
        sabs[:, ih, iw, :] += t.abs()
        nwin[ih, iw] += 1
    return dx, sabs, nwin


# ---------------------------------------------------------------------------------------------- activations
GELU_C, GELU_A = math.sqrt(2.0 / math.pi), 0.044715


def gelu64(v):
    """tanh form: 0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3)))"""
    return 0.5 * v * (1.0 + torch.tanh(GELU_C * (v + GELU_A * v ** 3)))


def act64(v, act):
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    return gelu64(v) if act == "gelu" else v


def act_grad64(v, act):
    """d act / d v at the fp64 pre-activation v (ReLU: 1 where v > 0)."""
    if act == "relu":
        return (v > 0).double()
    if act == "gelu":
        v = v.detach().clone().requires_grad_(True)
        (g,) = torch.autograd.grad(gelu64(v).sum(), v)
        return g
    return torch.ones_like(v)


def _gelu_d2_max():
    v = torch.linspace(-8.0, 8.0, 160001, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(gelu64(v).sum(), v, create_graph=True)
    (h,) = torch.autograd.grad(g.sum(), v)
    return float(h.abs().max())


GELU_D2_MAX = _gelu_d2_max() * (1.0 + 1e-6)      # max |gelu''| (about 0.80, at 0)


# ------------------------------------------------------------------------------------------------------- LRN
def lrn_ref(x, dy, r, bias, alpha, beta):
    """tf.nn.lrn: y_c = x_c / (bias + alpha * sum_{j in [c-r, c+r] & [0, C)} x_j^2)^beta over the last axis; returns
    y and dL/dx for dL/dy = dy (analytic: autograd through this fp64 expression)."""
    x = x.detach().clone().requires_grad_(True)
    c = x.shape[-1]
    sq = x * x
    win = torch.stack([sq[..., max(0, i - r):min(c, i + r + 1)].sum(-1) for i in range(c)], -1)
    y = x / (bias + alpha * win) ** beta
    (dx,) = torch.autograd.grad((y * dy).sum(), x)
    return y.detach(), dx


# ------------------------------------------------------------------------------------------ softmax cross-entropy
def xent_ref(x, labels, dloss):
    """x fp64 [N, K].  lse via max-shifted logsumexp, loss = lse - x[label], dlogits = (softmax - onehot) * dloss."""
    m = x.max(1, keepdim=True).values
    lse = (m + torch.log(torch.exp(x - m).sum(1, keepdim=True))).squeeze(1)
    loss = lse - x.gather(1, labels[:, None]).squeeze(1)
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, labels[:, None], 1.0)
    return lse, loss, (p - onehot) * dloss[:, None], p


def lse_bound(x, labels, lse, chain):
    """Bounds of the fp32 lse and loss.  s = sum exp(x - m) lies in [1, K]: every term is rounded by exp and the
    sum adds at most ``chain`` roundings on its longest path (per-thread partial sums, rescales of the online form and
    the merge tree), each relative to s, and d log(s) = ds / s: gamma(chain) absolute.  m + log s and lse - x_label
    round once each.  The intrinsics' own error: INTRINSIC_FACTOR times what the CPU's fp32 shows."""
    xl = x.gather(1, labels[:, None]).squeeze(1).abs()
    e_lse = gamma(chain) + U * lse.abs() + INTRINSIC_FACTOR * LSE_UNITS_CPU * U * lse.abs().clamp(min=1.0)
    e_loss = gamma(chain) + 2 * U * (lse.abs() + xl) + INTRINSIC_FACTOR * LOSS_UNITS_CPU * U * (lse.abs() + xl)
    return e_lse, e_loss


def xent_case(n, k, seed):
    """Logits [n, k] (bf16-representable fp32), labels and dloss.  Row 0: plain; row 1: shifted by +80; row 2: one
    logit 60 above the rest (the label elsewhere).  Labels: column 0, k - 1 and an odd interior column; dloss 1, 0,
    -2.5 (further rows: plain, random labels and dloss).  Columns 0 and k - 1 hold each row's larger logits, so a
    kernel that drops an edge column misses the bound by orders of magnitude."""
    x = randn((n, k), seed)
    x[:, 0] = x[:, 0].abs() + 3.0
    x[:, k - 1] = x[:, k - 1].abs() + 3.0
    x = bf16_exact(x)
    odd = (k // 2) | 1 if k > 2 else 1
    gen = torch.Generator().manual_seed(seed + 1)
    labels = torch.cat([torch.tensor([0, k - 1, odd]), torch.randint(0, k, (max(n - 3, 0),), generator=gen)])[:n]
    dloss = torch.cat([torch.tensor([1.0, 0.0, -2.5]), torch.randn(max(n - 3, 0), generator=gen)])[:n]
    if n > 1:
        x[1] = bf16_exact(x[1] + 80.0)
    if n > 2:
        peak = 4                                   # even: never the odd label column
        assert peak != odd
        x[2, peak] = bf16_exact(x[2].max() + 60.0)
    return x, labels, dloss
