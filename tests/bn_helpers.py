"""Shared pieces of ``tests/test_bn_kernels.py``: fp64 oracles of training / inference BatchNorm (+ residual) (+ ReLU),
of the dual form ``relu(BN(x) + BN2(r))`` and of the stem form ``maxpool(relu(BN(x)))``, written from the
definitions, and the elementwise bounds of their fp32 evaluation.  The comparisons, the seeded inputs, the guarded
buffers and the pooling oracles are those of ``nhwc_helpers``.

Statistics.  A bf16 x bf16 product is exact in fp32, so ``S = sum x``, ``Q = sum x^2`` (and, backward, ``sum dz``,
``sum dz x``) carry only the roundings of their additions: with k additions on the longest path of one accumulator,
``|dS| <= gamma(k) sum|x|`` and ``|dQ| <= gamma(k) Q``.  The kernels' k (``reduce_k``): a block sums ``span`` rows,
``rg = 256 / tpr`` row groups interleaved (``tpr`` the largest power of two ``<= min(C / 8, 256)``), so a thread adds
``ceil(span / rg)`` times, then ``log2(rg)`` tree levels, then the finalize, which adds in fp64 except for
``fin_adds(P)`` fp32 additions when more than 128 partial rows arrive.  The number of row blocks is recovered from
the exported workspace size.  On ``cpu`` k = M: any summation order meets it.  ``fin_adds``: the finalize keeps four
fp32 accumulators per thread over rows ``grp + 32 u + 128 j``; whole groups of 128 further rows add once to each, and
a last incomplete group adds its up to three rows to the FIRST accumulator.  That is ``ceil(P / 128) - 1`` for every
P used here (1, 33, 128, 131, 261 and the kernels' own row-block counts up to 128), but more for, say, P = 224 (three
additions): the count below follows the loop, not the closed form.

Propagation (``stats_ref``).  ``mean = S / M``: ``em = g sum|x| / M``.  ``var = Q / M - mean^2`` cancels:
``ev = g Q / M + 2 |mean| em + em^2``, that is ``k U (var + mean^2)``, or ``k U (1 + mean^2 / var)`` of the variance:
the known loss of this form for a channel whose mean dwarfs its spread; the bound states exactly that and no more.
``invstd``: the cast of var, the add of eps, the relative error ``0.5 ev / (v - ev)`` of ``v^-1/2`` for v within ev,
and the intrinsic: AMD's HIP math API reference lists ``rsqrtf`` with a maximum error of 1 ulp and the CDNA ISA guide
gives V_RSQ_F32 as accurate to 1 ulp; one ulp is at most 2 U relative (``RSQRT_REL``).  The PyTorch branch computes
``1 / sqrt``, two correctly rounded operations: 2 U as well.

Forward (``fwd_ref``): the kernel evaluates ``x scale + shift`` with ``scale = gamma invstd'`` and
``shift = beta - mean' gamma invstd'``, i.e. ``gamma invstd' (x - mean') + beta`` plus roundings, so the error of
invstd multiplies ``|x - mean|`` only, the error of the mean ``|gamma| invstd``, and the at most 8 roundings (scale,
mean * gamma, * invstd, shift, x * scale, + shift, + residual; on the PyTorch branch x - mean, invstd * gamma, the
product, + beta, + residual) act on intermediates of at most ``B = |gamma| invstd (|x| + |mean|) + |beta| + |res|``.

Backward (``bwd_ref``): ``dbeta = sum dz``, ``dgamma = invstd (sum dz x - mean sum dz)`` (cancels like the variance:
``invstd (g sum|dz x| + |mean| g sum|dz|)``), ``dx = gamma invstd (dz - dbeta / M - xhat dgamma / M)`` evaluated as
``k1 dz + k2 x + k3``: the errors of dbeta, dgamma, xhat and invstd propagate through the formula, and at most 12
roundings act on ``|gamma| invstd (|dz| + |dbeta| / M + invstd |dgamma| / M (|x| + |mean|))`` (the last factor is the
cancellation of ``k2 x`` against the mean part of ``k3``).  The oracle always uses the fp64 statistics of x; what the
backward is handed (saved fp32 mean / invstd) is within ``emf`` / ``einv`` of them.

An element whose fp64 pre-activation lies within its bound of zero has an undetermined ReLU sign: for it alone the
oracle takes the kernel's decision (``relu_sign``), and at most 0.5 % of a case's elements may be such (asserted on
the oracle alone).  A pooling window is ambiguous when two taps that the kernel cannot see as exactly equal lie
within the bound of the maximum (``stem_pool_ref``); same cap, and the kernel's tap must be one of them.  Exactly
equal taps (the same x in one channel, or all taps rectified to zero) are never ambiguous: the first in scan order
wins.

Observed on the MI355X (the ``NHWC_ERR`` / ``BN_*`` lines of one run of the file; headroom, not tolerances).  Worst
share of its bound per output kind: the bf16 outputs y, dx, dr, dres 1.000 (half a bf16 ulp is the whole bound and
some element always rounds from next to a tie); mean 0.99, invstd 0.47 and dgamma 0.89 where the sums are handed in as
partials and the bound is little more than the final casts; where the kernels sum the rows themselves mean 0.16, invstd
0.28, dgamma 0.71 (five rows: again the casts), dbeta 0.06; scale 0.39, shift 0.27, moving mean 0.31, moving variance
0.31; at eps = 1e-5 invstd 0.31, moving variance 0.31, dgamma 0.58, dbeta 0.02.  The stem: y 1.000, dx 0.999, dgamma
0.73 with the pooled-output statistics (the bf16 reconstruction of x is most of that bound) and 0.15 with the
input-row statistics, dbeta 0.000 either way: some hundred bf16 gradients of like magnitude sum exactly in fp32, so
only the final cast and the add onto the slot round.  The channel with mean 64 and unit spread: its invstd uses at
most 0.013 of the ``k U (1 + mean^2 / var)`` bound when the kernels sum the rows themselves (523 x 24, either eps),
0.22 from hand-made partials (there k = 0 and the bound is the cast of var and the intrinsic): the kernels lose far
less than the form allows, since the row blocks' partial sums are combined in fp64.  Undetermined ReLU signs: at most
2 of 10280 elements of a case; no ambiguous pooling window.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import TINY, U, gamma, half_ulp_bf16, out_bound  # noqa: E402,F401
from optim_helpers import f32  # noqa: E402

EPS = f32(1e-3)
DECAY = f32(0.9)
RSQRT_REL = 2.0 * U * (1.0 + U)       # 1 ulp (HIP math API reference: rsqrtf; CDNA ISA: V_RSQ_F32), or 1 / sqrt
E64 = 2.0 ** -45                      # the fp64 part of a finalize: well under 256 operations of unit 2^-53
CAP = 0.005
BIG = 1e300
CONST = 0.30078125                    # 77 / 256: bf16-representable
# planted channels of every case (C >= 8)
CH_ZERO, CH_CONST, CH_BIG, CH_GNEG, CH_GZERO = 0, 1, 2, 3, 4


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------ inputs
def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def plant(x2, seed):
    """x2 [M, C]: constant 0, constant 77/256, mean 64 with unit spread."""
    x2[:, CH_ZERO] = 0.0
    x2[:, CH_CONST] = CONST
    x2[:, CH_BIG] = NH.bf16_exact(64.0 + NH.randn((x2.shape[0],), seed))
    return x2


def params(C, seed):
    """gamma in [0.5, 1.5) with a negative and a zero channel; beta at least 1/8 from zero (a constant channel's
    output is beta: its ReLU sign must be determined)."""
    g = _rand((C,), seed) + 0.5
    g[CH_GNEG] = -g[CH_GNEG]
    g[CH_GZERO] = 0.0
    b = torch.randn(C, generator=torch.Generator().manual_seed(seed + 1))
    b = torch.where(b < 0, b - 0.125, b + 0.125)
    return g, b


def bn_case(M, C, seed):
    x = plant(NH.bf16_exact(NH.randn((M, C), seed, 2.0) + 0.5), seed + 1)
    g, b = params(C, seed + 2)
    return dict(x=x, g=g, b=b, res=NH.randn((M, C), seed + 4), dy=NH.randn((M, C), seed + 5),
                mm0=NH.randn((C,), seed + 6, 0.5), mv0=_rand((C,), seed + 7) + 0.5,
                dres0=NH.randn((M, C), seed + 8), dg0=NH.randn((C,), seed + 9, 3.0), db0=NH.randn((C,), seed + 10, 3.0))


def split_partials(terms, P, seed, extra=3):
    """[P + extra, C] fp32: slot p holds the fp64 sum of rows p, p + P, ... of ``terms`` rounded to fp32; the rows
    past P are filler the kernels must leave alone.  Returns the buffer, the exact sum of its first P rows and the
    sum of their magnitudes."""
    M, C = terms.shape
    buf = NH.randn((P + extra, C), seed, 5.0) + 1.0
    for p in range(P):
        buf[p] = terms[p::P].sum(0).float() if p < M else 0.0
    head = buf[:P].double()
    return buf, head.sum(0), head.abs().sum(0)


# --------------------------------------------------------------------------------------------------- bit masks
def pack_mask(pos):
    """bit k of byte i = element 8 i + k"""
    b = pos.reshape(-1, 8).to(torch.int32)
    w = (b << torch.arange(8, dtype=torch.int32)).sum(1)
    return w.to(torch.uint8)


def unpack_mask(mask, shape):
    m = mask.detach().cpu().to(torch.int32).reshape(-1, 1)
    return ((m >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(shape)


# ------------------------------------------------------------------------------------------- operation counts
def fin_adds(P):
    """fp32 additions on the longest path of one of the finalize's accumulators (see the module docstring)."""
    if P <= 128:
        return 0
    i, n = 128, 0
    while i + 96 < P:
        n, i = n + 1, i + 128
    return n + (ceil_div(P - i, 32) if P > i else 0)


def reduce_geo(M, C, ws_floats):
    """(row blocks, row groups) of the statistics kernels; the row blocks from the exported workspace size
    ``2 gx C + 4 C``."""
    gx = (int(ws_floats) - 4 * C) // (2 * C)
    assert gx >= 1 and 2 * gx * C + 4 * C == int(ws_floats)
    tpr = 1
    while tpr * 2 <= min(C // 8, 256):
        tpr *= 2
    return gx, 256 // tpr


def rows_k(nrows, W, C, ws_floats):
    """The stem's input-row reduction (C / 8 a power of two): a block sums ``rpb`` image rows, a thread one channel
    vector over pixels w0, w0 + wstep, ... (``wstep = 256 / (C / 8)``): ``rpb ceil(W / wstep)`` sequential additions,
    then the ``wstep`` threads of a channel vector added one after the other, of which only ``min(wstep, W)`` hold
    anything but an exact zero, then the finalize.  The row blocks: at most the statistics kernels'
    (``reduce_geo``) and at most one per image row."""
    gx = min(reduce_geo(nrows * W, C, ws_floats)[0], nrows)
    rpb = ceil_div(nrows, gx)
    gx = ceil_div(nrows, rpb)
    wstep = 256 // (C // 8)
    return rpb * ceil_div(W, wstep) + min(wstep, W) + fin_adds(gx)


def reduce_k(M, C, ws_floats):
    gx, rg = reduce_geo(M, C, ws_floats)
    span = ceil_div(ceil_div(M, gx), rg) * rg
    return ceil_div(min(span, M), rg) + int(math.log2(rg)) + fin_adds(gx)


# -------------------------------------------------------------------------------------------------- statistics
class Stats(object):
    pass


def stats_ref(S, Q, aS, aQ, M, k, eps=EPS, var=None):
    """S, Q: the exact sums (fp64 [C]); aS, aQ: the sums of their terms' magnitudes; k: fp32 additions."""
    st = Stats()
    g = gamma(k) + E64
    st.M = M
    st.mean = S / M
    st.var = (Q / M - st.mean ** 2).clamp(min=0.0) if var is None else var
    st.em = g * aS / M
    st.emf = st.em + U * (st.mean.abs() + st.em)                            # the saved fp32 mean
    st.mu_hi = st.mean.abs() + st.emf
    st.ev = g * aQ / M + 2.0 * st.mean.abs() * st.em + st.em ** 2           # k U (var + mean^2)
    v = st.var + eps
    e_v = st.ev + 2.0 * U * (v + st.ev)                                     # the cast of var, the add of eps
    ok = e_v < 0.5 * v
    st.ok = ok
    rel = torch.where(ok, 0.5 * e_v / (v - e_v).clamp(min=TINY), torch.full_like(v, BIG))
    st.inv = v ** -0.5
    st.einv = st.inv * (rel + RSQRT_REL * (1.0 + rel))
    st.inv_hi = st.inv + st.einv
    return st


def handed_stats(st):
    """For a backward that is HANDED the oracle's mean and invstd cast to fp32: one cast each, and neither the
    forward's summation error nor the intrinsic."""
    h = Stats()
    h.M, h.mean, h.var, h.inv = st.M, st.mean, st.var, st.inv
    h.em = h.ev = torch.zeros_like(st.mean)
    h.emf = U * st.mean.abs()
    h.mu_hi = st.mean.abs() + h.emf
    h.einv = U * st.inv
    h.inv_hi = st.inv + h.einv
    h.ok = torch.ones_like(st.ok)
    return h


def stats_of(x2, k, eps=EPS):
    """From the rows themselves: two-pass variance."""
    x = x2.double()
    M = x.shape[0]
    mean = x.mean(0)
    return stats_ref(x.sum(0), (x * x).sum(0), x.abs().sum(0), (x * x).sum(0), M, k, eps,
                     var=((x - mean) ** 2).mean(0))


def given_stats(mean, var, eps=EPS):
    """Inference: fp32 moving statistics handed in; only the add of eps and the reciprocal square root."""
    st = stats_ref(mean.double(), var.double() + mean.double() ** 2, 0.0 * mean.double(), 0.0 * mean.double(), 1, 0,
                   eps, var=var.double())
    return st


def moving_ref(st, mm0, mv0, decay, one_minus):
    """(moving mean, its bound, moving variance, its bound).  ``one_minus``: the fp32 factor the device forms
    (``1 - fp32(decay)``, exact) or the PyTorch branch passes (``fp32(1 - decay)``).  k = 5: the cast of the unbiased
    variance (or the rounded M / (M - 1) and its product), 1 - decay, the two products, the add."""
    M = st.M
    mm0, mv0 = mm0.double(), mv0.double()
    mmean = decay * mm0 + one_minus * st.mean
    e_mm = one_minus * st.emf + gamma(5) * ((decay * mm0).abs() + one_minus * st.mu_hi)
    f = M / float(max(M - 1, 1))
    unb = st.var * f
    mvar = decay * mv0 + one_minus * unb
    e_mv = one_minus * st.ev * f + gamma(5) * ((decay * mv0).abs() + one_minus * (unb + st.ev * f))
    return mmean, e_mm + TINY, mvar, e_mv + TINY


# ----------------------------------------------------------------------------------------------------- forward
def fwd_ref(x2, st, g, b, res=None):
    """The fp64 pre-activation ``gamma (x - mean) invstd + beta [+ res]`` and the bound of its fp32 value (k = 8)."""
    x = x2.double()
    g, b = g.double(), b.double()
    d = x - st.mean
    pre = g * d * st.inv + b
    B = g.abs() * st.inv_hi * (x.abs() + st.mu_hi) + b.abs()
    if res is not None:
        pre = pre + res.double()
        B = B + res.double().abs()
    acc = g.abs() * (d.abs() * st.einv + st.inv_hi * st.emf) + gamma(8) * B          # k = 8
    return pre, acc


def relu_sign(pre, acc, got_pos, what):
    """[pre > 0], the kernel's own decision where ``|pre| <= acc``; at most CAP of the elements are such."""
    und = pre.abs() <= acc
    n = int(und.sum())
    print("BN_UNDET %-58s %d of %d ReLU signs undetermined (cap %d)" % (what, n, und.numel(), int(CAP * und.numel())))
    assert n <= CAP * und.numel(), "%s: %d of %d ReLU signs undetermined" % (what, n, und.numel())
    return torch.where(und, got_pos.cpu().reshape(pre.shape), pre > 0), und


# ---------------------------------------------------------------------------------------------------- backward
def bwd_ref(x2, dy, pos, st, g, k, sums=None, dres0=None, dg0=None, db0=None, bf=True, e_dz=None, xS=0.0, xSx=0.0,
            dz=None):
    """Every output of the BN backward and its bound.  ``pos``: the ReLU decisions (None: no ReLU); ``sums``:
    (sum dz, sum dz x, sum |.|, sum |.|) taken as given (hand-made partials); ``e_dz``: the bound of an inexact dz
    (the stem's gathered gradient); ``xS`` / ``xSx``: further error of the two sums."""
    x = x2.double()
    M = st.M
    g = g.double()
    if dz is None:
        dz = dy.double() * (pos.double() if pos is not None else 1.0)
    e_dz = torch.zeros_like(dz) if e_dz is None else e_dz
    if sums is None:
        sums = (dz.sum(0), (dz * x).sum(0), dz.abs().sum(0), (dz * x).abs().sum(0))
    Sdz, Sdzx, aS, aSx = sums
    gk = gamma(k) + E64
    e_S = gk * (aS + e_dz.sum(0)) + e_dz.sum(0) + xS
    e_Sx = gk * (aSx + (e_dz * x.abs()).sum(0)) + (e_dz * x.abs()).sum(0) + xSx
    db = Sdz
    edb = e_S + U * (db.abs() + e_S)                                        # the cast to fp32
    core = Sdzx - st.mean * Sdz
    e_core = e_Sx + st.mean.abs() * e_S + st.emf * (Sdz.abs() + e_S)
    dg = core * st.inv
    edg = st.inv_hi * e_core + st.einv * core.abs()
    edg = edg + 2.0 * U * (dg.abs() + edg)                                  # the product with invstd, the cast
    xhat = (x - st.mean) * st.inv
    e_xhat = (x - st.mean).abs() * st.einv + st.inv_hi * st.emf
    t = dz - db / M - xhat * dg / M
    dx = g * st.inv * t
    B = g.abs() * st.inv_hi * (dz.abs() + e_dz + (db.abs() + edb) / M
                               + st.inv_hi * (dg.abs() + edg) / M * (x.abs() + st.mu_hi))
    acc = g.abs() * (st.einv * t.abs() + st.inv_hi * (e_dz + edb / M + (xhat.abs() + e_xhat) * edg / M
                                                      + dg.abs() / M * e_xhat)) + gamma(12) * B    # k = 12
    out = dict(dz=dz, dx=dx, dx_bound=out_bound(dx, acc, bf))
    dg0 = torch.zeros_like(dg) if dg0 is None else dg0.double()
    db0 = torch.zeros_like(db) if db0 is None else db0.double()
    out["dgamma"], out["dbeta"] = dg0 + dg, db0 + db
    out["dg"], out["db"], out["edg"], out["edb"] = dg, db, edg + TINY, edb + TINY
    out["dgamma_bound"] = edg + U * ((dg0 + dg).abs() + edg) + TINY         # the add onto the slot
    out["dbeta_bound"] = edb + U * ((db0 + db).abs() + edb) + TINY
    if dres0 is None:
        out["dres"], out["dres_bound"] = dz, out_bound(dz, e_dz, bf)        # dy or 0: exact
    else:
        out["dres"] = dres0.double() + dz
        out["dres_bound"] = out_bound(out["dres"], gamma(1) * (dres0.double().abs() + dz.abs()) + e_dz, bf)   # k = 1
    return out


# -------------------------------------------------------------------------------------------------------- stem
def stem_pool_ref(z, zacc, key, k, s, padding, got_arg, bf=True):
    """maxpool over z = relu(BN(x)) (fp64 NHWC, each element within ``zacc``).  ``key``: equal for two taps exactly
    when the kernel computes bit-identical values for them.  Returns the pooled reference and bound, the first
    near-maximal tap, the ambiguous windows and whether the kernel's tap is near-maximal."""
    n, h, w, c = z.shape
    fwd = NH.pool_ref(z, k, s, padding, True)
    accw = NH.pool_ref(zacc, k, s, padding, True)["y"]
    top, geo = fwd["y"], fwd["geo"]
    first = torch.full(top.shape, -1, dtype=torch.int64)
    kf = torch.zeros_like(top)
    amb = torch.zeros(top.shape, dtype=torch.bool)
    ingot = torch.zeros(top.shape, dtype=torch.bool)
    got = got_arg.cpu().to(torch.int64) if got_arg is not None else None
    for oh, ow, kh, kw, ih, iw in NH.taps(geo, h, w, k, s):
        tap = kh * k[1] + kw
        near = z[:, ih, iw, :] >= top[:, oh, ow, :] - 2.0 * accw[:, oh, ow, :]
        isfirst = near & (first[:, oh, ow, :] < 0)
        first[:, oh, ow, :] = torch.where(isfirst, torch.full_like(first[:, oh, ow, :], tap), first[:, oh, ow, :])
        kf[:, oh, ow, :] = torch.where(isfirst, key[:, ih, iw, :], kf[:, oh, ow, :])
        amb[:, oh, ow, :] |= near & ~isfirst & (key[:, ih, iw, :] != kf[:, oh, ow, :])
        if got is not None:
            ingot[:, oh, ow, :] |= near & (got[:, oh, ow, :] == tap)
    arg = first if got is None else torch.where(amb, got, first)
    return dict(y=top, y_bound=out_bound(top, accw, bf), first=first, amb=amb, ingot=ingot, arg=arg, geo=geo,
                cnt=fwd["cnt"])
