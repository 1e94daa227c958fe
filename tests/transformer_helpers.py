"""Shared pieces of ``tests/test_transformer_kernels.py``: fp64 oracles of the row kernels of ``csrc/transformer.hip``
(LayerNorm with the fused dropout and residual, its backward, the masked scaled softmax and its backward, the
embedding gather / scatter-add and the three-table BERT sum) written from the definitions, and the elementwise bounds
they are compared under.  Nothing here imports ``mdtf.ops``: the dropout counter hash is restated in numpy.  The
comparisons (``check_bound``, ``check_neighbour``), the seeded inputs and the sentinel-guarded buffers are those of
``nhwc_helpers``; ``check`` / ``check_nb`` add the ``TRF_ERR`` / ``TRF_NB`` line of this suite.

Conventions.  ``U = 2^-24``; ``gamma(k) = kU / (1 - kU)`` bounds k fp32 roundings on the longest path from the inputs
to a value, relative to the absolute sum of the terms below it.  ``chain(n, lanes)`` is the longest path of a row sum
of n terms: on the device a lane adds its ``8 * ceil(n / (8 lanes))`` terms in sequence and the lanes merge in
``log2(lanes)`` shuffle steps; on the CPU the order is ATen's, so n (any order) stands in.  Scalar arguments
(``eps``, ``p``, ``scale``) are rounded to fp32 first, as a kernel's ``float`` argument is.

LayerNorm forward (``ln_fwd_bounds``).  The residual sum s carries ``e_s`` (the product with 1 / (1 - p) and the
add).  mean: ``e_s`` averaged + the sum's roundings.  var (two passes): with d = s - mean exact, a computed
d' = d + a + c, |a| <= e_s + U |d| per element and |c| <= e_mean per row, gives
var' - var = 2 mean(d a) + mean((a + c)^2) (the cross term with c vanishes: sum d = 0) + the sum's roundings.
rstd = (var + eps)^-1/2 moves by ``rstd * e_v / (2 (v - e_v))`` for an error e_v of v = var + eps, and by the
``rsqrtf`` intrinsic's own error, which cannot be derived: see the measured constant below.
y = d rstd gamma + beta: ``|gamma| (rstd (a + c) + |d| e_rstd)``, the conditioning term (absolute: a bound relative to
y would be wrong near xhat = 0), + three roundings over ``|d| rstd |gamma| + |beta|``, then the rounding to bf16.

LayerNorm backward, raw (``ln_bwd_raw_bounds``): s (bf16), mean and rstd (fp32) are inputs, the oracle uses the same
values, and the kernel is a pure function of them: only roundoff over
``T = rstd (|g| + mean|g| + |xhat| mean|g xhat|)``, g = dy gamma, and the bf16 rounding of dx.  dgamma / dbeta: fp32
sums over the rows in any order, into the slot.

LayerNorm backward through autograd (``ln_bwd_autograd_bounds``) against fp64 autograd of the true function: the
kernel normalises the bf16-SAVED s with the statistics of the unrounded sum (the design's own approximation),
``d_xhat = rstd (half_ulp_bf16(s) + e_s + e_mean) + |d| e_rstd``, propagated through dx, dgamma; the share of the
bound that the ``rstd * half_ulp_bf16(s)`` term is responsible for is printed with every check.

The CPU branch (``F.layer_norm``) evaluates algebraically different forms: y = s (rstd gamma) + (beta - mean rstd
gamma) and dx = a dy gamma + b s + c with b, c from the uncentred sums sum(g s), sum(g).  Their roundings are relative
to the uncentred terms (|s| + |mean| in place of |d|); ``aten=True`` adds exactly those terms, so a row whose mean is
large against its spread is checked on the CPU under the bound of the form the CPU evaluates, and on the device under
the centred form's.

Softmax forward: ``check_neighbour`` with its 1 % cap.  For a row whose every key is masked the oracle's input is the
fp32-rounded logit ``fl(scale * x + mask)``: TF and the kernel both add in fp32, and at -10000 one fp32 ulp is about
1e-3, so against the true fp64 logits 1.5 % to 5.8 % of such rows' elements are the neighbour at scale 0.125 (over
the cap; up to 0.26 % at scale 1) and against the fp32-rounded logits at most 0.01 % (the CPU branch on the ``full``
inputs of ``softmax_inputs``, cols = 8, 40, 128, 520, 1024; every other row: none either way).  Backward: at the
saved bf16 y only roundoff; against the true gradient ``dp = half_ulp_bf16(p) + roundoff`` is propagated through
``scale p (dy - sum dy p)``.

Embedding: the gather is bitwise; a table-gradient element is an fp32 sum of its ``count`` addends in any order
(``gamma(count + 1)`` with the slot), rows no id selects keep their prior content exactly.

Measured constants (CPU, fp32 ``torch.native_layer_norm`` -- what ``F.layer_norm`` calls -- against the fp64 oracle,
over every LayerNorm input ``test_transformer_kernels.py`` builds):

* rstd: at most 2.82 units of ``U * rstd`` (37 x 8 with a residual; most shapes reach 1.6 to 2.1), over the rows
  whose mean lies within 4 standard deviations of 0: beyond that (the constant rows and the 1000 +- 8 row, 12 units)
  ATen's merge of per-chunk moments sets the error, not the reciprocal square root, and the ``aten`` term of the
  bound covers it.  ``RSTD_UNITS_CPU`` = 3 is the figure rounded up to a whole unit.  The tests on ``cpu`` assert it
  again; the kernel's ``rsqrtf`` gets ``INTRINSIC_FACTOR`` (8) times it on top of the derived terms.

Largest shares of the bounds on the MI355X (``TRF_ERR`` lines; the default forms and the four env-selected forms
alike).  Every bf16 output reaches 1.000 (or 0.97 to 0.999) of its bound, since the bound of an element is half a
bf16 ulp plus a far smaller fp32 term and some element always rounds from next to a tie: LayerNorm y, s, dx,
dx_branch, softmax dx, the BERT sum, the bf16 table gradients.  The fp32 outputs: LayerNorm mean 0.032, rstd 0.070,
dgamma 0.040 raw (0.179 at H = 8192 with atomics; 1.000 through autograd at one row, where the bf16-saved s is the
whole bound), dbeta 0.048; table gradients into fp32 slots 0.202.  Softmax forward: at most 0.013 % of the elements
of a case are the neighbour (cap 1 %).
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nhwc_helpers import (INTRINSIC_FACTOR, TINY, U, Guarded, assert_contained, bf16_exact,  # noqa: E402,F401
                          bits_equal, check_bound, check_neighbour, gamma, half_ulp_bf16, out_bound, put, randn,
                          round_bf16)
from optim_helpers import f32  # noqa: E402

RSTD_UNITS_CPU = 3.0
EPS = f32(1e-12)
BIG = 1e300


def check(got, ref, bound, what):
    r = check_bound(got, ref, bound, what)
    print("TRF_ERR %-62s max %.3f of its bound" % (what, r))
    return r


def check_nb(got, ref, what, cap=0.01):
    n = check_neighbour(got, ref, what, cap)
    print("TRF_NB  %-62s %d of %d elements are the neighbour" % (what, n, ref.numel()))
    return n


def chain(n, lanes, device):
    """Longest path of a sum of n terms (module docstring)."""
    if device == "cpu":
        return n
    return 8 * -(-n // (8 * lanes)) + int(math.log2(lanes))


def ln_lanes(H):
    """Lanes per row of the LayerNorm kernels (LN_DISPATCH)."""
    nvec = H // 8
    return 32 if (nvec % 64 != 0 and nvec % 32 == 0 and nvec // 32 <= 3) else 64


# ------------------------------------------------------------------------------------------------------ dropout
def hash_keep(seed, n, p):
    """Keep bits of elements 0..n-1: the counter hash of ``drop_keep`` with threshold floor(fl32(p) * 2^32)."""
    idx = np.arange(n, dtype=np.uint64).astype(np.uint32)
    x = (idx * np.uint32(0x9E3779B1)) ^ np.uint32(seed)
    x ^= x >> np.uint32(16)
    x = x * np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x = x * np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return torch.from_numpy(x >= np.uint32(min(int(f32(p) * 4294967296.0), 4294967295)))


# ---------------------------------------------------------------------------------------------------- LayerNorm
def ln_inputs(rows, H, seed, with_res):
    """x, res, gamma, beta, dy.  x and res are bf16-representable and off centre (mean about 0.4 against a spread
    of about 1), gamma holds zeros and negative values, dy a zero row."""
    x = bf16_exact(randn((rows, H), seed) + 0.25)
    res = bf16_exact(randn((rows, H), seed + 1, 0.5) + 0.125) if with_res else None
    gen = torch.Generator().manual_seed(seed + 2)
    g = 1.0 + 0.5 * torch.randn(H, generator=gen)
    g[1::5] = 0.0
    b = 0.5 * torch.randn(H, generator=gen)
    dy = randn((rows, H), seed + 3)
    if rows >= 3:
        dy[1] = 0.0
    return x, res, g, b, dy


def ln_edge_inputs(H, seed):
    """Rows: all 2.0 (every partial sum exact in fp32) | 1000 +- {0, 4, 8} (bf16-exact, mean large against the
    spread) | zeros | random.  beta is bf16-representable so that the constant rows give y == beta exactly."""
    gen = torch.Generator().manual_seed(seed)
    x = randn((4, H), seed + 1)
    x[0] = 2.0
    x[1] = 1000.0 + 4.0 * torch.randint(-2, 3, (H,), generator=gen).float()
    x[2] = 0.0
    g = 1.0 + 0.5 * torch.randn(H, generator=gen)
    g[1::5] = 0.0
    b = bf16_exact(0.5 * torch.randn(H, generator=gen))
    dy = randn((4, H), seed + 2)
    return bf16_exact(x), None, g, b, dy


def ln_fwd_ref(x, res, g, b, keep=None, p=0.0, eps=EPS):
    """s = keep x / (1 - p) + res, two-pass mean and variance, y = (s - mean) rstd gamma + beta; all fp64."""
    br = x.double()
    if keep is not None:
        br = keep.double() * br / (1.0 - f32(p))
    r64 = res.double() if res is not None else torch.zeros_like(br)
    s = br + r64
    mean = s.mean(1)
    d = s - mean[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd[:, None] * g.double() + b.double()
    return dict(s=s, br=br, res=r64, mean=mean, d=d, var=var, rstd=rstd, y=y, eps=eps,
                drop=keep is not None, has_res=res is not None)


def ln_fwd_bounds(ref, g, b, device, aten=False):
    """Bounds of s, mean, rstd, y (module docstring); ``e_*`` are the fp32 values' errors before any bf16 store."""
    bf = device != "cpu"
    H = ref["s"].shape[1]
    c = chain(H, ln_lanes(H), device)
    # k: p -> 1 - p, the reciprocal and the product (3) with dropout, the add of the residual (1)
    ks = (3 if ref["drop"] else 0) + (1 if ref["has_res"] else 0)
    e_s = gamma(ks) * (ref["br"].abs() + ref["res"].abs()) if ks else torch.zeros_like(ref["s"])
    sabs = ref["s"].abs() + e_s
    # k = chain + 1: the row sum and the division by H
    e_mean = e_s.mean(1) + gamma(c + 1) * sabs.mean(1)
    d, var, rstd = ref["d"], ref["var"], ref["rstd"]
    a = e_s + U * (d.abs() + e_s + e_mean[:, None])                       # the subtraction's own rounding
    ac = a + e_mean[:, None]
    dv = 2.0 * (d.abs() * a).mean(1) + (ac * ac).mean(1)
    # k = chain + 3: d (counted in a), the square, the row sum, the division by H
    e_var = dv + gamma(c + 3) * (var + dv)
    if aten:
        # ATen merges per-chunk (mean, m2) pairs: the difference of two chunk means, each off by its own roundoff
        # relative to |mean|, enters m2 squared and against the chunks' spread
        em = gamma(c + 1) * sabs.mean(1)
        e_var = e_var + 2.0 * torch.sqrt(var) * em + em * em
    v = var + ref["eps"]
    e_v = e_var + U * v                                                    # the add of eps
    ok = e_v < 0.5 * v
    rel = torch.where(ok, 0.5 * e_v / (v - e_v).clamp(min=TINY), torch.full_like(v, BIG))
    units = RSTD_UNITS_CPU * (INTRINSIC_FACTOR if bf else 1.0)
    e_rstd = rstd * (rel + units * U)
    ga, ba = g.double().abs(), b.double().abs()
    cond = ga * (rstd[:, None] * ac + d.abs() * e_rstd[:, None] + ac * e_rstd[:, None])
    t = d.abs() * rstd[:, None] * ga + ba
    if aten:
        t = (ref["s"].abs() + ref["mean"].abs()[:, None]) * rstd[:, None] * ga + ba
    # k = 3: the product with rstd, the product with gamma, the add of beta (the CPU form: scale, shift, fma: 4)
    e_y = cond + gamma(4 if aten else 3) * (t + cond)
    return dict(e_s=e_s, e_mean=e_mean, e_rstd=e_rstd, e_y=e_y, ac=ac,
                s=out_bound(ref["s"], e_s, bf), mean=e_mean + TINY, rstd=e_rstd, y=out_bound(ref["y"], e_y, bf))


def ln_bwd_ref(dy, s, mean, rstd, g, keep=None, p=0.0, dg0=None, db0=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; dgamma = sum_rows dy xhat, dbeta = sum_rows dy (onto
    the slots' prior content); dx_branch = keep dx / (1 - p).  All arguments are taken as they are (fp64)."""
    dy, s, g = dy.double(), s.double(), g.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    xh = (s - mean) * rstd
    gg = dy * g
    a, b = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    dx = rstd * (gg - a - xh * b)
    T = rstd * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
    H = s.shape[1]
    dg0 = dg0.double() if dg0 is not None else torch.zeros(H, dtype=torch.float64)
    db0 = db0.double() if db0 is not None else torch.zeros(H, dtype=torch.float64)
    out = dict(dx=dx, T=T, xh=xh, gg=gg, b=b, rstd=rstd, dgamma=(dy * xh).sum(0) + dg0, dbeta=dy.sum(0) + db0,
               Tg=(dy * xh).abs().sum(0) + dg0.abs(), Tb=dy.abs().sum(0) + db0.abs(), dy=dy, p=f32(p))
    out["dxb"] = (keep.double() if keep is not None else 1.0) * dx / (1.0 - f32(p))
    return out


def ln_bwd_raw_bounds(ref, blocks, device, bf=True):
    rows, H = ref["dx"].shape
    c = chain(H, ln_lanes(H), device)
    # k = chain + 8: xhat (2), g (1), g xhat (1), the row sum, / H (1), xhat b (1), the two subtractions (2), rstd (1)
    # (one more than the longest path: the two sums' paths are not added)
    e_dx = gamma(c + 8) * ref["T"]
    # k = 3: 1 - p, the reciprocal, the product
    e_dxb = (e_dx * (1.0 + gamma(3)) + gamma(3) * ref["dx"].abs()) / (1.0 - ref["p"])
    # k = rows + blocks + 1: the rows in any order, the blocks' partials, the add onto the slot; + 3 for dgamma: each
    # term dy xhat is itself three roundings from the inputs
    kg = rows + blocks + 1
    return dict(e_dx=e_dx, dx=out_bound(ref["dx"], e_dx, bf), dxb=out_bound(ref["dxb"], e_dxb, bf),
                dgamma=gamma(kg + 3) * ref["Tg"] + TINY, dbeta=gamma(kg) * ref["Tb"] + TINY)


def ln_autograd_ref(x, res, g, b, dy, keep=None, p=0.0, dg0=None, db0=None, eps=EPS):
    """fp64 autograd of y = LN(keep x / (1 - p) + res): y, dx (the branch input's), dres, dgamma, dbeta."""
    x64 = x.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if res is not None else None
    g64, b64 = g.double().requires_grad_(True), b.double().requires_grad_(True)
    br = x64 if keep is None else keep.double() * x64 / (1.0 - f32(p))
    s = br if r64 is None else br + r64
    mean = s.mean(1, keepdim=True)
    d = s - mean
    y = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * g64 + b64
    ins = [x64, g64, b64] + ([r64] if r64 is not None else [])
    gr = torch.autograd.grad((y * dy.double()).sum(), ins)
    H = x.shape[1]
    dg0 = dg0.double() if dg0 is not None else torch.zeros(H, dtype=torch.float64)
    db0 = db0.double() if db0 is not None else torch.zeros(H, dtype=torch.float64)
    return dict(y=y.detach(), dx=gr[0], dgamma=gr[1] + dg0, dbeta=gr[2] + db0, dres=gr[3] if r64 is not None else None)


def ln_bwd_autograd_bounds(fref, fb, g, dy, blocks, device, aten=False, dg0=None, db0=None, saved_term=True):
    """Bounds of the backward that starts from what the forward saved (module docstring).  ``fref`` / ``fb``: the
    forward's oracle and bounds.  Returns the bounds and the true-input quantities they were built from."""
    bf = device != "cpu"
    rows, H = fref["s"].shape
    r = ln_bwd_ref(dy, fref["s"], fref["mean"], fref["rstd"], g, None, 0.0, dg0, db0)      # at the TRUE s, mean, rstd
    raw = ln_bwd_raw_bounds(r, blocks, device, bf)
    rstd, e_rstd = r["rstd"], fb["e_rstd"][:, None]
    # the saved s: exact when the sum itself is (no dropout, no residual: s = x), else the unrounded sum's error and,
    # on the device, its rounding to bf16
    exact = torch.zeros_like(fref["s"])
    e_saved = fb["e_s"] + (half_ulp_bf16(fref["s"].abs() + fb["e_s"]) if (bf and saved_term) else 0.0)
    if not (fref["drop"] or fref["has_res"]):
        e_saved = exact
    dxh = rstd * (e_saved + fb["e_mean"][:, None] + U * fref["d"].abs()) + fref["d"].abs() * e_rstd
    gg, xh = r["gg"], r["xh"]
    db_ = (gg.abs() * dxh).mean(1, keepdim=True)
    inner = gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True)
    e_dx = raw["e_dx"] * (1.0 + e_rstd / rstd) + e_rstd * inner + (rstd + e_rstd) * (
        dxh * (r["b"].abs() + db_) + xh.abs() * db_)
    if aten:
        # dx = a dy gamma + b s + c, b = (sum(g) mean - sum(g s)) rstd^3 / H, c = -b mean - sum(g) rstd / H: roundings
        # relative to the uncentred terms
        s_, m_ = fref["s"].abs(), fref["mean"].abs()[:, None]
        B = rstd ** 3 * (m_ * gg.abs().mean(1, keepdim=True) + (gg.abs() * s_).mean(1, keepdim=True))
        e_dx = e_dx + gamma(H + 12) * (rstd * gg.abs() + B * (s_ + m_) + rstd * gg.abs().mean(1, keepdim=True))
    kg = rows + blocks + 1
    e_dg = (r["dy"].abs() * dxh).sum(0) * (1.0 + gamma(kg + 3)) + raw["dgamma"]
    return dict(dx=out_bound(r["dx"], e_dx, bf), e_dx=e_dx, dgamma=e_dg, dbeta=raw["dbeta"], ref=r)


# ------------------------------------------------------------------------------------------------------ softmax
NEG = -10000.0


def softmax_inputs(B, heads, sq, cols, seed, mask_kind):
    """scores [B, heads, sq, cols] (row 0: one logit 30 above the rest; row 1: equal logits), mask [B, cols] or None
    (``sparse``: about a third of the keys of every batch masked, key 0 never; ``full``: batch 1 entirely), dy."""
    x = randn((B, heads, sq, cols), seed, 3.0)
    x[0, 0, 0] = bf16_exact(x[0, 0, 0] * 0.25)
    x[0, 0, 0, cols // 2] = 30.0
    x[0, 0, 1] = 1.5
    dy = randn((B, heads, sq, cols), seed + 1)
    mask = None
    if mask_kind != "none":
        gen = torch.Generator().manual_seed(seed + 2)
        mask = torch.where(torch.rand((B, cols), generator=gen) < 0.33, torch.tensor(NEG), torch.tensor(0.0))
        mask[:, 0] = 0.0
        if mask_kind == "full":
            mask[1] = NEG
    return x, mask, dy


def softmax_ref(x, mask, scale):
    """softmax(scale x + mask[b]) in fp64; rows whose every key is masked take the fp32-rounded logits (module
    docstring)."""
    scale = f32(scale)
    z = x.double() * scale
    if mask is not None:
        z = z + mask.double()[:, None, None, :]
        full = (mask <= NEG).all(1)
        z32 = (x.float() * scale + mask.float()[:, None, None, :]).double()
        z = torch.where(full[:, None, None, None], z32, z)
    z = z - z.max(-1, keepdim=True).values
    e = torch.exp(z)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd_ref(p, dy, scale):
    """scale p (dy - sum(dy p)) and the absolute sum of its terms."""
    p, dy, scale = p.double(), dy.double(), f32(scale)
    D = (dy * p).sum(-1, keepdim=True)
    return scale * p * (dy - D), scale * p * (dy.abs() + (dy * p).abs().sum(-1, keepdim=True)), D


def softmax_bwd_bounds(p, dy, scale, device, true_p):
    """At the saved y (``true_p`` False): k = chain + 4 (the products dy p, the row sum, the subtraction, the two
    products).  Against the true gradient: dp = half_ulp_bf16(p) (the saved y is bf16 on the device) + the forward's
    own roundoff, through scale (p (dy - D)): scale (dp |dy - D| + (p + dp) sum |dy| dp)."""
    bf = device != "cpu"
    cols = p.shape[-1]
    c = chain(cols, 64, device)
    ref, T, D = softmax_bwd_ref(p, dy, scale)
    acc = gamma(c + 4) * T
    if true_p:
        p, dy = p.double(), dy.double()
        # the forward's fp32 error: the exponentials (INTRINSIC_FACTOR units each way), the sum, the reciprocal and
        # the product
        dp = (half_ulp_bf16(p) if bf else 0.0) + (gamma(c + 3) + 2 * INTRINSIC_FACTOR * U) * p
        dD = (dy.abs() * dp).sum(-1, keepdim=True)
        acc = acc * (1.0 + 2.0 ** -7) + f32(scale) * (dp * (dy - D).abs() + (p + dp) * dD)
    return ref, out_bound(ref, acc, bf)


# ---------------------------------------------------------------------------------------------------- embedding
def embed_inputs(vocab, n, H, seed, bad_ids):
    """table (with a -0.0 and a +0.0), ids (40 % of the tokens on one row; ``bad_ids``: a -1 and a ``vocab``), dy."""
    table = randn((vocab, H), seed)
    table[0, 0] = -0.0
    table[vocab - 1, H - 1] = 0.0
    gen = torch.Generator().manual_seed(seed + 1)
    ids = torch.randint(0, vocab, (n,), generator=gen)
    hot = min(1, vocab - 1)
    ids[torch.rand(n, generator=gen) < 0.4] = hot
    if vocab > 4 and n > 1:
        ids[ids == 3] = 2                            # row 3: no id selects it
    if bad_ids and n >= 8:
        ids[2], ids[7] = -1, vocab
    return table, ids, randn((n, H), seed + 2)


def embed_fwd_ref(table, ids):
    """Rows of the table; a zero row for an id outside [0, vocab)."""
    ok = (ids >= 0) & (ids < table.shape[0])
    out = table[ids.clamp(0, table.shape[0] - 1)].clone()
    out[~ok] = 0.0
    return out


def embed_bwd_ref(dy, ids, vocab, slot0=None):
    """(dtable, sum|terms|, count per row); ids outside [0, vocab) add nothing."""
    H = dy.shape[-1]
    dy, ids = dy.double().reshape(-1, H), ids.reshape(-1)
    ok = (ids >= 0) & (ids < vocab)
    s0 = slot0.double() if slot0 is not None else torch.zeros((vocab, H), dtype=torch.float64)
    dt = s0.clone().index_add_(0, ids[ok], dy[ok])
    ab = s0.abs().index_add_(0, ids[ok], dy[ok].abs())
    cnt = torch.zeros(vocab, dtype=torch.float64).index_add_(0, ids[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    return dt, ab, cnt


def check_embed_bwd(got, dy, ids, vocab, what, slot0=None, bf16_out=False):
    """k = count + 1 per table row: its addends in any order and the add onto the slot; rows without an addend keep
    the slot's content exactly."""
    dt, ab, cnt = embed_bwd_ref(dy, ids, vocab, slot0)
    check(got, dt, out_bound(dt, gamma(cnt + 1)[:, None] * ab, bf16_out), what)
    idle = cnt == 0
    g = got.detach().cpu().double()
    assert torch.equal(g[idle], dt[idle]), "%s: a table row that no id selects changed" % what


def bert_inputs(B, S, H, vocab, npos, ntypes, seed, bad):
    word, pos, typ = randn((vocab, H), seed), randn((npos, H), seed + 1), randn((ntypes, H), seed + 2)
    gen = torch.Generator().manual_seed(seed + 3)
    ids = torch.randint(0, vocab, (B, S), generator=gen)
    types = torch.randint(0, ntypes, (B, S), generator=gen)
    if bad:
        types[0, 1] = ntypes
        types[B - 1, S - 1] = -1
        ids[0, 2] = vocab
    return word, pos, typ, ids, types, randn((B, S, H), seed + 4)


def bert_fwd_ref(word, pos, typ, ids, types):
    """word[ids] + pos[s] + typ[types] in fp64 and the absolute sum of the three terms."""
    B, S = ids.shape
    w = embed_fwd_ref(word.double(), ids.reshape(-1)).view(B, S, -1)
    t = embed_fwd_ref(typ.double(), types.reshape(-1)).view(B, S, -1)
    p = pos.double()[:S][None]
    return w + p + t, w.abs() + p.abs() + t.abs()
