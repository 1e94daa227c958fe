"""Shared pieces of the fused-optimizer tests (``tests/test_optim_kernels.py``): an fp64 reference of sgd, momentum
and Adam written from the formulas of ``tf.train.{GradientDescent,Momentum,Adam}Optimizer`` (it never calls
``mdtf.ops.optim``), the per-element error bound it is compared under, seeded inputs and sentinel-guarded buffers.

The bound.  Every fp32 operation rounds its result by at most ``U = 2^-24`` relative.  An output is a sum of terms
(``w``, ``lr*g*gs``, ``lr*wd*w`` ...); a rounding anywhere in the expression is at most ``U`` times the absolute sum of
the terms below it, so the whole error is at most ``U * sum_t |t| * depth(t)`` with ``depth(t)`` the number of
roundings between term ``t`` and the output.  Hence

    |got - ref| <= K * U * scale + TINY,    scale = sum of |terms| BEFORE any cancellation,  K = longest path.

(``gamma(K) = K*U / (1 - K*U)`` replaces ``K*U``: the first-order count made rigorous.)  Hyper-parameters are rounded
to fp32 first, as the kernels' ``float`` arguments are, so they carry no error of their own; ``1 - beta`` is formed
from the fp32 ``beta`` as the kernels and TF's fp32 ``ApplyAdam`` do.

Sequential updates (five steps, ``apply_multi_``) feed each step the scales of the previous one instead of ``|w|``,
``|m|`` ...: the scale stays the absolute sum over the whole expression, every step adds at most the single-step
``K`` of ``w`` to the longest path, and ``k`` steps are checked under ``k * K_w``.
"""
import math

import torch

U = 2.0 ** -24                  # fp32 unit roundoff (round to nearest)
TINY = 2.0 ** -149              # one fp32 denormal: slack for a result that underflows

# ---- K per output: roundings on the longest path of ONE update from exact inputs.  g~ = g*gs + wd*w is
# [g*gs (1) | wd*w (1)], the add (2): depth 2.
# sgd       w:   g~ (2), lr * (3), w - (4)
K_SGD = {"w": 4}
# momentum  acc: g~ (2), [mom*acc (1)] the add (3)
#           w:   acc (3), lr * (4), w - (5);  nesterov: acc (3), mom * (4), g~ + (5), lr * (6), w - (7)
K_MOMENTUM = {"acc": 3, "w": 5}
K_NESTEROV = {"acc": 3, "w": 7}
# adam      m:   g~ (2), (1-b1) * (3), [b1*m (1)] the add (4)
#           v:   the term is (1-b2)*g~*g~; its error is (1-b2) * (2|g~| e_g + 2 roundings of the two products)
#                <= (depth(g~) + 1) * U * 2(1-b2) |g~| S_g with S_g the scale of g~: the square's derivative puts
#                2 |g~| S_g in the SCALE (not S_g^2: over several steps S_g^2 feeds on itself through wd*w) and leaves
#                depth 2 + 1 = 3, the add (4)
#           w:   upd = lr_t * m / (sqrt(v) + eps).  den = sqrt(v) + eps: |sqrt(v + e) - sqrt(v)| <= e / sqrt(v), so
#                sqrt(v) has scale S_v / sqrt(v) at depth 4, + its own rounding and the add of eps (2 roundings of at
#                most den each): depth 6 over the scale S_den = S_v / sqrt(v) + den.  upd then has the two parts
#                X = lr_t * S_m / den (depth 4) and Y = |upd| * S_den / den (depth 6), + the product and the
#                quotient (2): depth 8 over X + Y; + lr*wd*w when decoupled (9) [that term itself: lr*wd formed in
#                double and rounded once by the torch branch, twice by the kernel (<= 3), * w (4), the add (5)],
#                w - (10)
K_ADAM = {"m": 4, "v": 4, "w": 10}


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(x):
    """A Python float rounded to fp32 (what a kernel's float argument holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def adam_lr_t(lr, b1, b2, step, bias_correction=True):
    """tf.train.AdamOptimizer: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), t counting from 1 (host side, in double)."""
    if not bias_correction:
        return lr
    return lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)


# ------------------------------------------------------------------------------------------------ the reference
def start(**tensors):
    """The reference's state: name -> [fp64 value, fp64 scale] from fp32 tensors (w, and acc or m, v).  ``cond``
    (Adam) records the largest depth * S_v / v met (depth: K_w times the number of the step): where it is huge,
    g*gs and wd*w cancelled almost exactly and the first-order bound on 1 / (sqrt(v) + eps) does not hold
    (``check`` exempts those few elements)."""
    st = {k: [t.detach().cpu().double().clone(), t.detach().cpu().double().abs()] for k, t in tensors.items()}
    st["cond"] = torch.zeros_like(st["w"][0])
    st["steps"] = 0
    return st


def _gtilde(st, g, gs, wd):
    w, sw = st["w"]
    g = g.detach().cpu().double() * gs
    sg = g.abs()
    if wd:
        g = g + wd * w
        sg = sg + abs(wd) * sw
    return g, sg


def sgd_step(st, g, lr, gs=1.0, wd=0.0):
    """w -= lr * (g*gs + wd*w)"""
    lr, gs, wd = f32(lr), f32(gs), f32(wd)
    w, sw = st["w"]
    g, sg = _gtilde(st, g, gs, wd)
    st["w"] = [w - lr * g, sw + abs(lr) * sg]


def momentum_step(st, g, lr, mom, gs=1.0, wd=0.0, nesterov=False):
    """acc = mom*acc + g~;  w -= lr*acc  (nesterov: w -= lr*(g~ + mom*acc), acc the NEW accumulator)"""
    lr, mom, gs, wd = f32(lr), f32(mom), f32(gs), f32(wd)
    w, sw = st["w"]
    a, sa = st["acc"]
    g, sg = _gtilde(st, g, gs, wd)
    a, sa = mom * a + g, abs(mom) * sa + sg
    st["acc"] = [a, sa]
    if nesterov:
        st["w"] = [w - lr * (g + mom * a), sw + abs(lr) * (sg + abs(mom) * sa)]
    else:
        st["w"] = [w - lr * a, sw + abs(lr) * sa]


def adam_step(st, g, lr, lr_t, b1, b2, eps, gs=1.0, wd=0.0, decoupled=False):
    """m = b1*m + (1-b1)*g~;  v = b2*v + (1-b2)*g~^2;  w -= lr_t * m / (sqrt(v) + eps)  [+ lr*wd*w decoupled, and
    then g~ = g*gs without the decay term]"""
    lr, lr_t, b1, b2, eps, gs, wd = (f32(x) for x in (lr, lr_t, b1, b2, eps, gs, wd))
    c1, c2 = 1.0 - b1, 1.0 - b2                         # exact in fp32 for beta >= 0.5
    w, sw = st["w"]
    m, sm = st["m"]
    v, sv = st["v"]
    g, sg = _gtilde(st, g, gs, 0.0 if decoupled else wd)
    m, sm = b1 * m + c1 * g, b1 * sm + c1 * sg
    v, sv = b2 * v + c2 * g * g, b2 * sv + 2.0 * c2 * g.abs() * sg
    st["m"], st["v"] = [m, sm], [v, sv]
    rt = v.sqrt()
    den = rt + eps
    upd = lr_t * m / den
    s_sqrt = torch.where(sv > 0, sv / rt, torch.zeros_like(sv))
    s_upd = abs(lr_t) * sm / den + upd.abs() * (s_sqrt + den) / den
    st["steps"] += 1
    cond = st["steps"] * K_ADAM["w"] * torch.where(sv > 0, sv / v, torch.zeros_like(sv))
    st["cond"] = torch.maximum(st["cond"], cond)
    if decoupled and wd:
        upd = upd + lr * wd * w
        s_upd = s_upd + abs(lr * wd) * sw
    st["w"] = [w - upd, sw + s_upd]


def check(got, st, name, k, what, exempt_ok=None):
    """Elementwise ``|got - ref| <= gamma(k) * scale + TINY`` wherever the reference is finite; non-finite exactly
    where the reference is.  Prints and returns the largest error in units of ``U * scale``."""
    ref, scale = st[name]
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    where = lambda mask: mask.nonzero().flatten()[:8].tolist()                            # noqa: E731
    assert torch.equal(torch.isfinite(got), fin), \
        "%s %s: non-finite at %s, reference at %s" % (what, name, where(~torch.isfinite(got)), where(~fin))
    exempt = torch.zeros_like(fin)
    if name == "w" and "m" in st:
        # 1 / den is bounded to first order: its relative error depth * U * S_v / v must stay small (2^-6 here,
        # which the factor below gives back); elements past that are the near-exact cancellations of g*gs + wd*w
        exempt = fin & ~(U * st["cond"] <= 2.0 ** -6)
        # (at depth 10 that takes |g*gs + wd*w| < 2^-6.8 of |g*gs| + |wd*w|: well under 1 % of random elements)
        allowed = 1 + ref.numel() // 200 if exempt_ok is None else exempt_ok
        assert int(exempt.sum()) <= allowed, (what, int(exempt.sum()), ref.numel())
    cmp = fin & ~exempt
    err = (got - ref).abs()[cmp]
    sc = scale[cmp]
    bound = gamma(k) * (1.0 + 2.0 ** -5) * sc + TINY
    units = float((err / (U * sc + TINY)).max()) if err.numel() else 0.0
    print("OPTIM_ERR %-44s %-3s K=%-3d max %.3f units of 2^-24*scale, %d exempt" % (what, name, k, units,
                                                                                  int(exempt.sum())))
    bad = ~(err <= bound)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError("%s %s: %d of %d elements off; first at %d: err %.6g bound %.6g (%.2f units, K=%d)" % (
            what, name, int(bad.sum()), err.numel(), int(cmp.nonzero().flatten()[i]), float(err[i]), float(bound[i]),
            float(err[i] / (U * sc[i] + TINY)), k))
    return units


# ------------------------------------------------------------------------------------------------------ inputs
MAGS = (1e-3, 1.0, 1e3)         # gradient magnitudes, mixed element by element


def make_inputs(n, seed, k=1, zero_state=False, g_dtype=torch.float32):
    """CPU tensors: w, k gradients, acc / m / v of matching magnitude.  Gradient magnitudes cycle through MAGS
    element by element (|g*gs| <= ~5e3: g*g stays far inside fp32); exact zeros sit in g, acc, m and v."""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.tensor(MAGS)[torch.arange(n) % 3]
    w = torch.randn(n, generator=gen)
    gs = [(torch.randn(n, generator=gen) * mag).to(g_dtype) for _ in range(k)]
    if zero_state:
        acc, m, v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    else:
        acc = torch.randn(n, generator=gen) * mag
        m = torch.randn(n, generator=gen) * mag
        v = (0.5 + torch.rand(n, generator=gen)) * mag * mag
        acc[1::7] = 0
        m[2::7] = 0                                    # m = 0 alone, and m = v = 0 together (v = 0 under a
        m[5::11] = 0                                   # non-zero m is no state Adam reaches: the step would be
        v[5::11] = 0                                   # lr_t * m / eps)
    for i, g in enumerate(gs):
        g[(3 + i) % 5::5] = 0                          # another fifth of the elements in every gradient
    return dict(w=w, g=gs, acc=acc, m=m, v=v)


# ------------------------------------------------------------------------------------- sentinel-guarded buffers
PAD = 4                         # elements before and after: the smallest offset 16-byte accesses allow
_SENTINEL = {torch.float32: (torch.int32, -842150451), torch.bfloat16: (torch.int16, -12851)}      # 0xCDCD...


class Guarded(object):
    """``t`` as the slice [PAD : PAD + n] of a larger buffer pre-filled with a sentinel bit pattern."""

    def __init__(self, t, device, dtype=None, n=None):
        dtype = dtype or t.dtype
        n = t.numel() if n is None else n
        self.bits, pattern = _SENTINEL[dtype]
        self.buf = torch.empty(n + 2 * PAD, dtype=dtype, device=device)
        self.buf.view(self.bits).fill_(pattern)
        self.pattern = pattern
        self.t = self.buf[PAD:PAD + n]
        if t is not None:
            self.t.copy_(t)
        self.before = self.buf.clone()

    def guards_intact(self):
        b = self.buf.view(self.bits)
        return bool((b[:PAD] == self.pattern).all()) and bool((b[-PAD:] == self.pattern).all())

    def unchanged(self):
        return torch.equal(self.buf.view(self.bits), self.before.view(self.bits))


def bits_equal(a, b):
    bits = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits).cpu(),
                                                                     b.contiguous().view(bits).cpu())
