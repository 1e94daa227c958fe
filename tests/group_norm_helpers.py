"""Shared pieces of ``tests/test_group_norm.py``: the fp64 oracle of group normalization (+ ReLU) and its backward,
written from the definition, and the elementwise bounds of an fp32 evaluation, derived as ``bn_helpers`` derives
BatchNorm's (``U``, ``gamma(k)``, ``RSQRT_REL``, ``CAP`` and the bf16 output rounding are that module's).

Statistics of a group of m bf16 values (exact in fp32).  A mean summed in any order: ``em = (gamma(m) + 2 U) max|x|``
(also any chunk's mean).  The variance is a sum of squares about the computed mean mu' = mean + d,
``sum (x - mu')^2 = m var + m d^2`` exactly, three roundings per term and at most m in the sum:
``ev = gamma(m + 3) (var + em^2) + em^2 + 2 U var``.  With K > 1 streaming chunks the M2 are about chunk means (another
``em^2``) and Chan's merge adds ``delta^2 w`` with each delta within 2 em: by Cauchy-Schwarz with
``sum delta^2 w <= m var`` and ``sum w <= m`` that is ``4 em sqrt(var) + 4 em^2`` more.  Nothing here allows the
``U m (var + mean^2)`` of ``E[x^2] - mean^2``.  ``rstd``, ``pre`` (8 roundings) and the backward (12) follow
``bn_helpers.stats_ref`` / ``fwd_ref`` / ``bwd_ref`` with, per image and group, ``A = sum dz gamma`` and
``Q = sum dz gamma xhat`` over ``H W + Cg`` terms for BN's ``dbeta`` / ``dgamma``; the parameter gradients sum
``N H W`` terms per channel.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_helpers as BH  # noqa: E402
from nhwc_helpers import TINY, U, gamma, out_bound  # noqa: E402


class Ref(object):
    """The oracle of one case: x, dy [N, H, W, C] and gamma, beta [C] (bf16-representable fp32), K streaming chunks."""

    def __init__(self, x, g, b, dy, G, eps, K=1):
        N, H, W, C = x.shape
        self.shape, self.G, self.Cg, self.HW = x.shape, G, C // G, H * W
        self.m = m = self.HW * self.Cg
        self.x, self.dy = x.double().reshape(N, self.HW, G, self.Cg), dy.double().reshape(N, self.HW, G, self.Cg)
        self.g, self.b = g.double().reshape(G, self.Cg), b.double().reshape(G, self.Cg)
        x = self.x
        self.mean = x.mean((1, 3), keepdim=True)
        self.var = ((x - self.mean) ** 2).mean((1, 3), keepdim=True)
        em = (gamma(m) + 2 * U) * x.abs().amax((1, 3), keepdim=True)
        ev = gamma(m + 3) * (self.var + em ** 2) + em ** 2 + 2 * U * self.var
        if K > 1:
            ev = ev + 4 * em * self.var.sqrt() + 5 * em ** 2
        self.emf = em + U * (self.mean.abs() + em)                    # the saved fp32 mean
        v = self.var + eps
        e_v = ev + 2 * U * (v + ev)
        assert bool((e_v < 0.5 * v).all())
        rel = 0.5 * e_v / (v - e_v)
        self.inv = v ** -0.5
        self.einv = self.inv * (rel + BH.RSQRT_REL * (1 + rel)) + U * self.inv
        self.inv_hi, self.mu_hi = self.inv + self.einv, self.mean.abs() + self.emf
        self.d = x - self.mean
        self.xhat = self.d * self.inv
        self.e_xhat = self.d.abs() * self.einv + self.inv_hi * self.emf
        self.pre = self.xhat * self.g + self.b
        B = self.g.abs() * self.inv_hi * (x.abs() + self.mu_hi) + self.b.abs()
        self.pre_acc = self.g.abs() * self.e_xhat + gamma(8) * B

    def outputs(self, relu, got_pos, bf, what, dg0=None, db0=None):
        """Every output and its bound.  ``got_pos`` [N, H, W, C]: the signs the code under test took, used only for
        the elements whose pre-activation is within its bound of zero (at most ``bn_helpers.CAP`` of them)."""
        pre, g, m = self.pre, self.g, self.m
        self.nhwc = lambda t: t.reshape(self.shape)
        pos = torch.ones_like(pre, dtype=torch.bool)
        if relu:
            pos, _ = BH.relu_sign(pre, self.pre_acc, got_pos.reshape(pre.shape), what)
        y = torch.where(pos, pre, torch.zeros_like(pre))
        out = dict(y=self.nhwc(y), y_bound=self.nhwc(out_bound(y, self.pre_acc.expand_as(y), bf)))
        dz = self.dy * pos
        dzg = dz * g
        k = self.HW + self.Cg + 4
        A, Q = dzg.sum((1, 3), keepdim=True), (dzg * self.xhat).sum((1, 3), keepdim=True)
        eA = gamma(k) * dzg.abs().sum((1, 3), keepdim=True)
        eQ = (dzg.abs() * self.e_xhat).sum((1, 3), keepdim=True) + gamma(k) * (dzg * self.xhat).abs().sum(
            (1, 3), keepdim=True)
        if not bf:      # the PyTorch branch forms Q as rstd (sum dz gamma x - mean sum dz gamma), which cancels
            eQ = eQ + self.inv_hi * gamma(k) * ((dzg * self.x).abs().sum((1, 3), keepdim=True)
                                                + self.mu_hi * dzg.abs().sum((1, 3), keepdim=True))
        t = dzg - A / m - self.xhat * Q / m
        dx = self.inv * t
        B = self.inv_hi * (dzg.abs() + (A.abs() + eA) / m + self.inv_hi * (Q.abs() + eQ) / m * (
            self.x.abs() + self.mu_hi))
        acc = self.einv * t.abs() + self.inv_hi * (eA / m + (self.xhat.abs() + self.e_xhat) * eQ / m
                                                   + Q.abs() / m * self.e_xhat) + gamma(12) * B
        out["dx"], out["dx_bound"] = self.nhwc(dx), self.nhwc(out_bound(dx, acc, bf))
        R = self.shape[0] * self.HW
        db, dg = dz.sum((0, 1)).reshape(-1), (dz * self.xhat).sum((0, 1)).reshape(-1)
        edb = gamma(R) * dz.abs().sum((0, 1)).reshape(-1)
        edg = ((dz.abs() * self.e_xhat).sum((0, 1)) + gamma(R + 2) * (dz * self.xhat).abs().sum((0, 1))).reshape(-1)
        dg0 = torch.zeros_like(dg) if dg0 is None else dg0.double()
        db0 = torch.zeros_like(db) if db0 is None else db0.double()
        out["dgamma"], out["dbeta"] = dg0 + dg, db0 + db
        out["dgamma_bound"] = edg + 2 * U * (dg0.abs() + dg.abs() + edg) + TINY     # the cast, the add onto the slot
        out["dbeta_bound"] = edb + 2 * U * (db0.abs() + db.abs() + edb) + TINY
        return out

    def stats(self):
        f = lambda t: t.reshape(self.shape[0], self.G)                # noqa: E731
        return f(self.mean), f(self.emf) + TINY, f(self.inv), f(self.einv) + TINY
