"""The fp64 oracle, the cases and the limits of ``tests/test_lstm.py``.  The oracle is TF's ``LSTMCell`` (gate order
i, j, f, o) as a loop over t written from the formulas, its gradients fp64 autograd of that loop; nothing here imports
``mdtf.ops``.

Errors are ``max |got - ref| / max |ref|`` per tensor.  ``cpu`` (fp32 end to end): ``gamma(I + H + 8)``.  ``cuda``
(bf16 rounding of xg, h_t, the stored gates and dG, compounding over t): no sharp bound is derived; the limits are
twice what the same expression shows in fp32 on the CPU with those rounding points, worst over the cases a-e, measured
against this oracle by

    python -m bench.lstm_tolerance

(never from the kernels).  Over that expression the kernels change the summation order and the exp / reciprocal
units, both far below one bf16 step.
"""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import gamma  # noqa: E402

NAMES = ("outputs", "h_T", "c_T", "dx", "dkernel", "dbias", "dh0", "dc0")
#            (T, B,   I,  H)
CASES = {"a": (1, 1,   8,  32), "b": (3, 5, 16, 32), "c": (2, 80, 24, 96), "d": (4, 17, 32, 160),
         "e": (2, 130, 64, 64), "h48": (2, 5, 16, 48)}
FORGET_BIAS = 1.0

# worst error of the bf16-rounded fp32 expression over the cases a-e (output of the command above)
MEASURED_BF16 = {"outputs": 3.58e-03, "h_T": 3.58e-03, "c_T": 1.53e-03, "dx": 6.03e-03, "dkernel": 3.63e-03,
                 "dbias": 3.26e-03, "dh0": 4.96e-03, "dc0": 4.58e-03}
LIMIT_BF16 = {k: 2.0 * v for k, v in MEASURED_BF16.items()}


def oracle(x, kernel, bias, h0, c0, dhs, dh_t, dc_t, lengths=None):
    """Every tensor of NAMES in fp64.  ``lengths``: at t >= lengths[b] row b emits zeros and keeps its state."""
    leaves = [t.double().requires_grad_(True) for t in (x, kernel, bias, h0, c0)]
    xd, kd, bd, h, c = leaves
    hid = kd.shape[1] // 4
    outs = []
    for t in range(xd.shape[0]):
        gi, gj, gf, go = (torch.cat([xd[t], h], 1) @ kd + bd).split(hid, 1)
        c_new = c * torch.sigmoid(gf + FORGET_BIAS) + torch.sigmoid(gi) * torch.tanh(gj)
        h_new = torch.tanh(c_new) * torch.sigmoid(go)
        live = torch.ones(h.shape[0], 1, dtype=torch.bool) if lengths is None else (torch.tensor(lengths) > t)[:, None]
        h, c = torch.where(live, h_new, h), torch.where(live, c_new, c)
        outs.append(torch.where(live, h_new, torch.zeros_like(h_new)))
    hs = torch.stack(outs, 0)
    loss = (hs * dhs.double()).sum() + (h * dh_t.double()).sum() + (c * dc_t.double()).sum()
    dx, dk, db, dh0, dc0 = torch.autograd.grad(loss, leaves)
    return dict(zip(NAMES, (hs.detach(), h.detach(), c.detach(), dx, dk, db, dh0, dc0)))


class Case(object):
    """Inputs (bf16-representable fp32) and the oracle of one shape, computed once and left unchanged."""

    def __init__(self, name, lengths=None):
        t, b, i, h = self.shape = CASES[name]
        seed = 1000 + 10 * sorted(CASES).index(name)
        self.x = NH.randn((t, b, i), seed)
        self.kernel = NH.randn((i + h, 4 * h), seed + 1, (i + h) ** -0.5)
        self.bias = NH.randn((4 * h,), seed + 2, 0.25)
        self.h0, self.c0 = NH.randn((b, h), seed + 3, 0.5), NH.randn((b, h), seed + 4, 0.5)
        self.dhs, self.dh_t, self.dc_t = NH.randn((t, b, h), seed + 5), NH.randn((b, h), seed + 6), NH.randn((b, h), seed + 7)
        self.lengths = lengths
        self.ref = oracle(self.x, self.kernel, self.bias, self.h0, self.c0, self.dhs, self.dh_t, self.dc_t, lengths)


@functools.lru_cache(maxsize=None)
def case(name, lengths=None):
    return Case(name, lengths)


def errors(got, ref):
    """``max |got - ref| / max |ref|`` of every tensor in ``got``."""
    out = {}
    for k, g in got.items():
        g = g.detach().cpu().double()
        assert g.shape == ref[k].shape and bool(torch.isfinite(g).all()), k
        out[k] = float((g - ref[k]).abs().max() / ref[k].abs().max())
    return out


def check(what, got, c, bf16, slot0=None):
    """``got`` (a dict over NAMES) against the oracle of ``c``; ``slot0``: what the kernel's slot held before."""
    ref = dict(c.ref)
    if slot0 is not None:
        got = dict(got, dkernel=got["dkernel"].detach().cpu().double() - slot0.double())
    t, b, i, h = c.shape
    for k, e in errors(got, ref).items():
        limit = LIMIT_BF16[k] if bf16 else gamma(i + h + 8)
        print("LSTM_ERR %-28s %-8s %.3e (limit %.3e)" % (what, k, e, limit))
        assert e <= limit, "%s %s: error %.3e of max |ref| above %.3e" % (what, k, e, limit)
