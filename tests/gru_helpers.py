"""The fp64 oracle, the cases and the limits of ``tests/test_gru.py``.  The oracle is TF's ``GRUCell`` (the reset gate
applied before the candidate product) as a loop over t written from the formulas, its gradients fp64 autograd of that
loop; nothing here imports ``mdtf.ops``.

Errors are ``max |got - ref| / max |ref|`` per tensor.

``cpu`` (the fp32 loop on bf16-representable values): ``gamma(k)`` with ``k = T * (2 (I + H) + 3 H + 32)``.  A step
chains two products: the gate pre-activations are sums of ``I + H`` terms and a bias, their sigmoid (slope <= 1/4)
scales ``h`` into the candidate product, again ``I + H`` terms and a bias, whose tanh (slope <= 1) enters the update;
that is ``2 (I + H + 1)`` roundings on the longest path of a forward step.  The backward step chains the two
transposed products, ``H`` terms (candidate) then ``2 H`` terms (gates).  The elementwise arithmetic of a step adds
fewer than 30 more in both directions together.  The state passes from step to step with a factor of order one
(``u`` plus the gate terms), so the path of the last step's result runs through all ``T`` steps.

``cuda`` (bf16 rounding of xg, rh, h_t as operand and output, the stored gates, dG and dx; the carried state, the
carried gradient and the weight gradients in fp32): no sharp bound is derived; the limits are twice what the same
expression shows in fp32 on the CPU with those rounding points, measured against this oracle by

    python -m bench.gru_tolerance

(never from the kernels): ``MEASURED_BF16`` is the worst over the short cases a-f, ``MEASURED_CARRY`` belongs to the
carry case, whose 48 steps compound differently.  Over that expression the kernels change the summation order and the
exp / reciprocal units, both far below one bf16 step.
"""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import gamma  # noqa: E402

NAMES = ("outputs", "h_T", "dx", "dgates_kernel", "dgates_bias", "dcand_kernel", "dcand_bias", "dh0")
#            (T, B,   I,  H)
CASES = {"a": (1, 1,   8,  32), "b": (3, 5, 16, 32), "c": (2, 80, 24, 96), "d": (4, 17, 32, 160),
         "e": (2, 130, 64, 64), "f": (2, 256, 32, 512),      # f: the smallest shape whose blocks own 32 units
         "carry": (48, 3, 8, 32), "h48": (2, 5, 16, 48)}
SHORT = "abcdef"
U_SHIFT = {"carry": 3.0}       # added to the u half of gates/bias: u sits near 1 and a step adds little to h

# worst error of the bf16-rounded fp32 expression over the cases a-f / at the carry case (output of the command above)
MEASURED_BF16 = {"outputs": 3.08e-03, "h_T": 3.49e-03, "dx": 4.85e-03, "dgates_kernel": 5.00e-03, "dgates_bias": 3.10e-03,
                 "dcand_kernel": 3.32e-03, "dcand_bias": 3.77e-03, "dh0": 5.22e-03}
MEASURED_CARRY = {"outputs": 2.32e-03, "h_T": 3.07e-03, "dx": 1.62e-02, "dgates_kernel": 1.24e-02, "dgates_bias": 5.09e-03,
                  "dcand_kernel": 1.90e-02, "dcand_bias": 2.61e-03, "dh0": 3.98e-03}
# (the same run with the carried state rounded to bf16 every step: outputs 6.86e-03, h_T 7.66e-03 -- above twice the
# carry case's figures, so that case tells an fp32 carry from a bf16 one)
LIMIT_BF16 = {k: 2.0 * v for k, v in MEASURED_BF16.items()}
LIMIT_CARRY = {k: 2.0 * v for k, v in MEASURED_CARRY.items()}


def oracle(x, gk, gb, ck, cb, h0, dhs, dh_t, lengths=None):
    """Every tensor of NAMES in fp64.  ``lengths``: at t >= lengths[b] row b emits zeros and keeps its state."""
    leaves = [t.double().requires_grad_(True) for t in (x, gk, gb, ck, cb, h0)]
    xd, gkd, gbd, ckd, cbd, h = leaves
    hid = ckd.shape[1]
    outs = []
    for t in range(xd.shape[0]):
        r, u = torch.sigmoid(torch.cat([xd[t], h], 1) @ gkd + gbd).split(hid, 1)
        c = torch.tanh(torch.cat([xd[t], r * h], 1) @ ckd + cbd)
        h_new = u * h + (1 - u) * c
        live = torch.ones(h.shape[0], 1, dtype=torch.bool) if lengths is None else (torch.tensor(lengths) > t)[:, None]
        h = torch.where(live, h_new, h)
        outs.append(torch.where(live, h_new, torch.zeros_like(h_new)))
    hs = torch.stack(outs, 0)
    loss = (hs * dhs.double()).sum() + (h * dh_t.double()).sum()
    grads = torch.autograd.grad(loss, leaves)
    return dict(zip(NAMES, (hs.detach(), h.detach()) + tuple(grads)))


class Case(object):
    """Inputs (bf16-representable fp32) and the oracle of one shape, computed once and left unchanged."""

    def __init__(self, name, lengths=None):
        t, b, i, h = self.shape = CASES[name]
        seed = 2000 + 10 * sorted(CASES).index(name)
        self.name, self.lengths = name, lengths
        self.x = NH.randn((t, b, i), seed)
        self.gk = NH.randn((i + h, 2 * h), seed + 1, (i + h) ** -0.5)
        self.ck = NH.randn((i + h, h), seed + 2, (i + h) ** -0.5)
        gb = NH.randn((2 * h,), seed + 3, 0.25)
        gb[h:] += U_SHIFT.get(name, 0.0)
        self.gb = NH.bf16_exact(gb)
        self.cb = NH.randn((h,), seed + 4, 0.25)
        self.h0 = NH.randn((b, h), seed + 5, 0.5)
        self.dhs, self.dh_t = NH.randn((t, b, h), seed + 6), NH.randn((b, h), seed + 7)
        self.ref = oracle(self.x, self.gk, self.gb, self.ck, self.cb, self.h0, self.dhs, self.dh_t, lengths)


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


def cpu_limit(shape):
    t, b, i, h = shape
    return gamma(t * (2 * (i + h) + 3 * h + 32))


def check(what, got, c, bf16, slots0=None):
    """``got`` (a dict over NAMES) against the oracle of ``c``; ``slots0``: what the kernels' slots held before."""
    got = dict(got)
    for k, s0 in (slots0 or {}).items():
        got[k] = got[k].detach().cpu().double() - s0.double()
    limits = (LIMIT_CARRY if c.name == "carry" else LIMIT_BF16) if bf16 else dict.fromkeys(NAMES, cpu_limit(c.shape))
    for k, e in errors(got, c.ref).items():
        print("GRU_ERR %-28s %-14s %.3e (limit %.3e)" % (what, k, e, limits[k]))
        assert e <= limits[k], "%s %s: error %.3e of max |ref| above %.3e" % (what, k, e, limits[k])
