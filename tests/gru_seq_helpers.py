"""The cases, references and limits of ``tests/test_gru_lengths.py``: per-row lengths, the reverse direction and a
forward plus a reverse GRU.  The oracle is ``gru_helpers.oracle`` (fp64); a reverse direction is TF's definition
``reverse_sequence -> GRU -> reverse_sequence``: ``x`` and ``dhs`` gathered with each row's first ``len`` steps
reversed, the oracle run with the lengths, ``outputs`` and ``dx`` gathered back.  Nothing here imports ``mdtf.ops``.

Limits.  ``cpu``: ``gru_helpers.cpu_limit``.  ``cuda``: as ``gru_helpers``, twice the error of the fp32 expression
with the kernels' bf16 rounding points against the oracle, measured on the CPU (never from the kernels) by
``python -m bench.gru_tolerance --lengths``, worst over the modes ``fw``, ``bw`` and ``both`` (the parameters of
``other`` in the second direction, the pair's summed dx).  Where a figure does not exceed ``gru_helpers.MEASURED_BF16``
/ ``MEASURED_CARRY`` the limit is that file's ``LIMIT_BF16`` / ``LIMIT_CARRY`` entry, else twice the figure here.
"""
import functools
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_helpers as GH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

MODES = ("fw", "bw", "both")
# name: ((T, B, I, H), lengths).  mix: lengths 0, 1 and T in a partial tile.  tile: a whole dead tile between live ones,
# a ragged last tile, U = 16.  u32: blocks that own 32 units.  carry: gru_helpers' U_SHIFT; row 1 freezes at step 20.
CASES = {"mix": ((5, 5, 16, 32), (5, 0, 3, 1, 4)),
         "tile": ((4, 35, 32, 160), tuple((3 * b) % 5 for b in range(16)) + (0,) * 16 + (4, 1, 3)),
         "u32": ((3, 256, 32, 512), tuple(b % 4 for b in range(256))),
         "carry": ((48, 3, 8, 32), (48, 20, 1))}

# output of the command above: worst over the short cases and modes / at the carry case
MEASURED_SEQ = {"outputs": 3.38e-03, "h_T": 2.31e-03, "dx": 5.45e-03, "dgates_kernel": 4.33e-03, "dgates_bias": 3.73e-03,
                "dcand_kernel": 3.45e-03, "dcand_bias": 2.53e-03, "dh0": 5.28e-03}
MEASURED_SEQ_CARRY = {"outputs": 3.27e-03, "h_T": 3.87e-03, "dx": 1.70e-02, "dgates_kernel": 1.59e-02,
                      "dgates_bias": 1.21e-02, "dcand_kernel": 1.81e-02, "dcand_bias": 5.77e-03, "dh0": 6.86e-03}
# doubled where above gru_helpers' figure -- short: outputs 6.76e-03, dx 1.09e-02, dgates_bias 7.46e-03, dcand_kernel
# 6.90e-03, dh0 1.06e-02; carry: outputs 6.54e-03, h_T 7.74e-03, dx 3.40e-02, dgates_kernel 3.18e-02, dgates_bias
# 2.42e-02, dcand_bias 1.15e-02, dh0 1.37e-02 -- and gru_helpers' limit for the rest
LIMIT_SEQ = {k: GH.LIMIT_BF16[k] if v <= GH.MEASURED_BF16[k] else 2.0 * v for k, v in MEASURED_SEQ.items()}
LIMIT_SEQ_CARRY = {k: GH.LIMIT_CARRY[k] if v <= GH.MEASURED_CARRY[k] else 2.0 * v
                   for k, v in MEASURED_SEQ_CARRY.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    (t, b, i, h), lengths = CASES[name]
    s = 3000 + 10 * sorted(CASES).index(name)
    gb = NH.randn((2 * h,), s + 3, 0.25)
    gb[h:] += GH.U_SHIFT.get(name, 0.0)
    return types.SimpleNamespace(
        name=name, shape=(t, b, i, h), lengths=lengths, x=NH.randn((t, b, i), s),
        gk=NH.randn((i + h, 2 * h), s + 1, (i + h) ** -0.5), ck=NH.randn((i + h, h), s + 2, (i + h) ** -0.5),
        gb=NH.bf16_exact(gb), cb=NH.randn((h,), s + 4, 0.25), h0=NH.randn((b, h), s + 5, 0.5),
        dhs=NH.randn((t, b, h), s + 6), dh_t=NH.randn((b, h), s + 7))


@functools.lru_cache(maxsize=None)
def other(name):
    """Different parameters, state and gradients of the same shapes (the second direction of a pair)."""
    c = case(name)
    return types.SimpleNamespace(name=name, shape=c.shape, lengths=c.lengths, x=c.x, gk=-c.gk, ck=c.ck.flip(1),
                                 gb=c.gb, cb=-c.cb, h0=-c.h0, dhs=-c.dhs.flip(2), dh_t=c.dh_t.flip(1))


def reverse_sequence(x, lengths):
    t = torch.arange(x.shape[0])[:, None]
    n = torch.tensor(lengths)[None]
    return x[torch.where(t < n, n - 1 - t, t), torch.arange(x.shape[1])[None]]


@functools.lru_cache(maxsize=None)
def reference(name, direction, alt=False):
    """The oracle of one direction (``alt``: with the parameters of ``other``), computed once and left unchanged."""
    c = other(name) if alt else case(name)
    rev = functools.partial(reverse_sequence, lengths=c.lengths) if direction == "bw" else (lambda z: z)
    ref = GH.oracle(rev(c.x), c.gk, c.gb, c.ck, c.cb, c.h0, rev(c.dhs), c.dh_t, c.lengths)
    return dict(ref, outputs=rev(ref["outputs"]), dx=rev(ref["dx"]))


def plan(name, mode):
    """``[(inputs, direction, reference)]`` of a mode; the two directions of ``both`` share x, so their dx is the sum."""
    if mode != "both":
        return [(case(name), mode, reference(name, mode))]
    refs = [reference(name, "fw"), reference(name, "bw", True)]
    dx = refs[0]["dx"] + refs[1]["dx"]
    return [(case(name), "fw", dict(refs[0], dx=dx)), (other(name), "bw", dict(refs[1], dx=dx))]


def check(what, got, ref, c, direction, bf16):
    """``got`` (a dict over ``GH.NAMES``) against ``ref``; then: dead outputs are exactly zero and ``h_T`` has the bits
    of the output at the row's last visited live step (``h0`` for length 0)."""
    limits = (LIMIT_SEQ_CARRY if c.name == "carry" else LIMIT_SEQ) if bf16 else dict.fromkeys(GH.NAMES,
                                                                                            GH.cpu_limit(c.shape))
    for k, e in GH.errors(got, ref).items():
        print("GRU_LEN_ERR %-24s %-14s %.3e (limit %.3e)" % (what, k, e, limits[k]))
        assert e <= limits[k], "%s %s: error %.3e of max |ref| above %.3e" % (what, k, e, limits[k])
    out, h_t = got["outputs"].detach(), got["h_T"].detach()
    for b, n in enumerate(c.lengths):
        assert n == c.shape[0] or float(out[n:, b].abs().max()) == 0.0, (what, b)
        last = out[n - 1 if direction == "fw" else 0, b] if n else NH.put(c.h0, str(out.device.type))[b].to(out.dtype)
        assert NH.bits_equal(h_t[b], last), (what, b)
