"""Measure the bf16 limits of ``tests/lstm_helpers.py`` and ``tests/test_lstm_lengths.py`` on the CPU (no GPU, no
kernel involved).

The LSTM of ``mdtf/ops/rnn.py`` as an fp32 PyTorch expression, forward and backward, rounded to bf16 at exactly the
points where the HIP path rounds: xg (the input half with its bias), h_t, the stored post-activation gates, dG, and the
bf16 results dx and dh0.  The cell state, the carried cell gradient and the kernel / bias gradients stay fp32.  Its
error against the fp64 oracle, ``max |got - ref| / max |ref|`` per tensor, worst over the cases a-e, is
``MEASURED_BF16``; the tests allow the kernels twice that.

    python -m bench.lstm_tolerance

``--lengths``: the same expression with per-row lengths, in both directions and for the two directions at once (whose
dx is one bf16 tensor the second direction adds into), over the cases of ``tests/test_lstm_lengths.py`` against its
oracles: ``MEASURED_LENGTHS``.

    python -m bench.lstm_tolerance --lengths
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import lstm_helpers as LH  # noqa: E402


def _r(t):
    return t.bfloat16().float()


def emulate(c, reverse=False, dx_base=None):
    """``c.lengths`` (None: full length): a dead row keeps its state and emits zeros; ``reverse``: t runs from T - 1
    down.  ``dx_base``: the bf16 dx of another direction that this one's product adds into."""
    t_n, b_n, i_n, h_n = c.shape
    wx, wh = c.kernel[:i_n], c.kernel[i_n:]
    x2 = c.x.reshape(t_n * b_n, i_n)
    xg = _r(x2 @ wx + c.bias).reshape(t_n, b_n, 4 * h_n)
    lens = torch.tensor(c.lengths if c.lengths is not None else [t_n] * b_n)[:, None]
    order = list(range(t_n - 1, -1, -1) if reverse else range(t_n))
    h, cell = c.h0, c.c0
    hs, cs, gates, h_prev, c_prev = ([None] * t_n for _ in range(5))
    for t in order:
        live = lens > t
        gi, gj, gf, go = (xg[t] + h @ wh).split(h_n, 1)
        gi, gj, gf, go = torch.sigmoid(gi), torch.tanh(gj), torch.sigmoid(gf + LH.FORGET_BIAS), torch.sigmoid(go)
        h_prev[t], c_prev[t] = h, cell
        cs[t] = cell * gf + gi * gj
        h_new = _r(torch.tanh(cs[t]) * go)
        hs[t] = torch.where(live, h_new, torch.zeros_like(h_new))
        h, cell = torch.where(live, h_new, h), torch.where(live, cs[t], cell)
        gates[t] = [_r(g) for g in (gi, gj, gf, go)]
    h_fin, c_fin = h, cell
    carry, dh_next, dg = c.dc_t.clone(), c.dh_t, [None] * t_n      # dh_next: dL/dh of the state a row holds, in fp32
    for t in reversed(order):
        live = lens > t
        gi, gj, gf, go = gates[t]
        dh = c.dhs[t] + dh_next
        tc = torch.tanh(cs[t])
        dc = carry + dh * go * (1 - tc * tc)
        dg[t] = _r(torch.cat([dc * gj * gi * (1 - gi), dc * gi * (1 - gj * gj), dc * c_prev[t] * gf * (1 - gf),
                              dh * tc * go * (1 - go)], 1))
        dg[t] = torch.where(live, dg[t], torch.zeros_like(dg[t]))
        carry, dh_next = torch.where(live, dc * gf, carry), torch.where(live, dg[t] @ wh.t(), dh_next)
    dg2 = torch.stack(dg, 0).reshape(t_n * b_n, 4 * h_n)
    hp = torch.stack(h_prev, 0).reshape(t_n * b_n, h_n)
    dx = dg2 @ wx.t() if dx_base is None else dx_base.reshape(t_n * b_n, i_n) + dg2 @ wx.t()
    return dict(zip(LH.NAMES, (torch.stack(hs, 0), h_fin, c_fin, _r(dx).reshape(c.x.shape),
                               torch.cat([x2.t() @ dg2, hp.t() @ dg2], 0), dg2.sum(0), _r(dh_next), carry)))


def _show(what, worst, err):
    print("%s %s" % (what, " ".join("%s=%.3e" % kv for kv in err.items())))
    return {k: max(worst[k], err[k]) for k in worst}


def lengths_table():
    import test_lstm_lengths as TL
    worst = dict.fromkeys(LH.NAMES, 0.0)
    for name in TL.LENGTHS:
        c = TL.case(name)
        for direction in ("fw", "bw"):
            got = emulate(c, direction == "bw")
            worst = _show("case %s %s" % (name, direction), worst, LH.errors(got, TL.reference(name, direction)))
        if name not in TL.PAIRS:
            continue
        alt, ref_fw, ref_bw = TL.other(c), TL.reference(name, "fw"), TL.reference(name, "bw", True)
        fw = emulate(c)
        bw = emulate(alt, True, dx_base=fw["dx"])
        worst = _show("case %s bidirectional bw" % name, worst, LH.errors(bw, dict(ref_bw, dx=ref_fw["dx"] + ref_bw["dx"])))
    print("MEASURED_LENGTHS = {%s}" % ", ".join('"%s": %.2e' % kv for kv in worst.items()))


def main():
    if "--lengths" in sys.argv[1:]:
        return lengths_table()
    worst = dict.fromkeys(LH.NAMES, 0.0)
    for name in "abcde":
        c = LH.case(name)
        worst = _show("case %s" % name, worst, LH.errors(emulate(c), c.ref))
    print("MEASURED_BF16 = {%s}" % ", ".join('"%s": %.2e' % kv for kv in worst.items()))


if __name__ == "__main__":
    main()
