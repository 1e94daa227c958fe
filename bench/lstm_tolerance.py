"""Measure the bf16 limits of ``tests/lstm_helpers.py`` on the CPU (no GPU, no kernel involved).

The LSTM of ``mdtf/ops/rnn.py`` as an fp32 PyTorch expression, forward and backward, rounded to bf16 at exactly the
points where the HIP path rounds: xg (the input half with its bias), h_t, the stored post-activation gates, dG, and the
bf16 results dx and dh0.  The cell state, the carried cell gradient and the kernel / bias gradients stay fp32.  Its
error against the fp64 oracle, ``max |got - ref| / max |ref|`` per tensor, worst over the cases a-e, is
``MEASURED_BF16``; the tests allow the kernels twice that.

    python -m bench.lstm_tolerance
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import lstm_helpers as LH  # noqa: E402


def _r(t):
    return t.bfloat16().float()


def emulate(c):
    t_n, b_n, i_n, h_n = c.shape
    wx, wh = c.kernel[:i_n], c.kernel[i_n:]
    x2 = c.x.reshape(t_n * b_n, i_n)
    xg = _r(x2 @ wx + c.bias).reshape(t_n, b_n, 4 * h_n)
    h, cell = c.h0, c.c0
    hs, cs, gates = [], [], []
    for t in range(t_n):
        gi, gj, gf, go = (xg[t] + h @ wh).split(h_n, 1)
        gi, gj, gf, go = torch.sigmoid(gi), torch.tanh(gj), torch.sigmoid(gf + LH.FORGET_BIAS), torch.sigmoid(go)
        cell = cell * gf + gi * gj
        h = _r(torch.tanh(cell) * go)
        hs.append(h)
        cs.append(cell)
        gates.append([_r(g) for g in (gi, gj, gf, go)])
    carry, dg = c.dc_t.clone(), [None] * t_n
    for t in range(t_n - 1, -1, -1):
        gi, gj, gf, go = gates[t]
        dh = c.dhs[t] + (c.dh_t if t == t_n - 1 else dg[t + 1] @ wh.t())
        tc = torch.tanh(cs[t])
        dc = carry + dh * go * (1 - tc * tc)
        c_prev = cs[t - 1] if t else c.c0
        dg[t] = _r(torch.cat([dc * gj * gi * (1 - gi), dc * gi * (1 - gj * gj), dc * c_prev * gf * (1 - gf),
                              dh * tc * go * (1 - go)], 1))
        carry = dc * gf
    dg2 = torch.stack(dg, 0).reshape(t_n * b_n, 4 * h_n)
    h_prev = torch.stack([c.h0] + hs[:-1], 0).reshape(t_n * b_n, h_n)
    return dict(zip(LH.NAMES, (torch.stack(hs, 0), hs[-1], cs[-1], _r(dg2 @ wx.t()).reshape(c.x.shape),
                               torch.cat([x2.t() @ dg2, h_prev.t() @ dg2], 0), dg2.sum(0), _r(dg[0] @ wh.t()),
                               carry)))


def main():
    worst = dict.fromkeys(LH.NAMES, 0.0)
    for name in "abcde":
        c = LH.case(name)
        err = LH.errors(emulate(c), c.ref)
        print("case %s %s" % (name, " ".join("%s=%.3e" % kv for kv in err.items())))
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("MEASURED_BF16 = {%s}" % ", ".join('"%s": %.2e' % kv for kv in worst.items()))


if __name__ == "__main__":
    main()
