"""Measure the bf16 limits of ``tests/gru_helpers.py`` on the CPU (no GPU, no kernel involved).

The GRU of ``mdtf/ops/gru.py`` as an fp32 PyTorch expression, forward and backward, rounded to bf16 at exactly the
points where the HIP path rounds: xg (the input half with its biases), rh = r * h_prev, h_t as GEMM operand and as
output, the stored post-activation gates (which the backward reads; the forward's update takes u in fp32), dG, and
the bf16 results dx and dh0.  The carried state, the carried gradient and the kernel / bias gradients stay fp32.  Its
error against the fp64 oracle, ``max |got - ref| / max |ref|`` per tensor, is ``MEASURED_BF16`` (worst over the cases
a-f) and ``MEASURED_CARRY`` (the carry case); the tests allow the kernels twice that.

    python -m bench.gru_tolerance

The last line repeats the carry case with the carried state rounded to bf16 every step, the design the kernels avoid:
its ``h_T`` error has to exceed the carry case's limit, or that case distinguishes nothing.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gru_helpers as GH  # noqa: E402


def _r(t):
    return t.bfloat16().float()


def emulate(c, bf16_carry=False):
    t_n, b_n, i_n, h_n = c.shape
    wgx, wgh, wcx, wch = c.gk[:i_n], c.gk[i_n:], c.ck[:i_n], c.ck[i_n:]
    wx = torch.cat([wgx, wcx], 1)
    x2 = c.x.reshape(t_n * b_n, i_n)
    xg = _r(x2 @ wx + torch.cat([c.gb, c.cb])).reshape(t_n, b_n, 3 * h_n)
    hf, hb = c.h0, _r(c.h0)
    hs, rh, gates, hp_f, hp_b = ([None] * t_n for _ in range(5))
    for t in range(t_n):
        r, u = torch.sigmoid(xg[t][:, :2 * h_n] + hb @ wgh).split(h_n, 1)
        rh[t] = _r(r * hf)
        cand = torch.tanh(xg[t][:, 2 * h_n:] + rh[t] @ wch)
        hp_f[t], hp_b[t] = hf, hb
        hf = u * hf + (1 - u) * cand                   # u in fp32 here; the backward reads the stored one
        u = _r(u)
        if bf16_carry:
            hf = _r(hf)
        hs[t] = hb = _r(hf)
        gates[t] = (_r(r), u, _r(cand))
    carry, dg = c.dh_t.clone(), [None] * t_n
    for t in range(t_n - 1, -1, -1):
        r, u, cand = gates[t]
        dh = carry + c.dhs[t]
        if t < t_n - 1:
            dh = dh + dg[t + 1][:, :2 * h_n] @ wgh.t()
        dpc = _r(dh * (1 - u) * (1 - cand * cand))
        dpu = _r(dh * (hp_f[t] - cand) * u * (1 - u))
        d_rh = dpc @ wch.t()
        dpr = _r(d_rh * hp_f[t] * r * (1 - r))
        carry = dh * u + d_rh * r
        dg[t] = torch.cat([dpr, dpu, dpc], 1)
    carry = carry + dg[0][:, :2 * h_n] @ wgh.t()
    dg2 = torch.stack(dg, 0).reshape(t_n * b_n, 3 * h_n)
    dgate, dpc = dg2[:, :2 * h_n], dg2[:, 2 * h_n:]
    hp2, rh2 = torch.stack(hp_b, 0).reshape(t_n * b_n, h_n), torch.stack(rh, 0).reshape(t_n * b_n, h_n)
    return dict(zip(GH.NAMES, (torch.stack(hs, 0), hs[-1], _r(dg2 @ wx.t()).reshape(c.x.shape),
                               torch.cat([x2.t() @ dgate, hp2.t() @ dgate], 0), dgate.sum(0),
                               torch.cat([x2.t() @ dpc, rh2.t() @ dpc], 0), dpc.sum(0), _r(carry))))


def _show(what, err):
    print("%s %s" % (what, " ".join("%s=%.3e" % kv for kv in err.items())))
    return err


def main():
    worst = dict.fromkeys(GH.NAMES, 0.0)
    for name in GH.SHORT:
        c = GH.case(name)
        err = _show("case %s" % name, GH.errors(emulate(c), c.ref))
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("MEASURED_BF16 = {%s}" % ", ".join('"%s": %.2e' % kv for kv in worst.items()))
    c = GH.case("carry")
    err = _show("case carry", GH.errors(emulate(c), c.ref))
    print("MEASURED_CARRY = {%s}" % ", ".join('"%s": %.2e' % kv for kv in err.items()))
    _show("case carry, state rounded to bf16 every step", GH.errors(emulate(c, bf16_carry=True), c.ref))


if __name__ == "__main__":
    main()
