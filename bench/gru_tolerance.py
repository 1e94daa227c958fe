"""Measure the bf16 limits of ``tests/gru_helpers.py`` on the CPU (no GPU, no kernel involved).

The GRU of ``mdtf/ops/gru.py`` as an fp32 PyTorch expression, forward and backward, rounded to bf16 at exactly the
points where the HIP path rounds: xg (the input half with its biases), rh = r * h_prev, h_t as GEMM operand and as
output, the stored post-activation gates (which the backward reads; the forward's update takes u in fp32), dG, and
the bf16 results dx and dh0.  The carried state, the carried gradient and the kernel / bias gradients stay fp32.  Its
error against the fp64 oracle, ``max |got - ref| / max |ref|`` per tensor, is ``MEASURED_BF16`` (worst over the cases
a-f) and ``MEASURED_CARRY`` (the carry case); the tests allow the kernels twice that.

    python -m bench.gru_tolerance
    python -m bench.gru_tolerance --lengths

``--lengths`` does the same for ``tests/gru_seq_helpers.py``: its cases with per-row lengths, forward, reverse and as a
forward / reverse pair whose dx sums (``MEASURED_SEQ``, ``MEASURED_SEQ_CARRY``).  A dead row keeps its state and
carried gradient and has zeros in every saved buffer and in dG, as the kernels leave them.

The last line of the first form repeats the carry case with the carried state rounded to bf16 every step, the design the kernels avoid:
its ``h_T`` error has to exceed the carry case's limit, or that case distinguishes nothing.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gru_helpers as GH  # noqa: E402


def _r(t):
    return t.bfloat16().float()


def emulate(c, bf16_carry=False, reverse=False, dx0=None):
    """One direction; ``c.lengths`` (where the case has any) freezes rows as the kernels do.  ``dx0``: the bf16 dx of
    a first direction, which this one's product adds into before the rounding."""
    t_n, b_n, i_n, h_n = c.shape
    wgx, wgh, wcx, wch = c.gk[:i_n], c.gk[i_n:], c.ck[:i_n], c.ck[i_n:]
    wx = torch.cat([wgx, wcx], 1)
    x2 = c.x.reshape(t_n * b_n, i_n)
    xg = _r(x2 @ wx + torch.cat([c.gb, c.cb])).reshape(t_n, b_n, 3 * h_n)
    lens = torch.tensor(getattr(c, "lengths", None) or [t_n] * b_n).reshape(b_n, 1)
    order = list(range(t_n - 1, -1, -1) if reverse else range(t_n))
    zero = torch.zeros(b_n, h_n)
    hf, hb = c.h0, _r(c.h0)
    hs, rh, gates, hp_f, hp_b = ([None] * t_n for _ in range(5))
    for t in order:
        live = lens > t
        r, u = torch.sigmoid(xg[t][:, :2 * h_n] + hb @ wgh).split(h_n, 1)
        rh[t] = torch.where(live, _r(r * hf), zero)
        cand = torch.tanh(xg[t][:, 2 * h_n:] + rh[t] @ wch)
        hp_f[t], hp_b[t] = hf, hb
        h_new = u * hf + (1 - u) * cand                # u in fp32 here; the backward reads the stored one
        u = _r(u)
        if bf16_carry:
            h_new = _r(h_new)
        hf = torch.where(live, h_new, hf)              # a dead row keeps its state and emits zeros
        hb = _r(hf)
        hs[t] = torch.where(live, hb, zero)
        gates[t] = (_r(r), u, _r(cand))
    carry, dg = c.dh_t.clone(), [None] * t_n
    seen = torch.zeros(b_n, 3 * h_n)                   # per row, dG of the live step this pass handled last
    for t in reversed(order):
        live = lens > t
        r, u, cand = gates[t]
        dh = carry + seen[:, :2 * h_n] @ wgh.t() + c.dhs[t]
        dpc = _r(dh * (1 - u) * (1 - cand * cand))
        dpu = _r(dh * (hp_f[t] - cand) * u * (1 - u))
        d_rh = dpc @ wch.t()
        dpr = _r(d_rh * hp_f[t] * r * (1 - r))
        carry = torch.where(live, dh * u + d_rh * r, carry)
        dg[t] = torch.where(live, torch.cat([dpr, dpu, dpc], 1), torch.zeros(b_n, 3 * h_n))
        seen = torch.where(live, dg[t], seen)
    carry = carry + seen[:, :2 * h_n] @ wgh.t()        # dG of each row's first visited live step (none: zeros)
    dg2 = torch.stack(dg, 0).reshape(t_n * b_n, 3 * h_n)
    dgate, dpc = dg2[:, :2 * h_n], dg2[:, 2 * h_n:]
    hp2, rh2 = torch.stack(hp_b, 0).reshape(t_n * b_n, h_n), torch.stack(rh, 0).reshape(t_n * b_n, h_n)
    dx = dg2 @ wx.t() if dx0 is None else dx0.reshape(t_n * b_n, i_n) + dg2 @ wx.t()
    return dict(zip(GH.NAMES, (torch.stack(hs, 0), hb, _r(dx).reshape(c.x.shape),
                               torch.cat([x2.t() @ dgate, hp2.t() @ dgate], 0), dgate.sum(0),
                               torch.cat([x2.t() @ dpc, rh2.t() @ dpc], 0), dpc.sum(0), _r(carry))))


def _show(what, err):
    print("%s %s" % (what, " ".join("%s=%.3e" % kv for kv in err.items())))
    return err


def lengths_main():
    """The cases and modes of ``tests/test_gru_lengths.py``."""
    import gru_seq_helpers as GS
    worst = {False: dict.fromkeys(GH.NAMES, 0.0), True: dict.fromkeys(GH.NAMES, 0.0)}
    for name in GS.CASES:
        for mode in GS.MODES:
            dx0 = None
            for c, direction, ref in GS.plan(name, mode):
                got = emulate(c, reverse=direction == "bw", dx0=dx0)
                dx0 = got["dx"]
                if mode == "both" and direction == "fw":
                    got = dict(got, dx=ref["dx"])      # the pair's dx is complete after the second direction
                err = _show("case %s %s %s" % (name, mode, direction), GH.errors(got, ref))
                w = worst[name == "carry"]
                w.update({k: max(w[k], err[k]) for k in w})
    for carry, what in ((False, "MEASURED_SEQ"), (True, "MEASURED_SEQ_CARRY")):
        print("%s = {%s}" % (what, ", ".join('"%s": %.2e' % kv for kv in worst[carry].items())))


def main():
    if "--lengths" in sys.argv[1:]:
        return lengths_main()
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
