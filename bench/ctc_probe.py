#!/usr/bin/env python
"""CTC loss: the kernels of csrc/ctc.hip against ``torch.nn.functional.ctc_loss`` on the GPU, in one process.

(T, B, K, L) = (800, 64, 32, 120) a character model, (400, 32, 8192, 60) a word-piece model (the row kernels'
block-per-row form), (100, 64, 32, 20) a short one on the wave variant; bf16 logits, time-major, frame lengths uniform
in T/2 .. T and label lengths in L/2 .. L.

  native   ``mdtf.nn.ctc_loss`` on the HIP path: two launches forward, one backward
  torch    the same call under ``MDTF_KERNELS=torch``: ``F.ctc_loss`` over an fp32 ``log_softmax``

``fwd`` is the loss alone under ``no_grad``; ``fwd+bwd`` the loss and the gradient of the logits for a random upstream.
Each variant is captured into a hipGraph (warm-up calls first), at least ``--iters`` calls and as many as make one
replay 3 ms long (``calls`` in the output), and the replay is timed with device events ``--reps`` times (median, min,
max); the variants alternate ``--rounds`` times.  A variant that cannot be
captured (a library op that reads its lengths on the host) is timed eagerly instead, with a device synchronise, and
marked ``"eager": true``.  A second line per shape times the three entry points alone on buffers made once:
``step_us`` is the recurrence per time step (both directions run side by side), ``rows`` and ``grad`` stand against
their byte floors at 6.3 TB/s (read x, write lpc; read x, write dx).  One JSON line each.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.image_probe import HBM_BPS, graph_time, with_mode  # noqa: E402

SHAPES = [("char", 800, 64, 32, 120), ("wordpiece", 400, 32, 8192, 60), ("short", 100, 64, 32, 20)]


def eager_time(fn, iters, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def inputs(t, b, k, lmax, gen):
    x = (torch.randn((t, b, k), generator=gen) * 2).cuda().bfloat16().requires_grad_(True)
    labels = torch.randint(0, k - 1, (b, lmax), generator=gen, dtype=torch.int32).cuda()
    seq = torch.randint(t // 2, t + 1, (b,), generator=gen, dtype=torch.int32).cuda()
    ln = torch.randint(lmax // 2, lmax + 1, (b,), generator=gen, dtype=torch.int32).cuda()
    return x, labels, seq, ln, torch.randn(b, generator=gen).cuda()


def passes(x, labels, seq, ln, g):
    import mdtf

    def fwd():
        with torch.no_grad():
            return mdtf.nn.ctc_loss(labels, x, seq, label_length=ln)

    def both():
        return torch.autograd.grad([mdtf.nn.ctc_loss(labels, x, seq, label_length=ln)], [x], [g])[0]
    return {"fwd": fwd, "fwd+bwd": both}


def entry_points(x, labels, seq, ln, g):
    from mdtf.ops import _native as N, ctc  # noqa: F401
    t, b, k = x.shape
    lmax = labels.shape[1]
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    lse, lpc, chain, flag = new(t, b), new(t, b, lmax + 1), new(b, lmax, dtype=torch.int32), new(b, dtype=torch.int32)
    alpha, beta, loss, dx = new(t, b, 2 * lmax + 1), new(t, b, 2 * lmax + 1), new(b), torch.zeros_like(x)
    xd = x.detach()
    P, dims = N.ptr, lambda: (t, b, k, lmax, ctc.BF16, N.stream_ptr())
    lens = (P(labels), P(seq), P(ln))
    return {"rows": lambda: N.check(N.fn("mdtf_ctc_rows")(P(xd), *lens, P(lse), P(lpc), P(chain), P(flag), *dims()),
                                    "ctc_rows"),
            "alpha_beta": lambda: N.check(N.fn("mdtf_ctc_alpha_beta")(P(lpc), *lens, P(flag), P(alpha), P(beta),
                                                                      P(loss), 0, *dims()), "ctc_alpha_beta"),
            "grad": lambda: N.check(N.fn("mdtf_ctc_grad")(P(xd), *lens, P(flag), P(chain), P(lse), P(lpc), P(alpha),
                                                          P(beta), P(loss), P(g), P(dx), *dims()), "ctc_grad")}


WINDOW_US = 3000.0              # a timed replay covers at least this much work


def measure(variants, args):
    """us per call of every variant; the calls per graph grow from ``--iters`` until one replay is WINDOW_US long."""
    times, eager, iters = {k: [] for k in variants}, set(), {k: args.iters for k in variants}
    for rnd in range(args.rounds + 1):             # round 0 sizes the windows and is dropped
        for key, f in variants.items():
            if key not in eager:
                try:
                    got = graph_time(f, iters[key], args.reps)
                except RuntimeError:
                    eager.add(key)
                    torch.cuda.synchronize()
            if key in eager:
                got = eager_time(f, iters[key], args.reps)
            if rnd == 0:
                iters[key] = max(args.iters, min(256, int(WINDOW_US / max(got[0], 1.0)) + 1))
            else:
                times[key].append(got)
    out = {}
    for key, ts in times.items():
        out[key] = {"us": round(sorted(x[0] for x in ts)[len(ts) // 2], 1), "us_min": round(min(x[1] for x in ts), 1),
                    "us_max": round(max(x[2] for x in ts), 1), "calls": iters[key]}
        if key in eager:
            out[key]["eager"] = True
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3, help="calls per captured graph")
    p.add_argument("--reps", type=int, default=7, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("ctc_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native
    _native.lib()
    gen = torch.Generator().manual_seed(0)
    for name, t, b, k, lmax in SHAPES:
        data = inputs(t, b, k, lmax, gen)
        ours = passes(*data)
        for which in ("fwd", "fwd+bwd"):
            variants = {"native": with_mode("native", ours[which]), "torch": with_mode("torch", ours[which])}
            a, ref = variants["native"]().float(), variants["torch"]().float()
            rec = {"probe": "ctc", "shape": name, "T": t, "B": b, "K": k, "Lmax": lmax, "pass": which,
                   "variant": "wave" if 2 * lmax + 1 <= 64 else "block",
                   "native_vs_torch_max_abs_diff": float((a - ref).abs().max()), "max_abs": float(ref.abs().max()),
                   "iters": args.iters, "reps": args.reps, "rounds": args.rounds}
            rec.update(measure(variants, args))
            rec["torch_over_native"] = round(rec["torch"]["us"] / rec["native"]["us"], 2)
            print(json.dumps(rec), flush=True)
        rec = {"probe": "ctc_entry_points", "shape": name, "T": t, "B": b, "K": k, "Lmax": lmax}
        rec.update(measure(entry_points(*data), args))
        live = int(data[2].sum())                  # rows that are read
        floors = {"rows": live * (2 * k + 4 * (lmax + 2)), "grad": live * 2 * k + t * b * 2 * k}
        for key, nbytes in floors.items():
            rec[key]["floor_us"] = round(nbytes / HBM_BPS * 1e6, 2)
        rec["step_us"] = round(rec["alpha_beta"]["us"] / t, 3)
        print(json.dumps(rec), flush=True)
        del data, ours


if __name__ == "__main__":
    main()
