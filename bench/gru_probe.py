#!/usr/bin/env python
"""GRU over a whole sequence: the kernels of csrc/gru.hip against the PyTorch loop and ``torch.nn.GRU``.

(T, B, H) = (35, 64, 1024), (35, 128, 1536), (128, 32, 512), each with I = H, bf16, time-major, in one process:

  native   ``mdtf.ops.gru.gru`` on the HIP path: one dense forward for the input half, one pack launch and 2T step
           launches; backward: 2T + 1 step launches, the four weight-gradient GEMMs into fp32 slots and dx
  loop     the same call under ``MDTF_KERNELS=torch``: ``gru.gru_loop`` and its autograd backward
  nn.GRU   ``torch.nn.GRU`` (one layer, bf16), for context only: it is the reset-after cell (the reset gate scales
           the candidate's recurrent product, so that product does not wait for r), a different recurrence

``fwd`` is the forward alone under ``no_grad``; ``fwd+bwd`` a forward and the gradients of x, the four variables and
the initial state for random output gradients.  Each variant is captured ``--iters`` times into a hipGraph (warm-up
calls first) and the replay is timed with device events ``--reps`` times (median, min, max); the variants alternate
``--rounds`` times.  One JSON line per shape and pass.  Needs a GPU.

``--units`` times the recurrences alone through the entry points (no input GEMM, no weight gradients) with the
units per block forced to every (gate launch, other launches) pair of 16 and 32, per step (a forward step is its two
launches, a backward step two of its 2T + 1): what decides ``pick_u`` in csrc/gru.hip.

``--trace T,B,H`` runs the recurrences a few times with both block widths and nothing else, as the program of a
kernel-trace profiler run, which gives the time of each of the four step kernels.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.image_probe import graph_time, with_mode  # noqa: E402
from bench.lstm_probe import SHAPES, _Slot  # noqa: E402


def mdtf_passes(t, b, h, gen):
    from mdtf.ops import gru
    dev = "cuda"
    x = torch.randn((t, b, h), generator=gen).to(dev).bfloat16().requires_grad_(True)
    params = []
    for cols in (2 * h, h):
        k = (torch.randn((2 * h, cols), generator=gen) * (2 * h) ** -0.5).to(dev).bfloat16().requires_grad_(True)
        bias = torch.zeros(cols, device=dev, dtype=torch.bfloat16).requires_grad_(True)
        k._mdtf_var, bias._mdtf_var = _Slot(torch.zeros((2 * h, cols), device=dev)), _Slot(torch.zeros(cols, device=dev))
        params += [k, bias]
    h0 = torch.zeros((b, h), device=dev, dtype=torch.bfloat16).requires_grad_(True)
    dhs = torch.randn((t, b, h), generator=gen).to(dev).bfloat16()

    def fwd():
        with torch.no_grad():
            return gru.gru(x, *params, h0)[0]

    def both():
        return torch.autograd.grad([gru.gru(x, *params, h0)[0]], [x] + params + [h0], [dhs])[0]
    return {"fwd": fwd, "fwd+bwd": both}


def library_passes(t, b, h, gen):
    net = torch.nn.GRU(h, h).cuda().bfloat16()
    x = torch.randn((t, b, h), generator=gen).cuda().bfloat16().requires_grad_(True)
    dhs = torch.randn((t, b, h), generator=gen).cuda().bfloat16()
    params = [x] + list(net.parameters())

    def fwd():
        with torch.no_grad():
            return net(x)[0]

    def both():
        return torch.autograd.grad([net(x)[0]], params, [dhs])[0]
    return {"fwd": fwd, "fwd+bwd": both}


def recurrence(t, b, h, gen):
    """The recurrences alone through the entry points, on buffers made once: ``(forward, backward)``."""
    from mdtf.ops import _native as N, gru
    new = lambda *shape, dtype=torch.bfloat16, scale=1.0: (torch.randn(shape, generator=gen) * scale).cuda().to(dtype)
    f32 = torch.float32
    z = dict(xg=new(t, b, 3 * h), wg=new(h, 2 * h, scale=(2 * h) ** -0.5), wc=new(h, h, scale=(2 * h) ** -0.5),
             wt=new(3 * h * h), h0=new(b, h, scale=0.5), hs=new(t, b, h), hf=new(t, b, h, dtype=f32), rh=new(t, b, h),
             gates=new(t, b, 3 * h), dhs=new(t, b, h), carry=new(b, h, dtype=f32), dg=new(t, b, 3 * h))
    z["h0f"] = z["h0"].float()
    P = N.ptr
    fa = [z[k] for k in ("xg", "wg", "wc", "wt", "h0", "h0f", "hs", "hf", "rh", "gates")]
    ba = [z[k] for k in ("wg", "wc", "gates", "hf", "h0f", "dhs", "carry", "dg")]
    return (lambda: N.check(N.fn("mdtf_gru_fwd")(*[P(v) for v in fa], t, b, h, gru.BF16, N.stream_ptr()), "gru_fwd"),
            lambda: N.check(N.fn("mdtf_gru_bwd")(*[P(v) for v in ba], t, b, h, gru.BF16, N.stream_ptr()), "gru_bwd"))


def force_units(gate, cand):
    from mdtf.ops import _native as N
    N.check(N.fn("mdtf_gru_force_units")(gate, cand), "gru_force_units")


def units_probe(args, gen):
    from mdtf.ops import gru
    pairs = [(16, 16), (32, 32), (32, 16), (16, 32)]
    for t, b, h in SHAPES:
        passes = recurrence(t, b, h, gen)
        for i, which in enumerate(("fwd", "bwd")):
            rec = {"probe": "gru_units", "T": t, "B": b, "H": h, "pass": which, "rule": gru.units_per_block(t, b, h),
                   "iters": args.iters, "reps": args.reps, "rounds": args.rounds}
            times = {p: [] for p in pairs}
            for _ in range(args.rounds):
                for p in pairs:
                    force_units(*p)
                    times[p].append(graph_time(passes[i], args.iters, args.reps))
                    force_units(0, 0)
            for p, ts in times.items():
                rec["gate%d_rest%d" % p] = {"step_us": round(sorted(x[0] for x in ts)[len(ts) // 2] / t, 2),
                                            "step_us_min": round(min(x[1] for x in ts) / t, 2),
                                            "step_us_max": round(max(x[2] for x in ts) / t, 2)}
            print(json.dumps(rec), flush=True)


def trace_program(shape, gen):
    t, b, h = (int(v) for v in shape.split(","))
    fwd, bwd = recurrence(t, b, h, gen)
    for u in (16, 32):
        force_units(u, u)
        for _ in range(5):
            fwd()
            bwd()
    force_units(0, 0)
    torch.cuda.synchronize()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3, help="sequences per captured graph")
    p.add_argument("--reps", type=int, default=7, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    p.add_argument("--units", action="store_true", help="time the recurrences alone with forced units per block")
    p.add_argument("--trace", default=None, metavar="T,B,H", help="run the recurrences only (for a kernel trace)")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("gru_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native, gru
    _native.lib()
    gen = torch.Generator().manual_seed(0)
    if args.trace:
        return trace_program(args.trace, gen)
    if args.units:
        return units_probe(args, gen)
    for t, b, h in SHAPES:
        ours, lib = mdtf_passes(t, b, h, gen), library_passes(t, b, h, gen)
        for which in ("fwd", "fwd+bwd"):
            variants = {"native": with_mode("native", ours[which]), "loop": with_mode("torch", ours[which]),
                        "nn.GRU": lib[which]}
            a, ref = variants["native"]().float(), variants["loop"]().float()
            rec = {"probe": "gru", "T": t, "B": b, "H": h, "pass": which, "units_per_block": gru.units_per_block(t, b, h),
                   "native_vs_loop_max_abs_diff": float((a - ref).abs().max()), "max_abs": float(ref.abs().max()),
                   "iters": args.iters, "reps": args.reps, "rounds": args.rounds}
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for key, f in variants.items():
                    if key in rec:                 # failed in an earlier round
                        continue
                    try:
                        times[key].append(graph_time(f, args.iters, args.reps))
                    except RuntimeError as e:      # e.g. a library RNN that cannot be captured
                        rec[key] = {"error": str(e).splitlines()[0][:160]}
            for key, ts in times.items():
                if ts and key not in rec:
                    med = sorted(x[0] for x in ts)[len(ts) // 2]
                    rec[key] = {"us": round(med, 1), "us_min": round(min(x[1] for x in ts), 1),
                                "us_max": round(max(x[2] for x in ts), 1)}
            rec["loop_over_native"] = round(rec["loop"]["us"] / rec["native"]["us"], 2)
            if which == "fwd":
                rec["step_us"] = round(rec["native"]["us"] / t, 2)
            print(json.dumps(rec), flush=True)
        del ours, lib


if __name__ == "__main__":
    main()
