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

``--lengths`` times per-row lengths (uniform random in [T/2, T], an int32 device tensor) and two directions.  Whole
layer: ``full`` (no lengths, forward in time), ``lens``, ``bi`` (``gru.bigru``: a forward and a reverse GRU in the
same launches) and ``two calls`` (the same pair as ``gru.gru`` + ``gru.gru(reverse=True)``) on the HIP path, ``lens``
and ``bi`` also as the PyTorch loop.  Recurrences alone: ``mdtf_gru_fwd`` / ``mdtf_gru_bwd`` (the full-length
kernels) against ``mdtf_gru_fwd_seq`` / ``mdtf_gru_bwd_seq`` without lengths, with them, and with two directions.

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


def _direction(h, gen):
    """``(gates kernel, gates bias, candidate kernel, candidate bias, h0)`` with fp32 gradient slots, I = H."""
    out = []
    for cols in (2 * h, h):
        k = (torch.randn((2 * h, cols), generator=gen) * (2 * h) ** -0.5).cuda().bfloat16().requires_grad_(True)
        bias = torch.zeros(cols, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
        k._mdtf_var, bias._mdtf_var = _Slot(torch.zeros((2 * h, cols), device="cuda")), _Slot(torch.zeros(cols, device="cuda"))
        out += [k, bias]
    return out


def lengths_passes(t, b, h, lens, gen):
    """``{variant: {pass: fn}}`` of the whole layer with lengths and two directions (``--lengths``)."""
    from mdtf.ops import gru
    x = torch.randn((t, b, h), generator=gen).cuda().bfloat16().requires_grad_(True)
    fw, bw = _direction(h, gen), _direction(h, gen)
    h0 = torch.zeros((b, h), device="cuda", dtype=torch.bfloat16)
    dhs = torch.randn((t, b, h), generator=gen).cuda().bfloat16()
    calls = {"full": lambda: [gru.gru(x, *fw, h0)[0]],
             "lens": lambda: [gru.gru(x, *fw, h0, lens)[0]],
             "bi": lambda: [r[0] for r in gru.bigru(x, fw + [h0], bw + [h0], lens)],
             "two calls": lambda: [gru.gru(x, *fw, h0, lens)[0], gru.gru(x, *bw, h0, lens, reverse=True)[0]]}

    def passes(call, leaves):
        def fwd():
            with torch.no_grad():
                return call()[0]

        def both():
            ys = call()
            return torch.autograd.grad(ys, leaves, [dhs] * len(ys))[0]
        return {"fwd": fwd, "fwd+bwd": both}
    out = {k: passes(f, [x] + fw + (bw if k in ("bi", "two calls") else [])) for k, f in calls.items()}
    for k in ("lens", "bi"):
        out[k + " loop"] = {which: with_mode("torch", f) for which, f in out[k].items()}
    return out


def seq_recurrence(t, b, h, lens, ndir, gen):
    """The length-aware recurrences alone through the entry points: ``(forward, backward)``."""
    from mdtf.ops import _native as N, gru, rnn
    new = lambda *shape, dtype=torch.bfloat16, scale=1.0: (torch.randn(shape, generator=gen) * scale).cuda().to(dtype)
    f32 = torch.float32
    xg, fwd, bwd = new(t, b, 3 * h * ndir), [], []
    for d in range(ndir):
        z = dict(wg=new(h, 2 * h, scale=(2 * h) ** -0.5), wc=new(h, h, scale=(2 * h) ** -0.5), wt=new(3 * h * h),
                 h0=new(b, h, scale=0.5), hs=new(t, b, h), hf=new(t, b, h, dtype=f32), rh=new(t, b, h),
                 gates=new(t, b, 3 * h), h_fin=new(b, h), dhs=new(t, b, h), carry=new(b, h, dtype=f32), dg=new(t, b, 3 * h))
        z["h0f"] = z["h0"].float()
        fwd.append([xg[:, :, 3 * h * d:]] + [z[k] for k in ("wg", "wc", "wt", "h0", "h0f", "hs", "hf", "rh", "gates", "h_fin")])
        bwd.append([z[k] for k in ("wg", "wc", "gates", "hf", "h0f", "dhs", "carry", "dg")])
    rev = 0b10 if ndir == 2 else 0
    return (lambda: N.check(N.fn("mdtf_gru_fwd_seq")(rnn._table(fwd), ndir, rev, N.ptr(lens), t, b, h, 3 * h * ndir,
                                                     gru.BF16, N.stream_ptr()), "gru_fwd_seq"),
            lambda: N.check(N.fn("mdtf_gru_bwd_seq")(rnn._table(bwd), ndir, rev, N.ptr(lens), t, b, h, gru.BF16,
                                                     N.stream_ptr()), "gru_bwd_seq"))


def _timed(variants, args):
    """``{variant: {"us", "us_min", "us_max"}}``, the variants alternating ``args.rounds`` times."""
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for key, f in variants.items():
            times[key].append(graph_time(f, args.iters, args.reps))
    return {k: {"us": round(sorted(x[0] for x in ts)[len(ts) // 2], 1), "us_min": round(min(x[1] for x in ts), 1),
                "us_max": round(max(x[2] for x in ts), 1)} for k, ts in times.items()}


def lengths_probe(args, gen):
    for t, b, h in SHAPES:
        lens = torch.randint(t // 2, t + 1, (b,), generator=gen).to(torch.int32).cuda()
        base = {"T": t, "B": b, "H": h, "mean_length": round(float(lens.float().mean()), 1), "iters": args.iters,
                "reps": args.reps, "rounds": args.rounds}
        layer = lengths_passes(t, b, h, lens, gen)
        for which in ("fwd", "fwd+bwd"):
            rec = dict(base, probe="gru_lengths", **{"pass": which})
            rec.update(_timed({k: v[which] for k, v in layer.items()}, args))
            rec["loop_over_native"] = {k: round(rec[k + " loop"]["us"] / rec[k]["us"], 2) for k in ("lens", "bi")}
            print(json.dumps(rec), flush=True)
        del layer
        old = recurrence(t, b, h, gen)
        seq = {"seq": seq_recurrence(t, b, h, None, 1, gen), "seq lens": seq_recurrence(t, b, h, lens, 1, gen),
               "seq bi lens": seq_recurrence(t, b, h, lens, 2, gen)}
        for i, which in enumerate(("fwd", "bwd")):
            rec = dict(base, probe="gru_lengths_recurrence", **{"pass": which})
            rec.update(_timed(dict({"full-length kernels": old[i]}, **{k: v[i] for k, v in seq.items()}), args))
            print(json.dumps(rec), flush=True)


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
    p.add_argument("--lengths", action="store_true", help="time per-row lengths and two directions")
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
    if args.lengths:
        return lengths_probe(args, gen)
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
