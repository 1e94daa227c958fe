#!/usr/bin/env python
"""LSTM over a whole sequence: the kernels of csrc/lstm.hip against the PyTorch loop and ``torch.nn.LSTM``.

(T, B, H) = (35, 64, 1024), (35, 128, 1536), (128, 32, 512), each with I = H, bf16, time-major, in one process:

  native   ``mdtf.ops.rnn.lstm`` on the HIP path: one dense forward for the input half, one pack launch and T step
           launches; backward: T + 1 step launches, the two kernel-gradient GEMMs into an fp32 slot and dx
  loop     the same call under ``MDTF_KERNELS=torch``: ``rnn.lstm_loop`` and its autograd backward
  nn.LSTM  ``torch.nn.LSTM`` (one layer, bf16; the library's fused RNN), as a yardstick outside this package

``fwd`` is the forward alone under ``no_grad``; ``fwd+bwd`` a forward and the gradients of x, kernel, bias and the
initial state for random output gradients.  Each variant is captured ``--iters`` times into a hipGraph (warm-up calls
first) and the replay is timed with device events ``--reps`` times (median, min, max); the variants alternate
``--rounds`` times.  ``step_us`` is the native forward per time step, to hold against the dependent-launch floor.
``loses`` is set where the native median is above ``nn.LSTM``'s by more than that one's own min .. max spread.  One
JSON line per shape and pass.  Needs a GPU.

``--lengths {full,uniform,sorted}`` and ``--bidirectional`` time the recurrences alone instead (no input GEMM, no
weight gradients), per step, at the same shapes: what the length test costs a full-length batch, what skipping dead
tiles saves a ragged one, and one fused two-direction call against two calls (``recurrence_passes``).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.image_probe import graph_time, with_mode  # noqa: E402

SHAPES = [(35, 64, 1024), (35, 128, 1536), (128, 32, 512)]


class _Slot(object):
    """What ``variables.grad_sink`` looks for: an fp32 gradient slot."""

    def __init__(self, grad):
        self.grad = grad


def mdtf_passes(t, b, h, gen):
    from mdtf.ops import rnn
    x = torch.randn((t, b, h), generator=gen).cuda().bfloat16().requires_grad_(True)
    kernel = (torch.randn((2 * h, 4 * h), generator=gen) * (2 * h) ** -0.5).cuda().bfloat16().requires_grad_(True)
    bias = torch.zeros(4 * h, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
    kernel._mdtf_var = _Slot(torch.zeros((2 * h, 4 * h), device="cuda"))
    bias._mdtf_var = _Slot(torch.zeros(4 * h, device="cuda"))
    h0 = torch.zeros((b, h), device="cuda", dtype=torch.bfloat16).requires_grad_(True)
    c0 = torch.zeros((b, h), device="cuda").requires_grad_(True)
    dhs = torch.randn((t, b, h), generator=gen).cuda().bfloat16()

    def fwd():
        with torch.no_grad():
            return rnn.lstm(x, kernel, bias, h0, c0)[0]

    def both():
        hs = rnn.lstm(x, kernel, bias, h0, c0)[0]
        return torch.autograd.grad([hs], [x, kernel, bias, h0, c0], [dhs])[0]
    return {"fwd": fwd, "fwd+bwd": both}


def library_passes(t, b, h, gen):
    net = torch.nn.LSTM(h, h).cuda().bfloat16()
    x = torch.randn((t, b, h), generator=gen).cuda().bfloat16().requires_grad_(True)
    dhs = torch.randn((t, b, h), generator=gen).cuda().bfloat16()
    params = [x] + list(net.parameters())

    def fwd():
        with torch.no_grad():
            return net(x)[0]

    def both():
        return torch.autograd.grad([net(x)[0]], params, [dhs])[0]
    return {"fwd": fwd, "fwd+bwd": both}


def probe_lengths(kind, t, b, gen):
    """``full``: every row T; ``uniform``: uniform in 1 .. T, in batch order; ``sorted``: the same, longest first (a
    bucketed batch: the rows of a 16-row tile die together)."""
    if kind == "full":
        return torch.full((b,), t, dtype=torch.int32)
    lens = torch.randint(1, t + 1, (b,), generator=gen, dtype=torch.int32)
    return lens.sort(descending=True)[0] if kind == "sorted" else lens


def recurrence_passes(t, b, h, gen, lens, bidirectional):
    """The recurrences alone through the entry points, on buffers made once: name -> (forward, backward).  ``plain``:
    ``mdtf_lstm_fwd`` / ``mdtf_lstm_bwd`` (no lengths, the kernels of the full-length path before lengths existed);
    ``seq-full`` / ``seq-<kind>``: the length-aware kernels without and with ``lens``; ``bidirectional``: ``fused``
    (both directions in every launch) and ``two-calls`` (a forward then a reverse call), both with ``lens``."""
    from mdtf.ops import _native as N, rnn
    dev, st = "cuda", N.stream_ptr
    new = lambda *shape, dtype=torch.bfloat16: torch.randn(shape, generator=gen).to(dev).to(dtype)

    def direction():
        d = dict(xg=new(t, b, 4 * h), wh=new(h, 4 * h) * (2 * h) ** -0.5, wt=new(4 * h * h), h0=new(b, h) * 0.5,
                 c0=new(b, h, dtype=torch.float32) * 0.5, hs=new(t, b, h), cs=new(t, b, h, dtype=torch.float32),
                 gates=new(t, b, 4 * h), h_fin=new(b, h), c_fin=new(b, h, dtype=torch.float32), dhs=new(t, b, h),
                 dh_t=new(b, h), carry=new(b, h, dtype=torch.float32), dg=new(t, b, 4 * h), dh0=new(b, h))
        d["wh"] = d["wh"].contiguous()
        d["fwd"] = tuple(d[k] for k in ("xg", "wh", "wt", "h0", "c0", "hs", "cs", "gates", "h_fin", "c_fin"))
        d["bwd"] = tuple(d[k] for k in ("wh", "gates", "cs", "c0", "dhs", "dh_t", "carry", "dg", "dh0"))
        return d
    a, z = direction(), direction()
    lens = lens.to(dev)

    def seq(dirs, reverse, lengths):
        ft, bt = rnn._table([d["fwd"] for d in dirs]), rnn._table([d["bwd"] for d in dirs])
        return (lambda: N.check(N.fn("mdtf_lstm_fwd_seq")(ft, len(dirs), reverse, N.ptr(lengths), t, b, h, 4 * h, 1.0,
                                                          rnn.BF16, st()), "lstm_fwd_seq"),
                lambda: N.check(N.fn("mdtf_lstm_bwd_seq")(bt, len(dirs), reverse, N.ptr(lengths), t, b, h, rnn.BF16,
                                                          st()), "lstm_bwd_seq"))
    if bidirectional:
        (f_a, b_a), (f_z, b_z) = seq([a], 0, lens), seq([z], 1, lens)
        return {"fused": seq([a, z], 0b10, lens), "two-calls": (lambda: (f_a(), f_z()), lambda: (b_a(), b_z()))}
    P = N.ptr
    plain = (lambda: N.check(N.fn("mdtf_lstm_fwd")(*[P(x) for x in a["fwd"][:8]], t, b, h, 1.0, rnn.BF16, st()), "lstm_fwd"),
             lambda: N.check(N.fn("mdtf_lstm_bwd")(*[P(x) for x in a["bwd"]], t, b, h, rnn.BF16, st()), "lstm_bwd"))
    return {"plain": plain, "seq-full": seq([a], 0, None), "seq-lengths": seq([a], 0, lens)}


def recurrence_probe(args, gen):
    """One JSON line per shape and pass: us per step of every variant of :func:`recurrence_passes`, median (min, max)
    over the replays, the variants alternating ``--rounds`` times.  A backward "step" is one of its T + 1 launches."""
    for t, b, h in SHAPES:
        lens = probe_lengths(args.lengths or "full", t, b, gen)
        variants = recurrence_passes(t, b, h, gen, lens, args.bidirectional)
        for i, which in enumerate(("fwd", "bwd")):
            rec = {"probe": "lstm_recurrence", "T": t, "B": b, "H": h, "pass": which, "lengths": args.lengths or "full",
                   "mean_length": round(float(lens.float().mean()), 1), "iters": args.iters, "reps": args.reps,
                   "rounds": args.rounds}
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for key, fs in variants.items():
                    times[key].append(graph_time(fs[i], args.iters, args.reps))
            for key, ts in times.items():
                steps = t + i
                rec[key] = {"step_us": round(sorted(x[0] for x in ts)[len(ts) // 2] / steps, 2),
                            "step_us_min": round(min(x[1] for x in ts) / steps, 2),
                            "step_us_max": round(max(x[2] for x in ts) / steps, 2)}
            print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3, help="sequences per captured graph")
    p.add_argument("--reps", type=int, default=7, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    p.add_argument("--lengths", choices=["full", "uniform", "sorted"], default=None,
                   help="time the recurrences alone with these per-row lengths (see recurrence_passes)")
    p.add_argument("--bidirectional", action="store_true",
                   help="time one fused two-direction call against two one-direction calls")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("lstm_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native, rnn
    _native.lib()
    gen = torch.Generator().manual_seed(0)
    if args.lengths or args.bidirectional:
        return recurrence_probe(args, gen)
    for t, b, h in SHAPES:
        ours, lib = mdtf_passes(t, b, h, gen), library_passes(t, b, h, gen)
        for which in ("fwd", "fwd+bwd"):
            variants = {"native": with_mode("native", ours[which]), "loop": with_mode("torch", ours[which]),
                        "nn.LSTM": lib[which]}
            a, ref = variants["native"]().float(), variants["loop"]().float()
            rec = {"probe": "lstm", "T": t, "B": b, "H": h, "pass": which, "units_per_block": rnn.units_per_block(t, b, h),
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
            n, y = rec["native"], rec["nn.LSTM"]
            rec["loop_over_native"] = round(rec["loop"]["us"] / n["us"], 2)
            if which == "fwd":
                rec["step_us"] = round(n["us"] / t, 2)
            if "us" in y:
                rec["nn_lstm_over_native"] = round(y["us"] / n["us"], 2)
                rec["loses"] = bool(n["us"] - y["us"] > y["us_max"] - y["us_min"])
            print(json.dumps(rec), flush=True)
        del ours, lib


if __name__ == "__main__":
    main()
