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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3, help="sequences per captured graph")
    p.add_argument("--reps", type=int, default=7, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("lstm_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native, rnn
    _native.lib()
    gen = torch.Generator().manual_seed(0)
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
