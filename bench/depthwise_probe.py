#!/usr/bin/env python
"""Depthwise convolution alone: the kernels of csrc/depthwise.hip against the PyTorch expression of the same call.

Per case (batch 128, bf16 NHWC, SAME padding), forward / dgrad / wgrad each, in one process:

  3x3_s1_112x112x32   3x3_s2_112x112x64   3x3_s1_14x14x512   3x3_s1_7x7x1024   5x5_s1_28x28x240   5x5_s2_28x28x240

  native   ``mdtf.nn.depthwise_conv2d`` on the HIP kernels, and the launches its backward makes
           (``ops.depthwise.dgrad_nhwc``; ``wgrad_into``: both phases, fp32 result)
  torch    the same call under ``MDTF_KERNELS=torch``: ``F.conv2d(groups=C)`` on channels-last views (MIOpen), and
           ``aten.convolution_backward`` with one output asked for, which is what autograd calls for its backward

The backward passes are called directly, not through ``autograd.grad``: the backward of a forward that ran before the
capture runs on that forward's stream from the autograd engine's thread, outside the capture.

Each variant is captured ``--iters`` times into a hipGraph (a quarter of that for the comparator); the replay is timed
with device events ``--reps`` times (median, min, max) and the variants alternate ``--rounds`` times.
bytes = x once + y once + the filter (wgrad: x + dy + the fp32 partials); ``floor_us`` is that over 6.3 TB/s, the rate
the BatchNorm passes reach.  ``loses`` is set where the native median is above the comparator's by more than the
comparator's own min .. max spread.  One JSON line per case and pass; ``--markdown`` also writes the table.
Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.image_probe import HBM_BPS, graph_time, with_mode  # noqa: E402

CASES = [("3x3_s1_112x112x32", (112, 112, 32), 3, 1),
         ("3x3_s2_112x112x64", (112, 112, 64), 3, 2),
         ("3x3_s1_14x14x512", (14, 14, 512), 3, 1),
         ("3x3_s1_7x7x1024", (7, 7, 1024), 3, 1),
         ("5x5_s1_28x28x240", (28, 28, 240), 5, 1),
         ("5x5_s2_28x28x240", (28, 28, 240), 5, 2)]


def native_passes(x, w, dy, geo):
    """{pass: fn} on the HIP kernels: the public op, and the two launches its backward makes."""
    from mdtf.ops import depthwise
    from mdtf.ops import nn as ops
    stride = geo[8]
    dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)

    def fwd():
        with torch.no_grad():
            return ops.depthwise_conv2d(x, w, stride, "SAME")
    return {"fwd": fwd,
            "dgrad": lambda: depthwise.dgrad_nhwc(dy, w, geo),
            "wgrad": lambda: depthwise.wgrad_into(x, dy, geo, dw, False)}


def torch_passes(x, w, dy, geo):
    """{pass: fn} of the comparator: the public op under MDTF_KERNELS=torch, and the calls autograd makes for its
    backward (``aten.convolution_backward`` on the same channels-last views, groups = C).  With asymmetric SAME pads the
    PyTorch expression pads the input first; the padded input is made once outside the timed call and the padded dx is
    sliced (a view), so the comparator's backward passes are timed without their pad and slice kernels."""
    import torch.nn.functional as F
    from mdtf.ops import nn as ops
    n, h, wd, c, oh, ow, k, _, s = geo[:9]
    pt, pb, pl, pr = geo[12:16]
    xc, dyc = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    sym = pt == pb and pl == pr
    if not sym:
        xc = F.pad(xc, (pl, pr, pt, pb))
    pad = (pt, pl) if sym else (0, 0)
    wt = w.reshape(k, k, 1, c).permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)

    def bwd(mask):
        return torch.ops.aten.convolution_backward(dyc, xc, wt, None, (s, s), pad, (1, 1), False, (0, 0), c, mask)

    def fwd():
        with torch.no_grad():
            return ops.depthwise_conv2d(x, w, s, "SAME")

    def dgrad():
        dx = bwd((True, False, False))[0]
        if not sym:
            dx = dx[:, :, pt:pt + h, pl:pl + wd]
        return dx.permute(0, 2, 3, 1)
    return {"fwd": fwd, "dgrad": dgrad,
            "wgrad": lambda: bwd((False, True, False))[1].permute(2, 3, 0, 1).reshape(k, k, c, 1)}


def measure(name, which, native, ref, nbytes, args):
    a, b = native().float(), ref().float()
    worst = float((a - b).abs().max())
    scale = float(b.abs().max())
    times = {"native": [], "torch": []}
    for _ in range(args.rounds):
        for key, f in (("native", native), ("torch", ref)):
            times[key].append(graph_time(f, args.iters if key == "native" else max(args.iters // 4, 1), args.reps))
    rec = {"probe": name, "pass": which, "bytes": nbytes, "floor_us": round(nbytes / HBM_BPS * 1e6, 2),
           "max_abs_diff": worst, "max_abs": scale, "iters": args.iters, "reps": args.reps, "rounds": args.rounds}
    for key, ts in times.items():
        med = sorted(t[0] for t in ts)[len(ts) // 2]
        rec[key] = {"us": round(med, 2), "us_min": round(min(t[1] for t in ts), 2),
                    "us_max": round(max(t[2] for t in ts), 2), "TBps": round(nbytes / med / 1e6, 3)}
    n, t = rec["native"], rec["torch"]
    rec["torch_over_native"] = round(t["us"] / n["us"], 2)
    rec["native_over_floor"] = round(n["us"] / rec["floor_us"], 2)
    rec["loses"] = bool(n["us"] - t["us"] > t["us_max"] - t["us_min"])
    print(json.dumps(rec), flush=True)
    return rec


def markdown(recs, path):
    lines = ["| case | pass | bytes | native us (min .. max) | TB/s | torch us (min .. max) | torch / native | "
             "floor us at 6.3 TB/s | native / floor | loses |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        n, t = r["native"], r["torch"]
        lines.append("| %s | %s | %d | %.1f (%.1f .. %.1f) | %.2f | %.1f (%.1f .. %.1f) | %.2f | %.1f | %.1f | %s |"
                     % (r["probe"], r["pass"], r["bytes"], n["us"], n["us_min"], n["us_max"], n["TBps"], t["us"],
                        t["us_min"], t["us_max"], r["torch_over_native"], r["floor_us"], r["native_over_floor"],
                        "yes" if r["loses"] else ""))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20, help="calls per captured graph")
    p.add_argument("--reps", type=int, default=9, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    p.add_argument("--markdown", default="", help="also write the table to this file")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("depthwise_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native, depthwise
    _native.lib()
    wanted = [c for c in args.cases.split(",") if c]
    gen = torch.Generator().manual_seed(0)
    recs = []
    for name, (h, wd, c), k, s in CASES:
        if wanted and name not in wanted:
            continue
        oh, ow = -(-h // s), -(-wd // s)
        x = torch.randn((args.batch, h, wd, c), generator=gen).cuda().bfloat16()
        w = (torch.randn((k, k, c, 1), generator=gen) * 0.3).cuda().bfloat16()
        dy = torch.randn((args.batch, oh, ow, c), generator=gen).cuda().bfloat16()
        from mdtf.ops.padding import conv_geometry
        _, _, pt, pb, pl, pr = conv_geometry(h, wd, k, k, (s, s), "SAME")
        geo = [args.batch, h, wd, c, oh, ow, k, k, s, s, 1, 1, pt, pb, pl, pr]
        native, ref = native_passes(x, w, dy, geo), torch_passes(x, w, dy, geo)
        ws = int(_native.fn("mdtf_dwconv_wgrad_ws")(args.batch, oh, ow, c, k, k))
        assert depthwise.native_ok(x, w)
        io = 2 * (x.numel() + dy.numel())
        nbytes = {"fwd": io + 2 * w.numel(), "dgrad": io + 2 * w.numel(), "wgrad": io + 4 * ws}
        for which in ("fwd", "dgrad", "wgrad"):
            recs.append(measure(name, which, with_mode("native", native[which]), with_mode("torch", ref[which]),
                                nbytes[which], args))
        del native, ref, x, w, dy
    if args.markdown:
        markdown(recs, args.markdown)


if __name__ == "__main__":
    main()
