#!/usr/bin/env python
"""Grouped 3x3 convolution alone: the kernels of csrc/conv_group.hip against the library route of the same call.

The conv2 shapes of ResNeXt-50 32x4d (bf16 NHWC, batch 256), forward / dgrad / wgrad each, in one process:

  stride 1 (SAME)          56x56x128 cg4    28x28x256 cg8    14x14x512 cg16    7x7x1024 cg32
  stride 2 (pad 1, as the  56x56x256 cg8    28x28x512 cg16   14x14x1024 cg32
  first unit of a stage)

  native   ``mdtf.nn.conv2d(groups=G)`` on the HIP kernels, and the launches its backward makes
           (``ops.grouped.dgrad_nhwc``; ``wgrad_into``: both phases, fp32 result)
  torch    the same call under ``MDTF_KERNELS=torch``: ``F.conv2d(groups=G)`` on channels-last views (MIOpen), and
           ``aten.convolution_backward`` with one output asked for, which is what autograd calls for its backward

Each variant is captured ``--iters`` times into a hipGraph (warm-up replays first); the replay is timed with device
events ``--reps`` times (median, min, max) and the variants alternate ``--rounds`` times in the same process.
bytes = x once + y once + the filter (wgrad: x + dy + the fp32 partials).  ``floor_us`` is that over the copy rate this
machine reaches (the ``copy`` line of ``bench/hbm_probe.py``, measured here the same way at the start of the run).
``loses`` is set where the native median is above the comparator's by more than the comparator's own min .. max
spread.  One JSON line per case and pass; ``--markdown`` also writes the table.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.image_probe import graph_time, with_mode  # noqa: E402

#        name                 H   W   C     Cg  stride
CASES = [("s1_56x56x128_cg4", 56, 56, 128, 4, 1),
         ("s1_28x28x256_cg8", 28, 28, 256, 8, 1),
         ("s1_14x14x512_cg16", 14, 14, 512, 16, 1),
         ("s1_7x7x1024_cg32", 7, 7, 1024, 32, 1),
         ("s2_56x56x256_cg8", 56, 56, 256, 8, 2),
         ("s2_28x28x512_cg16", 28, 28, 512, 16, 2),
         ("s2_14x14x1024_cg32", 14, 14, 1024, 32, 2)]


def copy_rate():
    """Bytes per second of a device copy of 2 x 411 MB (bench/hbm_probe.py's ``copy``): median of 20 after 3."""
    n = 256 * 56 * 56 * 256
    x = torch.randn(n, device="cuda").bfloat16()
    y = torch.empty_like(x)
    ts = []
    for i in range(23):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y.copy_(x)
        b.record()
        b.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b))
    return 4 * n / (statistics.median(ts) * 1e-3)


def native_passes(x, w, dy, geo):
    from mdtf.ops import grouped
    from mdtf.ops import nn as ops
    groups, s, pads = geo[3] // geo[4], geo[9], tuple(geo[11:15])
    dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)

    def fwd():
        with torch.no_grad():
            return ops.conv2d(x, w, s, pads, groups=groups)
    return {"fwd": fwd,
            "dgrad": lambda: grouped.dgrad_nhwc(dy, w, geo),
            "wgrad": lambda: grouped.wgrad_into(x, dy, geo, dw, False)}


def torch_passes(x, w, dy, geo):
    """The comparator: the public op under MDTF_KERNELS=torch and the calls autograd makes for its backward.  With
    asymmetric pads the padded input is made once outside the timed call and the padded dx is sliced (a view)."""
    import torch.nn.functional as F
    from mdtf.ops import nn as ops
    n, h, wd, c, cg = geo[:5]
    s = geo[9]
    pt, pb, pl, pr = geo[11:15]
    groups = c // cg
    xc, dyc = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    sym = pt == pb and pl == pr
    if not sym:
        xc = F.pad(xc, (pl, pr, pt, pb))
    pad = (pt, pl) if sym else (0, 0)
    wt = w.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)

    def bwd(mask):
        return torch.ops.aten.convolution_backward(dyc, xc, wt, None, (s, s), pad, (1, 1), False, (0, 0), groups, mask)

    def fwd():
        with torch.no_grad():
            return ops.conv2d(x, w, s, (pt, pb, pl, pr), groups=groups)

    def dgrad():
        dx = bwd((True, False, False))[0]
        if not sym:
            dx = dx[:, :, pt:pt + h, pl:pl + wd]
        return dx.permute(0, 2, 3, 1)
    return {"fwd": fwd, "dgrad": dgrad, "wgrad": lambda: bwd((False, True, False))[1].permute(2, 3, 1, 0)}


def measure(name, which, native, ref, nbytes, rate, args):
    a, b = native().float(), ref().float()
    worst, scale = float((a - b).abs().max()), float(b.abs().max())
    times = {"native": [], "torch": []}
    for _ in range(args.rounds):
        for key, f in (("native", native), ("torch", ref)):
            times[key].append(graph_time(f, args.iters, args.reps))
    rec = {"probe": name, "pass": which, "bytes": nbytes, "floor_us": round(nbytes / rate * 1e6, 2),
           "max_abs_diff": worst, "max_abs": scale, "iters": args.iters, "reps": args.reps, "rounds": args.rounds}
    for key, ts in times.items():
        med = sorted(t[0] for t in ts)[len(ts) // 2]
        rec[key] = {"us": round(med, 2), "us_min": round(min(t[1] for t in ts), 2),
                    "us_max": round(max(t[2] for t in ts), 2), "GBps": round(nbytes / med / 1e3, 1)}
    n, t = rec["native"], rec["torch"]
    rec["torch_over_native"] = round(t["us"] / n["us"], 2)
    rec["floor_over_native"] = round(rec["floor_us"] / n["us"], 3)
    rec["loses"] = bool(n["us"] - t["us"] > t["us_max"] - t["us_min"])
    print(json.dumps(rec), flush=True)
    return rec


def markdown(recs, rate, path):
    lines = ["Copy rate of this run: %.2f TB/s." % (rate / 1e12), "",
             "| case | pass | bytes | native us (min .. max) | GB/s | fraction of the floor | torch us (min .. max) | "
             "torch / native | floor us | loses |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        n, t = r["native"], r["torch"]
        lines.append("| %s | %s | %d | %.1f (%.1f .. %.1f) | %.0f | %.2f | %.1f (%.1f .. %.1f) | %.2f | %.1f | %s |"
                     % (r["probe"], r["pass"], r["bytes"], n["us"], n["us_min"], n["us_max"], n["GBps"],
                        r["floor_over_native"], t["us"], t["us_min"], t["us_max"], r["torch_over_native"],
                        r["floor_us"], "yes" if r["loses"] else ""))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10, help="calls per captured graph")
    p.add_argument("--reps", type=int, default=9, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    p.add_argument("--markdown", default="", help="also write the table to this file")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("conv_group_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native, grouped
    from mdtf.ops.padding import conv_geometry
    _native.lib()
    rate = copy_rate()
    print(json.dumps({"copy_TBps": round(rate / 1e12, 3)}), flush=True)
    wanted = [c for c in args.cases.split(",") if c]
    gen = torch.Generator().manual_seed(0)
    recs = []
    for name, h, wd, c, cg, s in CASES:
        if wanted and name not in wanted:
            continue
        oh, ow, pt, pb, pl, pr = conv_geometry(h, wd, 3, 3, (s, s), "SAME" if s == 1 else (1, 1))
        x = torch.randn((args.batch, h, wd, c), generator=gen).cuda().bfloat16()
        w = (torch.randn((3, 3, cg, c), generator=gen) * 0.1).cuda().bfloat16()
        dy = torch.randn((args.batch, oh, ow, c), generator=gen).cuda().bfloat16()
        geo = [args.batch, h, wd, c, cg, oh, ow, 3, 3, s, 1, pt, pb, pl, pr]
        assert grouped.native_ok(x, w, c // cg, (s, s), (1, 1), (pt, pb, pl, pr))
        native, ref = native_passes(x, w, dy, geo), torch_passes(x, w, dy, geo)
        io = 2 * (x.numel() + dy.numel())
        nbytes = {"fwd": io + 2 * w.numel(), "dgrad": io + 2 * w.numel(),
                  "wgrad": io + 4 * grouped.wgrad_workspace(geo, "cuda").numel()}
        for which in ("fwd", "dgrad", "wgrad"):
            recs.append(measure(name, which, with_mode("native", native[which]), with_mode("torch", ref[which]),
                                nbytes[which], rate, args))
        del native, ref, x, w, dy
    if args.markdown:
        markdown(recs, rate, args.markdown)


if __name__ == "__main__":
    main()
