#!/usr/bin/env python
"""Group normalization alone: the kernels of csrc/groupnorm.hip, both designs, against ``F.group_norm`` on
channels-last bf16 in the same process.

Per case (bf16 NHWC, ``--batches`` images, G groups), forward and backward each:

  56x56x256  28x28x512  14x14x1024  7x7x2048  112x112x64  (G = 32: GN-ResNet-50 / ResNeXt)     128x128x64 (G = 64:
  instance norm)

  resident   ``ops.groupnorm.forward_nhwc`` / ``backward_nhwc`` with path 1, where the strip fits LDS
  streaming  the same with path 2
  torch      ``F.group_norm`` on the channels-last view (it copies the input to NCHW first and returns NCHW), and
             ``aten.native_group_norm_backward`` as its autograd calls it: the NCHW copy of x is the saved one, dy is
             copied to NCHW inside the timed call, dx comes back NCHW (no pass back to NHWC is timed)

Each variant is captured ``--iters`` times into a hipGraph; the replay is timed with device events ``--reps`` times
(median, min, max) and the variants alternate ``--rounds`` times.  Every variant is timed against its own byte floor
at 6.3 TB/s, the rate the BatchNorm passes reach: forward resident x + y, streaming 2 x + y; backward resident
x + dy + dx, streaming 2 (x + dy) + dx; torch is rated at the resident floor.  One JSON line per case, batch and pass;
``--markdown`` also writes the table.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.image_probe import HBM_BPS, graph_time  # noqa: E402

CASES = [("56x56x256", (56, 56, 256), 32), ("28x28x512", (28, 28, 512), 32), ("14x14x1024", (14, 14, 1024), 32),
         ("7x7x2048", (7, 7, 2048), 32), ("112x112x64", (112, 112, 64), 32), ("in_128x128x64", (128, 128, 64), 64)]
EPS = 1e-6


def variants(x, dy, gamma, beta, groups):
    """{pass: {variant: (fn, tensor passes over memory)}}"""
    from mdtf.ops import groupnorm as gn
    n, h, w, c = x.shape
    _, mean, rstd = gn.forward_nhwc(x, gamma, beta, groups, EPS, False, 2)
    dg, db = torch.empty_like(gamma), torch.empty_like(beta)
    xc, dyc = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    gb, bb = gamma.bfloat16(), beta.bfloat16()
    xn = xc.contiguous()                           # what the comparator's forward saves for its backward
    _, tmean, trstd = torch.ops.aten.native_group_norm(xn, gb, bb, n, c, h * w, groups, EPS)
    fwd = {"streaming": (lambda: gn.forward_nhwc(x, gamma, beta, groups, EPS, False, 2)[0], 3),
           "torch": (lambda: F.group_norm(xc, groups, gb, bb, EPS).permute(0, 2, 3, 1), 2)}
    bwd = {"streaming": (lambda: gn.backward_nhwc(x, dy, gamma, beta, mean, rstd, groups, False, dg, db, False, 2), 5),
           "torch": (lambda: torch.ops.aten.native_group_norm_backward(
               dyc.contiguous(), xn, tmean, trstd, gb, n, c, h * w, groups, (True, True, True))[0]
               .permute(0, 2, 3, 1), 3)}
    if gn.resident_fits(h, w, c, groups, False):
        fwd["resident"] = (lambda: gn.forward_nhwc(x, gamma, beta, groups, EPS, False, 1)[0], 2)
    if gn.resident_fits(h, w, c, groups, True):
        bwd["resident"] = (lambda: gn.backward_nhwc(x, dy, gamma, beta, mean, rstd, groups, False, dg, db, False, 1),
                           3)
    return {"fwd": fwd, "bwd": bwd}


def measure(name, batch, which, vs, tensor_bytes, args):
    ref = vs["streaming"][0]().float()
    times = {k: [] for k in vs}
    rec = {"probe": name, "batch": batch, "pass": which, "tensor_bytes": tensor_bytes, "iters": args.iters,
           "reps": args.reps, "rounds": args.rounds}
    for k, (f, _) in vs.items():
        rec["max_abs_diff_" + k] = float((f().float() - ref).abs().max())
    for _ in range(args.rounds):
        for k, (f, _) in vs.items():
            times[k].append(graph_time(f, args.iters, args.reps))
    for k, ts in times.items():
        med = sorted(t[0] for t in ts)[len(ts) // 2]
        nbytes = vs[k][1] * tensor_bytes
        rec[k] = {"us": round(med, 2), "us_min": round(min(t[1] for t in ts), 2),
                  "us_max": round(max(t[2] for t in ts), 2), "floor_us": round(nbytes / HBM_BPS * 1e6, 2),
                  "TBps": round(nbytes / med / 1e6, 3)}
    print(json.dumps(rec), flush=True)
    return rec


def markdown(recs, path):
    lines = ["| case | batch | pass | resident us (min .. max) | TB/s of 1R+1W | streaming us (min .. max) | "
             "TB/s of 2R+1W | torch us (min .. max) | resident / streaming | torch / best native |",
             "|---|---|---|---|---|---|---|---|---|---|"]

    def cell(r, k):
        return "%.1f (%.1f .. %.1f)" % (r[k]["us"], r[k]["us_min"], r[k]["us_max"]) if k in r else "does not fit"
    for r in recs:
        best = min(r[k]["us"] for k in ("resident", "streaming") if k in r)
        lines.append("| %s | %d | %s | %s | %s | %s | %.2f | %s | %s | %.2f |" % (
            r["probe"], r["batch"], r["pass"], cell(r, "resident"),
            "%.2f" % r["resident"]["TBps"] if "resident" in r else "", cell(r, "streaming"), r["streaming"]["TBps"],
            cell(r, "torch"), "%.2f" % (r["resident"]["us"] / r["streaming"]["us"]) if "resident" in r else "",
            r["torch"]["us"] / best))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10, help="calls per captured graph")
    p.add_argument("--reps", type=int, default=7, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    p.add_argument("--batches", default="32,256")
    p.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    p.add_argument("--markdown", default="", help="also write the table to this file")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("groupnorm_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native
    _native.lib()
    wanted = [c for c in args.cases.split(",") if c]
    gen = torch.Generator(device="cuda").manual_seed(0)
    recs = []
    for name, (h, w, c), groups in CASES:
        if wanted and name not in wanted:
            continue
        for batch in [int(b) for b in args.batches.split(",")]:
            x = torch.randn((batch, h, w, c), generator=gen, device="cuda").bfloat16()
            dy = torch.randn((batch, h, w, c), generator=gen, device="cuda").bfloat16()
            gamma = torch.rand((c,), generator=gen, device="cuda") + 0.5
            beta = torch.randn((c,), generator=gen, device="cuda")
            vs = variants(x, dy, gamma, beta, groups)
            for which in ("fwd", "bwd"):
                recs.append(measure(name, batch, which, vs[which], 2 * x.numel(), args))
            del vs, x, dy
            torch.cuda.empty_cache()
    if args.markdown:
        markdown(recs, args.markdown)


if __name__ == "__main__":
    main()
