#!/usr/bin/env python
"""Input preprocessing alone: ``mdtf.image`` (csrc/image.hip) against the PyTorch expression of the same calls.

Per case, in one process:

  imagenet_train  ``imagenet_preprocess(is_training=True)``   256 x (256, 256, 3) uint8 -> 224 x 224 bf16
  imagenet_eval   ``imagenet_preprocess(is_training=False)``  the same shapes (the central 224 box: the copy path)
  transform_only  ``transform`` over fixed distorted boxes and flips: the fused pass without the parameter launch
  cifar_train     ``cifar_preprocess(is_training=True)``      1024 x (32, 32, 3) uint8 -> fp32
  crop            ``random_crop`` to 224 x 224, uint8 out: the plain copy path

  native   the HIP kernels
  torch    the same call under ``MDTF_KERNELS=torch`` (the reference branch of ``mdtf.ops.image``: index tensors, gathers,
           lerps, normalize, cast; for device-drawn boxes it computes the copy and the resize branch and selects)

Each variant is captured ``--iters`` times into a hipGraph; the replay is timed with device events ``--reps`` times
(median, min, max) and the variants alternate ``--rounds`` times.  The step counter does not move between replays, so
every replay draws the same boxes.  bytes = the box bytes of the source (each once) + the output bytes;
``floor_us`` is that over 6.3 TB/s, the rate the BatchNorm passes reach.  One JSON line per case; ``--markdown`` also
writes the table.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.3e12


def graph_time(fn, iters, reps):
    """(median, min, max) us per call of ``fn`` from ``reps`` timed replays of a graph of ``iters`` calls."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    del g
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def with_mode(mode, fn):
    def run():
        prev = os.environ.get("MDTF_KERNELS")
        os.environ["MDTF_KERNELS"] = mode
        try:
            return fn()
        finally:
            if prev is None:
                del os.environ["MDTF_KERNELS"]
            else:
                os.environ["MDTF_KERNELS"] = prev
    return run


def case(name, fn, nbytes, args, check):
    native, ref = with_mode("native", fn), with_mode("torch", fn)
    a, b = native().float(), ref().float()
    worst = float((a - b).abs().max())
    if check is not None:
        assert worst <= check, "%s: native and torch differ by %g" % (name, worst)
    times = {"native": [], "torch": []}
    for _ in range(args.rounds):
        for key, f in (("native", native), ("torch", ref)):
            times[key].append(graph_time(f, args.iters if key == "native" else max(args.iters // 4, 1), args.reps))
    rec = {"probe": name, "bytes": nbytes, "floor_us": round(nbytes / HBM_BPS * 1e6, 2), "max_abs_diff": worst,
           "iters": args.iters, "reps": args.reps, "rounds": args.rounds}
    for key, ts in times.items():
        med = sorted(t[0] for t in ts)[len(ts) // 2]
        rec[key] = {"us": round(med, 2), "us_min": round(min(t[1] for t in ts), 2),
                    "us_max": round(max(t[2] for t in ts), 2), "TBps": round(nbytes / med / 1e6, 3)}
    rec["torch_over_native"] = round(rec["torch"]["us"] / rec["native"]["us"], 2)
    rec["native_over_floor"] = round(rec["native"]["us"] / rec["floor_us"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def markdown(recs, path):
    lines = ["| case | bytes | native us (min .. max) | TB/s | torch us | torch / native | floor us at 6.3 TB/s | "
             "native / floor |", "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        n, t = r["native"], r["torch"]
        lines.append("| %s | %d | %.1f (%.1f .. %.1f) | %.2f | %.1f | %.1f | %.1f | %.1f |"
                     % (r["probe"], r["bytes"], n["us"], n["us_min"], n["us_max"], n["TBps"], t["us"],
                        r["torch_over_native"], r["floor_us"], r["native_over_floor"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20, help="calls per captured graph")
    p.add_argument("--reps", type=int, default=9, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--cifar_batch", type=int, default=1024)
    p.add_argument("--markdown", default="", help="also write the table to this file")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("image_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf import image as I
    from mdtf.ops import _native
    _native.lib()
    B, S, O, C = args.batch, 256, 224, 3
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (B, S, S, C), generator=g, dtype=torch.uint8).cuda()
    small = torch.randint(0, 256, (args.cifar_batch, 32, 32, C), generator=g, dtype=torch.uint8).cuda()
    boxes = I.distorted_boxes(B, (S, S), seed=7, device=x.device)
    flips = I.random_flips(B, seed=7, device=x.device)
    box_bytes = int((boxes[:, 2].long() * boxes[:, 3].long()).sum()) * C
    out_bf16 = B * O * O * C * 2
    mean = (123.68, 116.78, 103.94)
    bf, recs = torch.bfloat16, []
    # bf16 outputs of magnitude < 256 round by up to 0.5; the two branches may also differ in the last fp32 bit of a lerp
    recs.append(case("imagenet_train", lambda: I.imagenet_preprocess(x, True, O, O, dtype=bf, seed=7),
                     box_bytes + out_bf16, args, None))   # (a box may round differently: reported, not asserted)
    recs.append(case("imagenet_eval", lambda: I.imagenet_preprocess(x, False, O, O, dtype=bf),
                     B * O * O * C + out_bf16, args, 0.0))
    recs.append(case("transform_only", lambda: I.transform(x, (O, O), boxes=boxes, flips=flips, mean=mean, dtype=bf),
                     box_bytes + out_bf16, args, 1.01))
    n = small.numel()
    recs.append(case("cifar_train", lambda: I.cifar_preprocess(small, True, dtype=torch.float32, seed=7),
                     n + 4 * n, args, 1e-5))
    recs.append(case("crop", lambda: I.random_crop(x, (O, O), seed=7), 2 * B * O * O * C, args, 0.0))
    if args.markdown:
        markdown(recs, args.markdown)


if __name__ == "__main__":
    main()
