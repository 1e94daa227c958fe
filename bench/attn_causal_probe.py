#!/usr/bin/env python
"""Causal attention (csrc/attention_causal.hip) against the non-causal tiled kernels (csrc/attention_flash.hip).

For each shape (B, S, heads, head dim) the forward entry point and the backward entry point (Dq + dK/dV + dQ) are
timed on their own, on preallocated buffers, with dropout 0.1 and a key mask:

  full            mdtf_attn_{fwd,bwd}_flash              every key tile of every query block
  causal          mdtf_attn_{fwd,bwd}_causal             tiles above the diagonal skipped, heaviest block first
  causal_natural  mdtf_attn_{fwd,bwd}_causal_order(..., 1): blockIdx.y in natural order (forward and dQ; dK/dV's
                  natural order is already heaviest-first)

One call is captured ``--iters`` times into a hipGraph; the replay is timed with device events ``--reps`` times
(median).  The three variants alternate ``--rounds`` times in one process after one discarded warm-up round, so each
ratio stands beside the non-causal kernel's own round-to-round spread (max - min over the rounds).  ``tile_ratio`` is
the share of (128-query block, 64-key tile) pairs the causal forward visits: sum_y min(nkt, 2(y+1)) / (nblk * nkt).
One JSON line per shape and direction.  Needs a GPU.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 128, 12, 64), (16, 512, 12, 64), (4, 2048, 12, 64), (8, 512, 16, 128)]


def graph_time(fn, iters, reps):
    """us per call of ``fn`` from ``reps`` timed replays of a graph of ``iters`` calls (median)."""
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
    return out[len(out) // 2]


def tile_ratio(S):
    nblk, nkt = (S + 127) // 128, S // 64
    return sum(min(nkt, 2 * (y + 1)) for y in range(nblk)) / float(nblk * nkt)


def probe(B, S, nh, dh, args):
    from mdtf.ops import _native as N
    from mdtf.ops import transformer  # noqa: F401  (registers the attention entry points)
    from mdtf.train.graph import rng_offset_tensor
    H = nh * dh
    gen = torch.Generator().manual_seed(S + dh)
    qkv = (torch.randn(B * S, 3 * H, generator=gen) * 0.5).to("cuda", torch.bfloat16)
    dout = torch.randn(B * S, H, generator=gen).to("cuda", torch.bfloat16)
    mask = ((torch.rand(B, S, generator=gen) < 0.15).float() * -10000.0).cuda()
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
    lse = torch.empty(B * nh, S, dtype=torch.float32, device="cuda")
    ws = torch.empty(B * nh * S, dtype=torch.float32, device="cuda")
    off = rng_offset_tensor(qkv.device)
    scale, p, seed = 1.0 / math.sqrt(dh), 0.1, 4321

    def fwd(kind, order=()):
        def run():
            N.check(N.fn("mdtf_attn_fwd_" + kind)(N.ptr(qkv), N.ptr(mask), N.ptr(out), N.ptr(lse), B, S, nh, dh, scale,
                                                  p, seed, N.ptr(off), *order, N.stream_ptr()), "attn_fwd_" + kind)
        return run

    def bwd(kind, order=()):
        def run():
            N.check(N.fn("mdtf_attn_bwd_" + kind)(N.ptr(qkv), N.ptr(mask), N.ptr(out), N.ptr(dout), N.ptr(lse),
                                                  N.ptr(dqkv), N.ptr(ws), B, S, nh, dh, scale, p, seed, N.ptr(off),
                                                  *order, N.stream_ptr()), "attn_bwd_" + kind)
        return run

    variants = [("full", "flash", ()), ("causal", "causal", ()), ("causal_natural", "causal_order", (1,))]
    for direction, make in (("fwd", fwd), ("bwd", bwd)):
        times = {name: [] for name, _, _ in variants}
        for rnd in range(args.rounds + 1):                # round 0 warms the shape up and is discarded
            for name, kind, order in variants:
                if direction == "bwd":
                    fwd(kind, order)()               # out / lse of the variant whose backward is timed
                t = graph_time(make(kind, order), args.iters, args.reps)
                if rnd:
                    times[name].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        full = times["full"]
        rec = {"probe": "attn_causal", "dir": direction, "B": B, "S": S, "heads": nh, "dh": dh, "iters": args.iters,
               "reps": args.reps, "rounds": args.rounds, "tile_ratio": round(tile_ratio(S), 3)}
        for k, v in times.items():
            rec[k + "_us"] = [round(t, 2) for t in v]
            rec[k + "_us_median"] = round(med[k], 2)
        rec["full_spread_us"] = round(max(full) - min(full), 2)
        rec["margin_us"] = round(med["full"] - med["causal"], 2)
        rec["causal_over_full"] = round(med["causal"] / med["full"], 3)
        rec["natural_over_heaviest_first"] = round(med["causal_natural"] / med["causal"], 3)
        # the condition of S >= 512: faster than the non-causal kernel by more than that kernel's own spread
        rec["causal_faster_beyond_spread"] = bool(med["full"] - med["causal"] > max(full) - min(full))
        print(json.dumps(rec), flush=True)
    del qkv, dout, out, dqkv, lse, ws
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="calls per captured graph")
    ap.add_argument("--reps", type=int, default=40, help="timed replays per measurement")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the three variants")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_causal_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native as N
    N.lib()
    # the order-taking entry points exist for this A/B only; the package does not register them
    N.register("mdtf_attn_fwd_causal_order", [N.P, N.P, N.P, N.P, N.I, N.I, N.I, N.I, N.F, N.F, N.U, N.P, N.I, N.P])
    N.register("mdtf_attn_bwd_causal_order", [N.P, N.P, N.P, N.P, N.P, N.P, N.P, N.I, N.I, N.I, N.I, N.F, N.F, N.U, N.P,
                                              N.I, N.P])
    for shape in SHAPES:
        probe(*shape, args)


if __name__ == "__main__":
    main()
