#!/usr/bin/env python
"""Encoder-decoder attention (csrc/attention_cross.hip) against the unfused path and PyTorch's fused attention.

For each shape (B, Sq, Sk, heads, head dim), once with full lengths and once with seeded lengths uniform in
[Sk / 4, Sk], the forward and the forward + backward are timed with dropout 0.1:

  cross     ops.transformer.cross_attention(q, kv, ..., kv_lengths=device int32)   the length-aware kernels
  unfused   ops.transformer.attention(q, k, v, mask)         two batched GEMMs around the masked softmax kernel,
                                                             lengths as an additive -10000 key mask
  sdpa      torch.nn.functional.scaled_dot_product_attention with a boolean [B, 1, 1, Sk] key mask
  cross_q64 / cross_q128   (forward only) mdtf_attn_fwd_cross_qb: 64 or 128 queries per forward block

The comparators get q, k, v already in their [B, heads, S, d] layout.  One call is captured ``--iters`` times into a
hipGraph; the replay is timed with device events ``--reps`` times (median).  The candidates alternate ``--rounds``
times in one process after one discarded warm-up round; ``*_spread_us`` is max - min over the rounds.
``visible_tiles`` is the share of 64-key tiles that hold a visible key, sum_b ceil(len_b / 64) / (B * Sk / 64).
One JSON line per shape, length mode and direction.  Needs a GPU.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.attn_causal_probe import graph_time  # noqa: E402

#          B  Sq   Sk   nh  dh
SHAPES = [(64, 64, 64, 8, 64), (64, 64, 256, 8, 64), (64, 128, 512, 8, 64), (64, 128, 512, 16, 128)]
P_DROP = 0.1


def probe(B, Sq, Sk, nh, dh, ragged, args):
    from mdtf.ops import _native as N
    from mdtf.ops import transformer as T
    from mdtf.train.graph import rng_offset_tensor
    H = nh * dh
    gen = torch.Generator().manual_seed(Sq + Sk + dh)
    q = (torch.randn(B * Sq, H, generator=gen) * 0.5).to("cuda", torch.bfloat16).requires_grad_(True)
    kv = (torch.randn(B * Sk, 2 * H, generator=gen) * 0.5).to("cuda", torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B * Sq, H, generator=gen).to("cuda", torch.bfloat16)
    n = torch.randint(Sk // 4, Sk + 1, (B,), generator=gen) if ragged else torch.full((B,), Sk)
    lens = n.to("cuda", torch.int32)
    visible = float(((n + 63) // 64).sum()) / (B * Sk // 64)
    hidden = (torch.arange(Sk)[None, :] >= n[:, None]).cuda()
    add_mask = hidden.float() * -10000.0
    keep_mask = ~hidden[:, None, None, :]
    # the comparators' operands in their own layout
    qh = q.detach().view(B, Sq, nh, dh).transpose(1, 2).contiguous().requires_grad_(True)
    kh, vh = (t.transpose(1, 2).contiguous().requires_grad_(True)
              for t in kv.detach().view(B, Sk, 2, nh, dh).unbind(2))
    dh_out = dout.view(B, Sq, nh, dh).transpose(1, 2).contiguous()
    out = torch.empty_like(dout)
    lse = torch.empty(B * nh, Sq, dtype=torch.float32, device="cuda")
    off = rng_offset_tensor(q.device)
    scale = 1.0 / math.sqrt(dh)

    def cross():
        return T.cross_attention(q, kv, B, Sq, Sk, nh, None, lens, P_DROP), (q, kv), dout

    def unfused():
        return T.attention(qh, kh, vh, add_mask, P_DROP), (qh, kh, vh), dh_out

    def sdpa():
        return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=keep_mask, dropout_p=P_DROP), (qh, kh, vh), dh_out

    def forward(make):
        def run():
            with torch.no_grad():
                make()
        return run

    def both(make):
        def run():
            o, leaves, g = make()
            torch.autograd.grad(o, leaves, g)
        return run

    def fixed_block(qb):
        def run():
            N.check(N.fn("mdtf_attn_fwd_cross_qb")(N.ptr(q), N.ptr(kv), None, N.ptr(lens), N.ptr(out), N.ptr(lse), B, Sq,
                                                   Sk, nh, dh, scale, P_DROP, 4321, N.ptr(off), qb, N.stream_ptr()),
                    "attn_fwd_cross_qb")
        return run

    makers = [("cross", cross), ("unfused", unfused), ("sdpa", sdpa)]
    plans = [("fwd", [(k, forward(m)) for k, m in makers] + [("cross_q64", fixed_block(64)),
                                                            ("cross_q128", fixed_block(128))]),
             ("fwd_bwd", [(k, both(m)) for k, m in makers])]
    for direction, candidates in plans:
        times = {name: [] for name, _ in candidates}
        for rnd in range(args.rounds + 1):                # round 0 warms the shape up and is discarded
            for name, fn in candidates:
                t = graph_time(fn, args.iters, args.reps)
                if rnd:
                    times[name].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        rec = {"probe": "attn_cross", "dir": direction, "B": B, "Sq": Sq, "Sk": Sk, "heads": nh, "dh": dh,
               "lengths": "ragged" if ragged else "full", "visible_tiles": round(visible, 3), "iters": args.iters,
               "reps": args.reps, "rounds": args.rounds}
        for k, v in times.items():
            rec[k + "_us"] = round(med[k], 2)
            rec[k + "_spread_us"] = round(max(v) - min(v), 2)
        rec["unfused_over_cross"] = round(med["unfused"] / med["cross"], 3)
        rec["sdpa_over_cross"] = round(med["sdpa"] / med["cross"], 3)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="calls per captured graph")
    ap.add_argument("--reps", type=int, default=20, help="timed replays per measurement")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the candidates")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_cross_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native as N
    N.lib()
    # the block-size-taking entry point exists for this A/B only; the package does not register it
    N.register("mdtf_attn_fwd_cross_qb", [N.P] * 6 + [N.I] * 5 + [N.F, N.F, N.U, N.P, N.I, N.P])
    for shape in SHAPES:
        for ragged in (False, True):
            probe(*shape, ragged, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
