#!/usr/bin/env python
"""Forward + backward of the classification loss alone: mdtf.losses (csrc/losses.hip) against what it replaces.

A  smoothed (eps = 0.1) mean cross entropy: ``mdtf.losses.sparse_softmax_cross_entropy`` against the PyTorch
   expression ``SoftmaxCrossEntropyLoss(0.1)`` ran before (log_softmax on an fp32 copy, a dense fp32 one-hot target,
   multiply, sum, mean), at the ResNet head (256 x 1000 bf16) and the masked-LM head (the 1280 x 30522 view of
   1280 x 30720 bf16 logits).
B  unsmoothed, unweighted mean at the masked-LM head: the new kernels (SUM_OVER_BATCH_SIZE) against
   ``mdtf_xent_fwd`` / ``mdtf_xent_bwd`` plus ``.mean()``, the default path of the benchmarks.

Every variant is one forward and one ``autograd.grad`` to the logits, captured ``--iters`` times into a hipGraph; the
replay is timed with device events ``--reps`` times (median).  Old and new alternate ``--rounds`` times in one
process, so each ratio stands beside the old variant's own round-to-round spread.  One JSON line per comparison.
Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    with torch.cuda.graph(g, capture_error_mode="thread_local"):      # as mdtf.train.graph captures a step
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


def old_smoothed(logits, labels, eps):
    n = logits.shape[-1]
    logp = torch.log_softmax(logits.float(), -1)
    onehot = torch.nn.functional.one_hot(labels.long(), n).float()
    target = onehot * (1 - eps) + eps / n
    return -(target * logp).sum(-1).mean()


def compare(name, n, k, ld, eps, args):
    from mdtf import losses as L
    from mdtf.ops import nn as ops
    gen = torch.Generator().manual_seed(0)
    buf = (torch.randn(n, ld, generator=gen) * 2.0).to("cuda", torch.bfloat16).requires_grad_(True)
    labels = torch.randint(0, k, (n,), generator=gen).to("cuda")

    def view():
        # made inside every call: the gradient is taken at this view (what the tied decoder's backward receives), and
        # a view made once outside would be an autograd node of the default stream, which backward inside a capture
        # then makes wait for the capture stream: a stream forked into the capture that never joins it again
        return buf[:, :k] if ld != k else buf

    def new():
        logits = view()
        loss = L.sparse_softmax_cross_entropy(labels, logits, reduction=L.Reduction.SUM_OVER_BATCH_SIZE,
                                              label_smoothing=eps)
        return loss, torch.autograd.grad(loss, logits)[0]

    def old():
        logits = view()
        if eps:
            loss = old_smoothed(logits, labels, eps)
        else:
            loss = ops.sparse_softmax_cross_entropy_with_logits(labels, logits).mean()
        return loss, torch.autograd.grad(loss, logits)[0]

    (lo, go), (ln, gn) = old(), new()
    agree = {"loss_old": float(lo.detach()), "loss_new": float(ln.detach()),
             "grad_max_abs_diff": float((go.float() - gn.float()).abs().max()), "grad_max_abs": float(go.abs().max())}
    del lo, go, ln, gn
    t_old, t_new = [], []
    for _ in range(args.rounds):
        t_old.append(graph_time(old, args.iters, args.reps))
        t_new.append(graph_time(new, args.iters, args.reps))
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    rec = {"probe": name, "rows": n, "classes": k, "row_stride": ld, "eps": eps, "iters": args.iters,
           "reps": args.reps, "old_us": [round(t, 2) for t in t_old], "new_us": [round(t, 2) for t in t_new],
           "old_us_median": round(med(t_old), 2), "new_us_median": round(med(t_new), 2),
           "old_spread_pct": round(100.0 * (max(t_old) - min(t_old)) / med(t_old), 2),
           "old_over_new": round(med(t_old) / med(t_new), 3)}
    rec.update(agree)
    print(json.dumps(rec), flush=True)
    del buf
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20, help="forward + backward pairs per captured graph")
    p.add_argument("--reps", type=int, default=9, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=5, help="old / new alternations")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native
    _native.lib()
    compare("A smoothed, ResNet head", 256, 1000, 1000, 0.1, args)
    compare("A smoothed, masked-LM head", 1280, 30522, 30720, 0.1, args)
    compare("B unsmoothed mean, masked-LM head", 1280, 30522, 30720, 0.0, args)


if __name__ == "__main__":
    main()
