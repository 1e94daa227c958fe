#!/usr/bin/env python
"""Evaluation metrics alone: ``mdtf.metrics.top_k_accuracy`` (csrc/metrics.hip) against what it replaces and against
the cross-entropy forward that reads the same rows.

Default mode, per shape (the ResNet head 256 x 1000 in fp32 and bf16, the masked-LM head: the 1280 x 30522 view of
1280 x 30720 bf16 logits), in one process:

  in_top_k   ``mdtf_in_top_k`` + ``mdtf_metric_reduce`` (k = 5, into an accumulator)
  hits_only  ``mdtf_in_top_k`` alone: one launch, as xent below is
  torch     ``((x > x.gather(1, l)).sum(1) < k).float().mean()``
  xent       ``mdtf_xent_w_fwd`` on the same rows (no reduction): the yardstick, same bytes, more math

Each variant is captured ``--iters`` times into a hipGraph; the replay is timed with device events ``--reps`` times
(median, min, max) and the three alternate ``--rounds`` times.  bytes = N * K * itemsize, the logits read once.

``--eval``: steps/s of a ResNet-50 ``Eval`` at batch 256 on synthetic data, initial weights: the wall time of a run of
``--steps`` batches minus that of a run of ``--short`` batches, over the difference (model build and the first forward
cancel).  This mode uses nothing newer than the ``Eval`` operator itself.  One JSON line per record.  Needs a GPU.
"""
import argparse
import gc
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def kernels(name, n, k_classes, ld, dtype, args):
    from mdtf import metrics as M
    from mdtf.ops import losses as L
    from mdtf.ops import metrics as OM
    gen =torch.Generator().manual_seed(0)
    buf = (torch.randn(n, ld, generator=gen) * 2.0).to("cuda", dtype)
    x = buf[:, :k_classes] if ld != k_classes else buf
    labels = torch.randint(0, k_classes, (n,), generator=gen).to("cuda")
    col = labels[:, None]
    acc = M.Accumulator("cuda")
    k = args.k

    def new():
        return M.top_k_accuracy(labels, x, k, accumulator=acc)

    def hits():
        return OM.in_top_k_hits(x, labels, k)

    def old():
        return ((x > x.gather(1, col)).sum(1) < k).float().mean()

    def xent():
        return L.weighted_softmax_xent(x, labels, None, mode=L.NONE)

    agree = {"value_in_top_k": new().value(), "value_torch": float(old())}
    nbytes = n * k_classes * buf.element_size()
    rec = {"probe": name, "rows": n, "classes": k_classes, "row_stride": ld, "dtype": str(dtype).split(".")[-1],
           "k": k, "iters": args.iters, "reps": args.reps, "rounds": args.rounds, "bytes": nbytes}
    rec.update(agree)
    times = {"in_top_k": [], "hits_only": [], "torch": [], "xent": []}
    for _ in range(args.rounds):
        for key, fn in (("in_top_k", new), ("hits_only", hits), ("torch", old), ("xent", xent)):
            times[key].append(graph_time(fn, args.iters, args.reps))
    for key, ts in times.items():
        med = sorted(t[0] for t in ts)[len(ts) // 2]
        rec[key] = {"us": round(med, 2), "us_min": round(min(t[1] for t in ts), 2),
                    "us_max": round(max(t[2] for t in ts), 2), "TBps": round(nbytes / med / 1e6, 3)}
    rec["torch_over_in_top_k"] = round(rec["torch"]["us"] / rec["in_top_k"]["us"], 3)
    rec["xent_over_in_top_k"] = round(rec["xent"]["us"] / rec["in_top_k"]["us"], 3)
    print(json.dumps(rec), flush=True)
    del buf, x
    torch.cuda.empty_cache()


def eval_run(steps, batch):
    from mdtf.data.loaders import InputOptions, SyntheticDataLoader
    from mdtf.models import ResNet, SoftmaxCrossEntropyLoss
    from mdtf.runtime import Net
    from mdtf.runtime.eval import Eval
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    gc.collect()
    torch.cuda.empty_cache()
    V.get_store().generator.manual_seed(1234)
    server = types.SimpleNamespace(is_chief=True, local_rank=0, target="", worker_group=None, store=None,
                                   layout=types.SimpleNamespace(num_worker_ranks=1),
                                   device=lambda: torch.device("cuda", 0), signal_done=lambda: None)
    loader = SyntheticDataLoader(shape=(224, 224, 3), num_classes=1000, dtype=torch.bfloat16, seed=0)
    loader.batch_size = batch
    e = Eval.__new__(Eval)
    for key, val in dict(task_index=0, job_name="worker", server=server, data_loader=loader,
                         input_mode=InputOptions.SYNTHETIC, batch_size=batch, sample_number=batch * steps,
                         model_dir="", data_dir="", net=Net(ResNet(50)), loss=SoftmaxCrossEntropyLoss(),
                         eval_steps=steps).items():
        setattr(e, key, val)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = e.run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, m


def eval_mode(args):
    eval_run(args.short, args.batch)                                  # code objects, allocator
    rates, m = [], None
    for _ in range(args.rounds):
        t_short, _ = eval_run(args.short, args.batch)
        t_long, m = eval_run(args.steps, args.batch)
        rates.append((args.steps - args.short) / (t_long - t_short))
    rates.sort()
    print(json.dumps({"probe": "ResNet-50 Eval", "run": args.tag, "batch": args.batch, "steps": args.steps,
                      "short": args.short, "rounds": args.rounds, "steps_per_s": [round(r, 2) for r in rates],
                      "steps_per_s_median": round(rates[len(rates) // 2], 2),
                      "metrics": {k: v for k, v in m.items()}}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20, help="calls per captured graph")
    p.add_argument("--reps", type=int, default=9, help="timed replays per measurement")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the variants")
    p.add_argument("--k", type=int, default=5)
    p.add_argument("--eval", action="store_true", help="time a ResNet-50 Eval instead of the kernels")
    p.add_argument("--steps", type=int, default=24)
    p.add_argument("--short", type=int, default=4)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--tag", default="this commit")
    args = p.parse_args()
    sys.argv = sys.argv[:1]                        # mdtf's own flags parse the command line on first use
    if not torch.cuda.is_available():
        raise SystemExit("metrics_probe needs a GPU")
    torch.cuda.set_device(0)
    from mdtf.ops import _native
    _native.lib()
    if args.eval:
        return eval_mode(args)
    kernels("ResNet head fp32", 256, 1000, 1000, torch.float32, args)
    kernels("ResNet head bf16", 256, 1000, 1000, torch.bfloat16, args)
    kernels("masked-LM head bf16", 1280, 30522, 30720, torch.bfloat16, args)


if __name__ == "__main__":
    main()
