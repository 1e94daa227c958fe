#!/usr/bin/env python
"""What the weights' moving average (mdtf.train.ExponentialMovingAverage, csrc/ema.hip) costs.

Kernels.  At the ResNet-50 (25.6 M) and BERT-base (110 M) parameter counts, ``mdtf_ema_update`` and
``mdtf_fused_momentum`` run over equally sized buffers in the same process.  Each is captured ``--iters`` times
into a hipGraph and the replay timed with device events, ``--reps`` times: us per launch and bytes/s (ema 12 B per
parameter: ema in and out, w in; momentum 22 B: w and acc in and out, g in, the bf16 shadow out), median and the
min-max spread of the repeats.  ``pair`` is a momentum launch followed by an ema launch over the weights it just
wrote, as in a training step; ``ema_after_momentum_us`` = pair - momentum.  The whole set is measured twice (runs
``a`` and ``a2``), so every figure stands beside this run's own repeat-to-repeat spread.

Steps.  ``--model resnet|bert`` times the benchmark step (bench.py's ResNet-50 at batch 256, bench/bert_bench.py's
BERT-base at batch 64 x seq 128; hipGraph replay) with the average off and on, alternating, ``--rounds`` times.

One JSON line per measurement.  Needs a GPU.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"resnet50": 25600000, "bert_base": 110000000}
EMA_BYTES, MOMENTUM_BYTES = 12, 22


def graph_time(fn, iters, reps):
    """us per call of ``fn`` from ``reps`` timed replays of a graph of ``iters`` calls: (median, min, max)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
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
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def kernels(args, tag):
    from mdtf.ops import _native
    from mdtf.ops import ema as E
    from mdtf.ops import optim as O
    _native.lib()
    for name, n in SIZES.items():
        w = torch.randn(n, device="cuda")
        g = torch.randn(n, device="cuda") * 1e-3
        acc = torch.zeros(n, device="cuda")
        e = w.clone()
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        omd = torch.tensor([1e-4], device="cuda")

        def ema():
            E.ema_update_(e, w, 1e-4, omd_dev=omd)

        def mom():
            O.momentum_(w, g, acc, sh, 1e-4, 0.9, 1.0, 5e-5)

        def pair():
            mom()
            ema()

        rec = {"probe": "kernels", "run": tag, "model": name, "elements": n, "iters": args.iters, "reps": args.reps}
        for key, fn, nbytes in (("ema", ema, EMA_BYTES * n), ("momentum", mom, MOMENTUM_BYTES * n),
                                ("pair", pair, (EMA_BYTES + MOMENTUM_BYTES) * n)):
            med, lo, hi = graph_time(fn, args.iters, args.reps)
            rec[key] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "bytes": nbytes,
                        "TBps": round(nbytes / med / 1e6, 3), "TBps_min": round(nbytes / hi / 1e6, 3),
                        "TBps_max": round(nbytes / lo / 1e6, 3)}
        rec["ema_after_momentum_us"] = round(rec["pair"]["us"] - rec["momentum"]["us"], 2)
        print(json.dumps(rec), flush=True)
        del w, g, acc, e, sh
        torch.cuda.empty_cache()


def build_step(model, average):
    import mdtf
    from mdtf.runtime import Net, Tower
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    gc.collect()
    torch.cuda.empty_cache()
    store = V.get_store()
    store.device = torch.device("cuda", 0)
    store.compute_dtype = torch.bfloat16
    store.generator.manual_seed(1234)
    if model == "bert":
        from mdtf.models import Bert, BertPretrainingLoss, SyntheticBertLoader
        batch = 64
        ld = SyntheticBertLoader(128, 20, seed=0)
        ld.batch_size = batch
        raw, gt = ld.load_train_batch()
        net, loss = Bert("base", seq_len=128, max_predictions=20), BertPretrainingLoss(20)
        base = mdtf.train.AdamWeightDecayOptimizer(1e-4, weight_decay_rate=0.01)
    else:
        from mdtf.data.loaders import SyntheticDataLoader
        from mdtf.models import ResNet, SoftmaxCrossEntropyLoss
        batch = 256
        ld = SyntheticDataLoader(shape=(224, 224, 3), num_classes=1000, dtype=torch.bfloat16, seed=0)
        ld.batch_size = batch
        raw, gt = ld.load_train_batch()
        net, loss = ResNet(50), SoftmaxCrossEntropyLoss()
        base = mdtf.train.MomentumOptimizer(0.1, momentum=0.9, weight_decay=5e-5)
    tg = []
    Tower(Net(net), "tower_0/", tg, raw, gt, loss, base, batch_size=batch).process()
    opt = mdtf.train.SyncReplicasOptimizer(base, 1, 1, hip_graph=True)
    gs = mdtf.train.get_or_create_global_step()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=gs)
    if average:
        mdtf.train.ExponentialMovingAverage(0.9999, num_updates=gs).apply(train_op=op)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    return sess, op, batch


def steps(args):
    for rnd in range(args.rounds):
        for average in (False, True):
            sess, op, batch = build_step(args.model, average)
            for _ in range(args.warmup):
                sess.run(op)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    sess.run(op)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0) / args.steps)
            times.sort()
            print(json.dumps({"probe": "step", "model": args.model, "round": rnd, "average": average, "batch": batch,
                              "elements": op.space.numel(), "replays": op.graph.replays if op.graph else 0,
                              "ms_per_step": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4),
                              "ms_max": round(times[-1], 4), "steps": args.steps, "reps": args.reps}), flush=True)
            sess.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20, help="launches per captured graph")
    p.add_argument("--reps", type=int, default=7, help="timed repeats of every measurement")
    p.add_argument("--model", default="none", choices=["none", "resnet", "bert"], help="also time this model's step")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=6)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--kernels", type=int, default=1)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_probe needs a GPU")
    torch.cuda.set_device(0)
    if args.kernels:
        kernels(args, "a")
        kernels(args, "a2")
    if args.model != "none":
        steps(args)


if __name__ == "__main__":
    main()
