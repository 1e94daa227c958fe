#!/usr/bin/env python
"""Device-event timings of the layer-wise optimizer kernels (csrc/layerwise.hip) over the real layer maps of
BERT-base and ResNet-50, built from the models' variable lists.

Warm: back-to-back launches over the same buffers.  Cold: each launch behind a fill of a buffer larger than the
last-level cache, as a step's update follows a whole backward.  Bytes per call come from the element counts:
lamb_moments 6 fp32 streams (g, m, v, w in; m, v out), lamb_apply 4 + the bf16 shadow, lars_norms 2, lars_apply 5 +
the shadow.  One JSON line per model.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_targets(model, kind):
    import mdtf
    from mdtf.runtime import Net, Tower
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device = torch.device("cuda", 0)
    store.compute_dtype = torch.bfloat16
    if model == "bert":
        from mdtf.models import Bert, BertPretrainingLoss, SyntheticBertLoader
        ld = SyntheticBertLoader(128, 20, seed=0)
        ld.batch_size = 2
        raw, gt = ld.load_train_batch()
        net, loss = Bert("base", seq_len=128, max_predictions=20), BertPretrainingLoss(20)
    else:
        from mdtf.data.loaders import SyntheticDataLoader
        from mdtf.models import ResNet, SoftmaxCrossEntropyLoss
        ld = SyntheticDataLoader(shape=(64, 64, 3), num_classes=1000, dtype=torch.bfloat16)
        ld.batch_size = 2
        raw, gt = ld.load_train_batch()
        net, loss = ResNet(50), SoftmaxCrossEntropyLoss()
    opt = (mdtf.train.LAMBOptimizer(1e-4, weight_decay_rate=0.01) if kind == "lamb"
           else mdtf.train.LARSOptimizer(0.1, weight_decay=5e-5))
    tg = []
    Tower(Net(net), "tower_0/", tg, raw, gt, loss, opt, batch_size=2).process()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    op.finalize()
    return op, opt


def timed(fn, reps, flush=None):
    out = []
    for _ in range(reps):
        if flush is not None:
            flush.fill_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--flush_mb", type=int, default=1024)
    args = p.parse_args()
    from mdtf.ops import layerwise as LW
    flush = torch.empty(args.flush_mb << 18, dtype=torch.float32, device="cuda")
    for model, kind in (("bert", "lamb"), ("resnet", "lars")):
        op, opt = build_targets(model, kind)
        targets = op.reducer.update_targets()
        for t in targets:
            t.grad.normal_(0, 1e-3)
        lmap, buf = LW.state_for(targets, op.reducer)
        n = sum(x for it in lmap.items for _, x, _ in it)
        T = range(len(targets))
        if kind == "lamb":
            st = [(t.master, t.grad, t.state("m"), t.state("v"), t.shadow) for t in targets]
            kernels = {
                "lamb_moments": (lambda: [LW.lamb_moments_(lmap, buf, i, st[i][0], st[i][1], st[i][2], st[i][3], 0.9,
                                                           0.999, 1e-6, 1.0, 0.01) for i in T], 24 * n),
                "layer_finalize": (lambda: LW.layer_finalize_(lmap, buf, LW.LAMB), 8 * lmap.num_items),
                "lamb_apply": (lambda: [LW.lamb_apply_(lmap, buf, i, st[i][0], st[i][2], st[i][3], st[i][4], 1e-4,
                                                       1e-6, 0.01) for i in T], 18 * n),
            }
        else:
            st = [(t.master, t.grad, t.state("momentum"), t.shadow) for t in targets]
            kernels = {
                "lars_norms": (lambda: [LW.lars_norms_(lmap, buf, i, st[i][0], st[i][1]) for i in T], 8 * n),
                "layer_finalize": (lambda: LW.layer_finalize_(lmap, buf, LW.LARS, 1e-3, 5e-5, 0.0, 1.0),
                                   8 * lmap.num_items),
                "lars_apply": (lambda: [LW.lars_apply_(lmap, buf, i, st[i][0], st[i][1], st[i][2], st[i][3], 0.1, 0.9,
                                                       1.0, 5e-5) for i in T], 22 * n),
            }
        rec = {"model": model, "optimizer": kind, "elements": n, "layers": lmap.num_layers, "items": lmap.num_items,
               "targets": len(targets), "kernels": {}}
        for name, (fn, nbytes) in kernels.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            warm, warm_min = timed(fn, args.reps)
            cold, cold_min = timed(fn, args.reps, flush)
            rec["kernels"][name] = {"bytes": nbytes, "warm_us": round(warm, 1), "warm_min_us": round(warm_min, 1),
                                    "cold_us": round(cold, 1), "cold_min_us": round(cold_min, 1),
                                    "warm_TBps": round(nbytes / warm / 1e6, 3),
                                    "cold_TBps": round(nbytes / cold / 1e6, 3)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
