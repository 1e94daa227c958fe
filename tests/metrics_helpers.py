"""Case builders and oracles of ``tests/test_metrics.py``; the worker body of its two-rank gloo test."""
import json
import math
import os
import types

import torch

NAN, INF = float("nan"), float("inf")
TARGET, ABOVE = 1.0, 2.0


# ------------------------------------------------------------------------------------------------------ in_top_k
def oracle_hits(x, labels, weights, k):
    """The definition, row by row, on the CPU: an integer count of ``x > t`` over ``[0, K)`` in fp64, 1 iff the label
    is in range, the target finite and the count below k; 0 for a skipped row."""
    n, kk = x.shape
    out = torch.zeros(n)
    for r in range(n):
        lab = int(labels[r])
        if weights is not None and float(weights[r]) == 0.0:
            continue
        if not 0 <= lab < kk:
            continue
        row = x[r].double()
        t = float(row[lab])
        if not math.isfinite(t):
            continue
        out[r] = 1.0 if int((row > t).sum()) < k else 0.0
    return out


def _row(kk, gen, lab, greater=0, equal=0, target=TARGET, pinned=(), extra=()):
    """One row of K logits: the target value at ``lab``, ``greater`` columns above it (``pinned`` columns first),
    ``equal`` columns tied with it, the values of ``extra`` in further columns, everything else below the target.
    All values are multiples of 1/8 of small magnitude, exact in bf16.  Counts are cut to the columns there are."""
    row = -(torch.randint(1, 65, (kk,), generator=gen).float() / 8.0)
    free = [c for c in torch.randperm(kk, generator=gen).tolist() if c != lab and c not in pinned]
    cols = [c for c in pinned if c != lab] + free
    greater = min(greater, len(cols))
    for i, c in enumerate(cols[:greater]):
        row[c] = ABOVE + (i % 8) / 8.0
    cols = cols[greater:]
    equal = min(equal, len(cols))
    for c in cols[:equal]:
        row[c] = target
    cols = cols[equal:]
    for c, v in zip(cols, extra):
        row[c] = v
    row[lab] = target
    return row


def scenario_rows(kk, k, gen):
    """(rows [R, K], labels [R], weights [R]) holding every situation the definition names; see test_metrics.py."""
    rows, labels, weights = [], [], []

    def add(row, lab, w=1.0):
        rows.append(row)
        labels.append(lab)
        weights.append(w)

    mid = kk // 2
    add(_row(kk, gen, mid, greater=k - 1, equal=3), mid, 2.5)              # ties straddle the boundary: a hit
    add(_row(kk, gen, mid, greater=k), mid)                                # k strictly greater: a miss
    add(_row(kk, gen, mid, greater=k - 1), mid, 0.5)                       # k - 1: a hit
    for t in (NAN, INF, -INF):                                             # the target itself is not finite
        add(_row(kk, gen, min(3, kk - 1), greater=0, target=t), min(3, kk - 1))
    add(_row(kk, gen, mid, greater=max(k - 2, 0), extra=(INF, NAN, -INF, NAN)), mid)   # +inf counts, NaN / -inf do not
    add(_row(kk, gen, mid, greater=max(k - 1, 0), extra=(NAN, -INF)), mid)
    add(torch.full((kk,), NAN), -1)                                        # labels outside [0, K): never read
    add(torch.full((kk,), NAN), kk)
    add(torch.full((kk,), NAN), mid, 0.0)                                  # weight 0: never read
    add(_row(kk, gen, mid, greater=k, pinned=(kk - 1,)), mid)              # the greatest in the last valid column
    add(_row(kk, gen, mid, greater=k, pinned=(0,)), mid)                   # ... and in column 0
    add(_row(kk, gen, kk - 1, greater=k - 1, equal=1), kk - 1)             # the target in the last valid column
    add(_row(kk, gen, 0, greater=k, pinned=(kk - 1,)), 0)                  # ... and in column 0
    return torch.stack(rows), torch.tensor(labels), torch.tensor(weights)


def launches(rows, labels, weights, n, ld, offset, dtype, device):
    """The scenario rows in launches of ``n`` rows (the last one filled up with the first rows again): each a
    ``[n, K]`` view, rows ``ld`` apart and ``offset`` elements into its buffer, pad columns ``[K, ld)`` = +inf."""
    total, kk = rows.shape
    out = []
    for lo in range(0, total, n):
        idx = [(lo + i) % total for i in range(n)]
        buf = torch.full((offset + n * ld,), INF)
        view = buf[offset:].view(n, ld)
        view[:, :kk] = rows[idx]
        dev = buf.to(dtype).to(device)
        x = dev[offset:].view(n, ld)[:, :kk]
        out.append((x, labels[idx], weights[idx]))
    return out


# ------------------------------------------------------------------------------------------------------ reduce
def oracle_pair(values, weights=None, wscale=1.0):
    """{total, count} with correctly rounded sums (``math.fsum``) of the exact fp64 products; weight 0 is skipped."""
    v = [float(x) for x in values.reshape(-1).double().tolist()]
    w = [1.0] * len(v) if weights is None else [float(x) for x in weights.reshape(-1).double().tolist()]
    assert len(v) == len(w)
    total = math.fsum(wi * vi for wi, vi in zip(w, v) if wi != 0.0)
    count = math.fsum(wi for wi in w if wi != 0.0)
    if wscale == 0.0 or not v:
        return [0.0, 0.0]
    return [wscale * total, wscale * count]


def bound(values, weights, n):
    """N * 2^-53 * sum |w v| (and the same form for the count): the products of two fp32 are exact in fp64, so only
    the at most N - 1 additions round, each by at most 2^-53 relative to a partial sum of magnitude <= sum |w v|."""
    w = torch.ones_like(values) if weights is None else weights
    return (n * 2.0 ** -53 * float((w.double() * values.double()).abs().sum()),
            n * 2.0 ** -53 * float(w.double().abs().sum()))


# ------------------------------------------------------------------------------------------------------ Eval
class ListLoader(object):
    """Serves the given (input, ground truth) batches in turn and records what it served."""
    type = "SyntheticDataLoader"

    def __init__(self, batches):
        self.batches, self.served = list(batches), []
        self.batch_size = int(batches[0][0].shape[0])

    def _next(self):
        b = self.batches[len(self.served) % len(self.batches)]
        self.served.append(b)
        return b

    def load_train_batch(self, name_queue=None, *args, **kwargs):
        from mdtf.train import step as S
        return S.BatchSource(self._next, name="list").outputs(2)

    def load_eval_batch(self, *args, **kwargs):
        return self.load_train_batch()


def class_batches(count, batch, classes=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 8, generator=g), torch.randint(0, classes, (batch,), generator=g))
            for _ in range(count)]


def classifier():
    """A 10-class linear model and its mean cross entropy."""
    from mdtf.ops import nn as ops
    from mdtf.runtime import Loss, Model
    from mdtf.train import variables as V

    class Lin10(Model):
        def inference(self, x):
            w = V.get_variable("dense/w", [8, 10], initializer=V.random_normal_initializer(stddev=0.3))
            b = V.get_variable("dense/b", [10], initializer=V.constant_initializer(0.0))
            return x @ w + b

    class Xent(Loss):
        def loss(self, p, t):
            return ops.sparse_softmax_cross_entropy_with_logits(t, p).mean()

    return Lin10, Xent


def operator(cls, model_dir, net, loss, loader, server=None, **extra):
    """A run-loop operator with what the annotation entry point injects (the style of test_ema._operator)."""
    import mdtf
    from mdtf.cluster import ClusterSpec
    from mdtf.data.loaders import InputOptions
    from mdtf.runtime import Net
    if server is None:
        server = types.SimpleNamespace(is_chief=True, local_rank=0, target="", worker_group=None, store=None,
                                       layout=types.SimpleNamespace(num_worker_ranks=1),
                                       device=lambda: torch.device("cpu"), signal_done=lambda: None)
    op = cls.__new__(cls)
    attrs = dict(task_index=0, job_name="worker", optimizer=mdtf.train.MomentumOptimizer(0.1, 0.9), server=server,
                 cluster=ClusterSpec({"worker": ["127.0.0.1:1"]}), data_loader=loader,
                 input_mode=InputOptions.SYNTHETIC, batch_size=loader.batch_size, epoch_num=1,
                 sample_number=loader.batch_size * 5, model_dir=str(model_dir), data_dir="", net=Net(net), loss=loss,
                 gpu_num=0, ps_mode="allreduce")
    attrs.update(extra)
    for k, v in attrs.items():
        setattr(op, k, v)
    return op


def fresh():
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device = torch.device("cpu")
    store.compute_dtype = None
    return store


def eval_worker(rank, world, port, model_dir, out_dir, per_rank):
    """One gloo rank of a multi-replica Eval: rank r sees batches [r * per_rank, (r + 1) * per_rank)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dist_helpers as DH
    from mdtf.cluster import Server
    from mdtf.runtime.eval import Eval
    server = Server.from_env(backend="gloo")
    fresh()
    Lin10, Xent = classifier()
    batches = class_batches(world * per_rank, 8, seed=3)[rank * per_rank:(rank + 1) * per_rank]
    e = operator(Eval, model_dir, Lin10(), Xent(), ListLoader(batches), server=server, eval_steps=per_rank,
                 eval_top_k=3)
    m = e.run()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(m, f)
    DH._teardown(server)
