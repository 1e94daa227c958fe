"""Shared pieces of the global-norm clipping tests: the tiny three-variable model (as ``dist_helpers._linear_setup``),
a plain-torch reference of clipped momentum training, and the body of the spawned gloo ranks."""
import json
import math
import os

import torch


def linear_setup(world, batch, seed=0):
    import mdtf
    from mdtf.runtime import Loss, Model
    from mdtf.train import variables as V

    class Lin(Model):
        def inference(self, x):
            w = V.get_variable("dense/w", [8, 3], initializer=V.constant_initializer(0.1))
            b = V.get_variable("dense/b", [3], initializer=V.constant_initializer(0.0))
            h = V.get_variable("dense2/w", [3, 1], initializer=V.constant_initializer(0.2))
            return torch.tanh(x @ w + b) @ h

    class MSE(Loss):
        def loss(self, p, t):
            return ((p - t) ** 2).mean()

    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(world * batch, 8, generator=g)
    ys = torch.randn(world * batch, 1, generator=g)
    x_ph = mdtf.placeholder(torch.float32, [None, 8])
    y_ph = mdtf.placeholder(torch.float32, [None, 1])
    return Lin, MSE, xs, ys, x_ph, y_ph


def torch_reference(xs, ys, steps, clip_norm=None, lr=0.1, momentum=0.9):
    """Plain torch: autograd, norm = sqrt(fp64 sum of squares), coef = clip / max(norm, clip), momentum update.
    Returns (weights by variable name, per-step pre-clip norms)."""
    w = torch.full((8, 3), 0.1, requires_grad=True)
    b = torch.zeros(3, requires_grad=True)
    h = torch.full((3, 1), 0.2, requires_grad=True)
    params = [w, b, h]
    acc = [torch.zeros_like(p) for p in params]
    norms = []
    for _ in range(steps):
        loss = ((torch.tanh(xs @ w + b) @ h - ys) ** 2).mean()
        grads = torch.autograd.grad(loss, params)
        norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
        norms.append(norm)
        coef = 1.0 if not clip_norm else clip_norm / max(norm, clip_norm)
        with torch.no_grad():
            for p, a, g in zip(params, acc, grads):
                a.mul_(momentum).add_(g * coef)
                p.sub_(lr * a)
    return {"dense/w": w.detach(), "dense/b": b.detach(), "dense2/w": h.detach()}, norms


def clip_between(xs, ys, steps):
    """A clip_norm between the smallest and the largest unclipped reference norm."""
    _, norms = torch_reference(xs, ys, steps)
    return 0.5 * (min(norms) + max(norms))


def build_train(xs, x_ph, y_ph, Lin, MSE, clip_norm, how, batch, sync_kwargs=None):
    """The train op over the tiny model.  how: 'call' (clip_by_global_norm), 'keyword' (global_clipnorm=),
    'norm' (global_norm only), None (no clip).  Returns (op, loss, norm handle or None, optimizer)."""
    import mdtf
    from mdtf.runtime import Net, Tower
    base = mdtf.train.MomentumOptimizer(0.1, 0.9, global_clipnorm=clip_norm if how == "keyword" else None)
    tg = []
    tower = Tower(Net(Lin()), "tower_0/", tg, x_ph, y_ph, MSE(), base, batch_size=batch)
    _, loss, _ = tower.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, **sync_kwargs) if sync_kwargs is not None else base
    gv = Tower.average_gradients(tg)
    gnorm = None
    if how == "call":
        grads, vs = zip(*gv)
        clipped, gnorm = mdtf.train.clip_by_global_norm(grads, clip_norm)
        gv = list(zip(clipped, vs))
    elif how == "norm":
        gnorm = mdtf.train.global_norm([g for g, _ in gv])
    op = opt.apply_gradients(gv, global_step=mdtf.train.get_or_create_global_step())
    return op, loss, gnorm, opt


def clip_worker(rank, world, port, mode, steps, out_dir, clip_norm, batch=4):
    """One gloo rank of clipped synchronous training (tiny buckets, as dist_helpers.sync_worker)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mdtf
    from dist_helpers import _teardown
    from mdtf.cluster import Server
    from mdtf.train import variables as V
    server = Server.from_env(backend="gloo")
    Lin, MSE, xs, ys, x_ph, y_ph = linear_setup(world, batch)
    op, loss, gnorm, opt = build_train(xs, x_ph, y_ph, Lin, MSE, clip_norm, "call", batch,
                                       sync_kwargs=dict(replicas_to_aggregate=world, total_num_replicas=world,
                                                        mode=mode, bucket_bytes=64))
    hook = opt.make_session_run_hook(rank == 0)
    sess = mdtf.train.MonitoredTrainingSession(is_chief=rank == 0, hooks=[hook], log_step_count_steps=0,
                                               server=server)
    lo, hi = rank * batch, (rank + 1) * batch
    norms, coefs = [], []
    for _ in range(steps):
        _, n = sess.run([op, gnorm], feed_dict={x_ph: xs[lo:hi], y_ph: ys[lo:hi]})
        norms.append(float(n).hex())                      # bitwise comparison across ranks
        coefs.append(float(op.last_global_norm[1]).hex())
    sess.close()
    op.reducer.gather_full_master()
    w = {v.name: v.master.tolist() for v in V.get_store().trainable_variables()}
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump({"weights": w, "norms": norms, "coefs": coefs, "collective": bool(op.reducer.collective)}, f)
    _teardown(server)
