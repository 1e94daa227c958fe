"""Shared pieces of the moving-average tests (``tests/test_ema.py``; not collected as a test): the fp64 reference of
``tf.train.ExponentialMovingAverage`` written from TF's formula (it never calls ``mdtf.ops.ema``), the tiny model the
train-op tests run, the body of the spawned gloo ranks and of the kernel-variant child process.

The bound is ``optim_helpers``': ``|got - ref| <= gamma(K) * scale``.  One update ``e - omd * (e - w)`` rounds the
subtract (1), the product (2) and the final subtract (3): K = 3 for the PyTorch branch, 2 for the kernel's fma form;
its scale is ``|e| + omd * (|e| + |w|)``.  ``k`` consecutive updates carry the scale forward and are checked under
``k * K``.

Run as a script (``ema_helpers.py variant OUT``) it saves ``variant_outputs()`` to OUT: the variant test starts it as
a fresh process with ``MDTF_NT_OPT=0``, which the kernel library reads once.
"""
import json
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

K_EMA = 3


# ------------------------------------------------------------------------------------------------ the reference
def ref_start(w, ema):
    import optim_helpers as OH
    return OH.start(w=w, ema=ema)


def ref_step(st, w, omd):
    """e -= omd * (e - w), omd rounded to fp32 first (what the kernel's float argument holds)."""
    import optim_helpers as OH
    omd = OH.f32(omd)
    w = w.detach().cpu().double()
    e, se = st["ema"]
    st["ema"] = [e - omd * (e - w), se + abs(omd) * (se + w.abs())]
    st["w"] = [w, w.abs()]


def omd_of(decay, n=None):
    """1 - min(decay, (1 + n) / (10 + n)) in double (n None: the constant decay), rounded to fp32 once."""
    import optim_helpers as OH
    if n is not None:
        decay = min(decay, (1.0 + n) / (10.0 + n))
    return OH.f32(1.0 - decay)


# ------------------------------------------------------------------------------------------------ the tiny model
def linear_setup(world, batch, seed=0):
    """clip_helpers' three-variable model and data, plus a non-trainable ``dense/moving_mean`` (what BN's moving
    statistics are to a checkpoint); the input is cast to the weights' dtype, so it also runs with bf16 shadows."""
    import clip_helpers as CH
    from mdtf.runtime import Model
    from mdtf.train import variables as V
    _, MSE, xs, ys, x_ph, y_ph = CH.linear_setup(world, batch, seed)

    class Lin(Model):
        def inference(self, x):
            V.get_variable("dense/moving_mean", [3], initializer=V.constant_initializer(0.0), trainable=False)
            w = V.get_variable("dense/w", [8, 3], initializer=V.constant_initializer(0.1))
            b = V.get_variable("dense/b", [3], initializer=V.constant_initializer(0.0))
            h = V.get_variable("dense2/w", [3, 1], initializer=V.constant_initializer(0.2))
            return (torch.tanh(x.to(w.dtype) @ w + b.to(w.dtype)) @ h).float()

    return Lin, MSE, xs, ys, x_ph, y_ph


def build(batch, world=1, ema_kwargs=None, sync_kwargs=None, lr=0.1, clip_norm=None):
    """Momentum SGD over the tiny model (``clip_norm``: with ``global_clipnorm=``); ``ema_kwargs`` (None: no
    average) may hold ``num_updates="global_step"``.
    Returns (op, loss, ema or None, xs, ys, x_ph, y_ph)."""
    import mdtf
    from mdtf.runtime import Net, Tower
    Lin, MSE, xs, ys, x_ph, y_ph = linear_setup(world, batch)
    base = mdtf.train.MomentumOptimizer(lr, 0.9, global_clipnorm=clip_norm)
    tg = []
    tower = Tower(Net(Lin()), "tower_0/", tg, x_ph, y_ph, MSE(), base, batch_size=batch)
    _, loss, _ = tower.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, **sync_kwargs) if sync_kwargs is not None else base
    gs = mdtf.train.get_or_create_global_step()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=gs)
    ema = None
    if ema_kwargs is not None:
        kw = dict(ema_kwargs)
        if kw.get("num_updates") == "global_step":
            kw["num_updates"] = gs
        ema = mdtf.train.ExponentialMovingAverage(**kw)
        assert ema.apply(train_op=op) is op
    return op, loss, ema, xs, ys, x_ph, y_ph


def fresh(device="cpu", compute_dtype=None):
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device = torch.device(device)
    store.compute_dtype = compute_dtype
    return store


def flat_weights():
    """Every trainable variable's fp32 master, concatenated in creation order (CPU copy)."""
    from mdtf.train import variables as V
    return torch.cat([v.master.detach().reshape(-1).float().cpu() for v in V.get_store().trainable_variables()])


def flat_averages(ema):
    from mdtf.train import variables as V
    return torch.cat([ema.average(v).reshape(-1).cpu() for v in V.get_store().trainable_variables()])


def train(steps, ema_kwargs, device="cpu", batch=8, compute_dtype=None, sync_kwargs=None, clip_norm=None):
    """A fresh store, ``steps`` steps.  Returns dict(w0, ws (after every step), losses, avg, op, ema, sess)."""
    import mdtf
    fresh(device, compute_dtype)
    op, loss, ema, xs, ys, x_ph, y_ph = build(batch, ema_kwargs=ema_kwargs, sync_kwargs=sync_kwargs,
                                              clip_norm=clip_norm)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    out = dict(w0=flat_weights(), ws=[], losses=[], op=op, ema=ema, sess=sess, feed={x_ph: xs, y_ph: ys}, loss=loss)
    for _ in range(steps):
        _, lv = sess.run([op, loss], feed_dict=out["feed"])
        out["losses"].append(float(lv))
        out["ws"].append(flat_weights())
    out["avg"] = flat_averages(ema) if ema is not None else None
    return out


def recurrence(w0, ws, omds):
    """The host fp64 recurrence e_0 = w_0, e_t = e_{t-1} - omd_t (e_{t-1} - w_t) with its carried scale."""
    st = ref_start(w0, w0)
    for w, omd in zip(ws, omds):
        ref_step(st, w, omd)
    return st


# ------------------------------------------------------------------------------------------------ two-rank gloo
def ema_worker(rank, world, port, mode, steps, out_dir, batch=4):
    """One gloo rank of synchronous training with an average whose decay follows the global step; afterwards a
    collective checkpoint, one more step, and a restore of that checkpoint."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    import mdtf
    from dist_helpers import _teardown
    from mdtf.cluster import Server
    from mdtf.train import variables as V
    server = Server.from_env(backend="gloo")
    op, loss, ema, xs, ys, x_ph, y_ph = build(
        batch, world=world, ema_kwargs=dict(decay=0.999, num_updates="global_step"),
        sync_kwargs=dict(replicas_to_aggregate=world, total_num_replicas=world, mode=mode, bucket_bytes=64))
    hook = op.optimizer.make_session_run_hook(rank == 0)
    sess = mdtf.train.MonitoredTrainingSession(is_chief=rank == 0, hooks=[hook], log_step_count_steps=0,
                                               server=server)
    lo, hi = rank * batch, (rank + 1) * batch
    feed = {x_ph: xs[lo:hi], y_ph: ys[lo:hi]}
    op.reducer.gather_full_master()
    res = {"w0": flat_weights().tolist(), "ws": [], "collective": bool(op.reducer.collective),
           "buckets": len(op.space.buckets)}
    for _ in range(steps):
        sess.run(op, feed_dict=feed)
        op.reducer.gather_full_master()
        res["ws"].append(flat_weights().tolist())
    res["avg"] = flat_averages(ema).tolist()                  # collective in sharded mode
    res["state_keys"] = sorted(k[0] for g in op.space.groups for k in g.state)
    saver = mdtf.train.Saver()
    path = saver.save(sess, os.path.join(out_dir, "model.ckpt"), global_step=V.get_global_step())
    sess.run(op, feed_dict=feed)                              # the state moves on ...
    res["avg_after"] = flat_averages(ema).tolist()
    import torch.distributed as dist
    dist.barrier()                                            # the chief's files are complete
    saver.restore(sess, path)                                 # ... and comes back
    op.reducer.gather_full_master()
    res["restored_w"] = flat_weights().tolist()
    res["restored_avg"] = flat_averages(ema).tolist()
    res["restored_step"] = V.get_global_step().value()
    sess.close()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(res, f)
    _teardown(server)


# ------------------------------------------------------------------------------------------------ GPU: conv model
class _TinyRes(object):
    def inference(self, x):
        from mdtf.layers import tools
        from mdtf.ops import nn as ops
        from mdtf.train import variables as V
        store = V.get_store()
        if store.compute_dtype is not None:
            x = x.to(store.compute_dtype)
        s = tools.conv_bn("c1", x, 64, 3, 1, relu=True)
        y = tools.conv_bn("c2", s, 64, 1, 1, relu=True)
        x = tools.conv_bn("c3", y, 64, 3, 1, relu=True, residual=s)
        x = tools.conv_bn("c4", x, 128, 3, 2, relu=True)
        x = ops.global_avg_pool(x)
        return tools.dense("logits", x, 16)


def run_resnetish(batches, hip_graph, mode="allreduce", decay=0.999, clip_norm=None):
    """A small conv net with bf16 shadows on the GPU (as ``tests/test_hip_graph.py``), momentum SGD with a decaying
    LR (``clip_norm``: and ``global_clipnorm=``) and an average whose decay follows the global step.  Returns (losses, weights, averages, op)."""
    import mdtf
    from mdtf.models import SoftmaxCrossEntropyLoss
    from mdtf.runtime import Model, Net, Tower
    store = fresh("cuda", torch.bfloat16)
    store.generator.manual_seed(7)
    x0, _ = batches[0]
    xp = mdtf.placeholder(torch.float32, [None] + list(x0.shape[1:]))
    yp = mdtf.placeholder(torch.int64, [None])
    base = mdtf.train.MomentumOptimizer(lambda step: 0.05 / (1 + step), 0.9, weight_decay=1e-4,
                                        global_clipnorm=clip_norm)
    tg = []
    M = type("TinyResModel", (_TinyRes, Model), {})
    t = Tower(Net(M()), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), base, batch_size=x0.shape[0])
    _, loss, _ = t.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, hip_graph=hip_graph, mode=mode, bucket_bytes=1 << 18)
    gs = mdtf.train.get_or_create_global_step()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=gs)
    ema = mdtf.train.ExponentialMovingAverage(decay, num_updates=gs)
    ema.apply(train_op=op)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    losses = []
    for x, y in batches:
        _, lv = sess.run([op, loss], feed_dict={xp: x, yp: y})
        losses.append(lv)
    losses = [float(v) for v in losses]
    op.reducer.gather_full_master()            # sharded mode: the full fp32 masters are current only on demand
    vs = store.trainable_variables()
    weights = {v.name: v.value().detach().float().cpu().clone() for v in vs}
    averages = {v.name: ema.average(v).cpu() for v in vs}
    return losses, weights, averages, op


# ------------------------------------------------------------------------------------------------ kernel variants
VARIANT_N = 2 * 4096 + 4 * 257          # two full chunks and a ragged third (asserted against E.CHUNK by the test)


def variant_outputs():
    """Five consecutive GPU updates (scalar decay, then the device buffer) on seeded inputs; outputs on the CPU."""
    import optim_helpers as OH
    from mdtf.ops import _native
    from mdtf.ops import ema as E
    _native.lib()
    assert _native.mode() != "torch"
    inp = OH.make_inputs(VARIANT_N, 51, k=5)
    gen = torch.Generator().manual_seed(52)
    e = torch.randn(VARIANT_N, generator=gen).cuda()
    out = {}
    dev = torch.zeros(1, device="cuda")
    for i, omd in enumerate([0.1, 1e-3, 0.5, 1e-4, 1.0]):
        w = (inp["w"] + 1e-3 * inp["g"][i]).cuda()
        if i % 2:
            dev.fill_(omd)
            E.ema_update_(e, w, 0.77, omd_dev=dev)
        else:
            E.ema_update_(e, w, E.one_minus_decay(1.0 - omd))
        out["ema%d" % i] = e.cpu()
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    assert sys.argv[1] == "variant"
    torch.save(variant_outputs(), sys.argv[2])
