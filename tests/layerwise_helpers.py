"""Shared pieces of the LAMB / LARS tests: plain-torch references over the tiny three-variable model of
``clip_helpers.linear_setup``, the fp64 formulas the kernels are checked against, the train-op builder and the body of
the spawned gloo ranks."""
import json
import math
import os

import torch

LAMB_HP = dict(lr=0.01, wd=0.01, b1=0.9, b2=0.999, eps=1e-6)
LARS_HP = dict(lr=0.1, momentum=0.9, wd=1e-4, eeta=0.05, eps=0.0)
DECAY = {"dense/w": True, "dense/b": False, "dense2/w": True}      # rank > 1


def _norm(t):
    return math.sqrt(float(t.double().pow(2).sum()))


def torch_reference(kind, xs, ys, steps, clip_norm=None, nesterov=False):
    """Plain torch LAMB / LARS on the tiny model: autograd, fp64 norms, one variable at a time.
    Returns (weights by name, per-step pre-clip global norms, per-step {name: ratio})."""
    w = torch.full((8, 3), 0.1, requires_grad=True)
    b = torch.zeros(3, requires_grad=True)
    h = torch.full((3, 1), 0.2, requires_grad=True)
    names = ["dense/w", "dense/b", "dense2/w"]
    params = [w, b, h]
    s1 = [torch.zeros_like(p) for p in params]
    s2 = [torch.zeros_like(p) for p in params]
    norms, ratios = [], []
    for _ in range(steps):
        loss = ((torch.tanh(xs @ w + b) @ h - ys) ** 2).mean()
        grads = torch.autograd.grad(loss, params)
        norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
        norms.append(norm)
        coef = 1.0 if not clip_norm else clip_norm / max(norm, clip_norm)
        rs = {}
        with torch.no_grad():
            for name, p, a, v, g in zip(names, params, s1, s2, grads):
                g = g * coef
                if kind == "lamb":
                    hp = LAMB_HP
                    a.mul_(hp["b1"]).add_(g, alpha=1 - hp["b1"])
                    v.mul_(hp["b2"]).addcmul_(g, g, value=1 - hp["b2"])
                    u = a / (v.sqrt() + hp["eps"])
                    r = 1.0
                    if DECAY[name]:
                        u = u + hp["wd"] * p
                        wn, un = _norm(p), _norm(u)
                        r = wn / un if wn > 0 and un > 0 else 1.0
                    p.sub_(hp["lr"] * r * u)
                else:
                    hp = LARS_HP
                    r = 1.0
                    if DECAY[name]:
                        wn, gn = _norm(p), _norm(g)
                        if wn > 0 and gn > 0:
                            r = hp["eeta"] * wn / (gn + hp["wd"] * wn + hp["eps"])
                        g = g + hp["wd"] * p
                    s = hp["lr"] * r * g
                    a.mul_(hp["momentum"]).add_(s)
                    p.sub_(s + hp["momentum"] * a if nesterov else a)
                rs[name] = r
        ratios.append(rs)
    return dict(zip(names, [p.detach() for p in params])), norms, ratios


def clip_between(kind, xs, ys, steps):
    """A clip_norm between the smallest and the largest unclipped reference norm (as clip_helpers.clip_between)."""
    _, norms, _ = torch_reference(kind, xs, ys, steps)
    return 0.5 * (min(norms) + max(norms))


def make_optimizer(kind, clip_norm=None, nesterov=False, lr=None):
    import mdtf
    if kind == "lamb":
        hp = LAMB_HP
        return mdtf.train.LAMBOptimizer(lr if lr is not None else hp["lr"], weight_decay_rate=hp["wd"],
                                        beta_1=hp["b1"], beta_2=hp["b2"], epsilon=hp["eps"],
                                        global_clipnorm=clip_norm)
    hp = LARS_HP
    return mdtf.train.LARSOptimizer(lr if lr is not None else hp["lr"], momentum=hp["momentum"],
                                    weight_decay=hp["wd"], eeta=hp["eeta"], epsilon=hp["eps"],
                                    use_nesterov=nesterov, global_clipnorm=clip_norm)


def build_train(kind, x_ph, y_ph, Lin, MSE, batch, clip_norm=None, sync_kwargs=None, nesterov=False):
    """The train op over the tiny model.  Returns (op, loss, optimizer, base optimizer)."""
    import mdtf
    from mdtf.runtime import Net, Tower
    base = make_optimizer(kind, clip_norm, nesterov)
    tg = []
    tower = Tower(Net(Lin()), "tower_0/", tg, x_ph, y_ph, MSE(), base, batch_size=batch)
    _, loss, _ = tower.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, **sync_kwargs) if sync_kwargs is not None else base
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    return op, loss, opt, base


def weights():
    import mdtf
    from mdtf.train import variables as V
    return {mdtf.runtime.tower.strip_tower_prefix(v.name): v.master.detach().clone()
            for v in V.get_store().trainable_variables()}


def worker(rank, world, port, mode, kind, steps, out_dir, batch=4):
    """One gloo rank of synchronous LAMB / LARS training (tiny buckets: shard boundaries cut variables)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mdtf
    from clip_helpers import linear_setup
    from dist_helpers import _teardown
    from mdtf.cluster import Server
    from mdtf.train import variables as V
    server = Server.from_env(backend="gloo")
    Lin, MSE, xs, ys, x_ph, y_ph = linear_setup(world, batch)
    op, loss, opt, base = build_train(kind, x_ph, y_ph, Lin, MSE, batch,
                                      sync_kwargs=dict(replicas_to_aggregate=world, total_num_replicas=world,
                                                       mode=mode, bucket_bytes=64))
    hook = opt.make_session_run_hook(rank == 0)
    sess = mdtf.train.MonitoredTrainingSession(is_chief=rank == 0, hooks=[hook], log_step_count_steps=0,
                                               server=server)
    lo, hi = rank * batch, (rank + 1) * batch
    ratios = []
    for _ in range(steps):
        sess.run(op, feed_dict={x_ph: xs[lo:hi], y_ph: ys[lo:hi]})
        ratios.append([float(r).hex() for r in base.last_ratios.tolist()])
    sess.close()
    op.reducer.gather_full_master()
    w = {v.name: [float(x).hex() for x in v.master.reshape(-1).tolist()] for v in V.get_store().trainable_variables()}
    cut = [[p for ps in op._layer_map.pieces for p in ps if p[2] == l] for l in range(op._layer_map.num_layers)]
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump({"weights": w, "ratios": ratios, "collective": bool(op.reducer.collective),
                   "names": list(base.last_layer_names), "pieces": cut}, f)
    _teardown(server)


# ---------------------------------------------------------------------------------------- fp64 formulas (ops tests)
def f32(x):
    """A Python float rounded to fp32 (what a kernel's float argument holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def layer_index(pieces, nl):
    """Per layer: one index tensor per target over the elements of its pieces."""
    out = [[[] for _ in pieces] for _ in range(nl)]
    for ti, ps in enumerate(pieces):
        for o, n, l in ps:
            out[l][ti].append(torch.arange(o, o + n))
    return [[torch.cat(ix) if ix else None for ix in per] for per in out]


def _ratio_lamb(sw, su):
    if not (math.isfinite(sw) and math.isfinite(su)):
        return float("nan")
    return math.sqrt(sw) / math.sqrt(su) if sw > 0 and su > 0 else 1.0


def _ratio_lars(sw, sg, gs, eeta, wd, eps):
    if not (math.isfinite(sw) and math.isfinite(sg)):
        return float("nan")
    wn, gn = math.sqrt(sw), gs * math.sqrt(sg)
    return eeta * wn / (gn + wd * wn + eps) if wn > 0 and gn > 0 else 1.0


def lamb_fp64(pieces, decay, ws, gs_, ms, vs, lr, b1, b2, eps, gscale, wd):
    """The LAMB formulas in fp64 from fp32 inputs (hyper-parameters rounded to fp32 as the kernel's arguments,
    1 - beta computed in fp32 as the kernel does).  ws / gs_ / ms / vs: one CPU fp32 tensor per target.  Returns
    (w, m, v per target in fp64, sums [(sum w^2, sum u^2)], ratios)."""
    lr, b1, b2, eps, gscale, wd = (f32(x) for x in (lr, b1, b2, eps, gscale, wd))
    c1, c2 = f32(torch.tensor(1.0) - torch.tensor(b1)), f32(torch.tensor(1.0) - torch.tensor(b2))
    W = [t.double().clone() for t in ws]
    M = [t.double().clone() for t in ms]
    Vv = [t.double().clone() for t in vs]
    sums, ratios = [], []
    for l, per in enumerate(layer_index(pieces, len(decay))):
        sw = su = 0.0
        us = []
        for ti, ix in enumerate(per):
            if ix is None:
                us.append(None)
                continue
            g = gs_[ti].double()[ix] * gscale
            M[ti][ix] = b1 * M[ti][ix] + c1 * g
            Vv[ti][ix] = b2 * Vv[ti][ix] + c2 * g * g
            u = M[ti][ix] / (Vv[ti][ix].sqrt() + eps) + (wd if decay[l] else 0.0) * W[ti][ix]
            us.append(u)
            sw += float(W[ti][ix].pow(2).sum())
            su += float(u.pow(2).sum())
        r = _ratio_lamb(sw, su) if decay[l] else 1.0
        for ti, ix in enumerate(per):
            if ix is not None:
                W[ti][ix] = W[ti][ix] - lr * r * us[ti]
        sums.append((sw, su))
        ratios.append(r)
    return W, M, Vv, sums, ratios


def lars_fp64(pieces, decay, ws, gs_, accs, lr, mom, gscale, wd, eeta, eps, nesterov=False):
    """The LARS formulas in fp64 from fp32 inputs.  Returns (w, acc per target, sums [(sum w^2, sum g^2)], ratios)."""
    lr, mom, gscale, wd, eeta, eps = (f32(x) for x in (lr, mom, gscale, wd, eeta, eps))
    W = [t.double().clone() for t in ws]
    A = [t.double().clone() for t in accs]
    sums, ratios = [], []
    for l, per in enumerate(layer_index(pieces, len(decay))):
        sw = sg = 0.0
        for ti, ix in enumerate(per):
            if ix is not None:
                sw += float(W[ti][ix].pow(2).sum())
                sg += float(gs_[ti].double()[ix].pow(2).sum())
        r = _ratio_lars(sw, sg, gscale, eeta, wd, eps) if decay[l] else 1.0
        for ti, ix in enumerate(per):
            if ix is None:
                continue
            s = lr * r * (gs_[ti].double()[ix] * gscale + (wd if decay[l] else 0.0) * W[ti][ix])
            A[ti][ix] = mom * A[ti][ix] + s
            W[ti][ix] = W[ti][ix] - (s + mom * A[ti][ix] if nesterov else A[ti][ix])
        sums.append((sw, sg))
        ratios.append(r)
    return W, A, sums, ratios
