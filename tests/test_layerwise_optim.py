"""LAMB and LARS (``mdtf.train.LAMBOptimizer`` / ``LARSOptimizer``), ``mdtf.ops.layerwise`` and
``csrc/layerwise.hip``: per-layer trust ratios computed on the device.

CPU tests run the PyTorch reference path of ``ops.layerwise``, GPU tests the HIP kernels.
"""
import json
import math
import os
import sys
import types

import pytest
import torch

import mdtf
from mdtf.ops import layerwise as LW

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_helpers as CH  # noqa: E402
import layerwise_helpers as LH  # noqa: E402


def _rel(a, b):
    """tests/test_kernels_gpu.py::_rel"""
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _run_lamb(lmap, buf, ws, gs, ms, vs, shadows, lr, hp, gscale, dyn=None, split=False):
    for ti in range(len(ws)):
        LW.lamb_moments_(lmap, buf, ti, ws[ti], gs[ti], ms[ti], vs[ti], hp["b1"], hp["b2"], hp["eps"], gscale,
                         hp["wd"], dyn=dyn)
    if split:
        LW.layer_finalize_(lmap, buf, LW.LAMB, grad_scale=gscale, dyn=dyn, mode=LW.REDUCE)
        LW.layer_finalize_(lmap, buf, LW.LAMB, grad_scale=gscale, dyn=dyn, mode=LW.COEF)
    else:
        LW.layer_finalize_(lmap, buf, LW.LAMB, grad_scale=gscale, dyn=dyn)
    for ti in range(len(ws)):
        LW.lamb_apply_(lmap, buf, ti, ws[ti], ms[ti], vs[ti], shadows[ti], lr, hp["eps"], hp["wd"], dyn=dyn)


def _run_lars(lmap, buf, ws, gs, accs, shadows, lr, hp, gscale, dyn=None, split=False, nesterov=False):
    kw = dict(eeta=hp["eeta"], weight_decay=hp["wd"], epsilon=hp["eps"], grad_scale=gscale, dyn=dyn)
    for ti in range(len(ws)):
        LW.lars_norms_(lmap, buf, ti, ws[ti], gs[ti])
    if split:
        LW.layer_finalize_(lmap, buf, LW.LARS, mode=LW.REDUCE, **kw)
        LW.layer_finalize_(lmap, buf, LW.LARS, mode=LW.COEF, **kw)
    else:
        LW.layer_finalize_(lmap, buf, LW.LARS, **kw)
    for ti in range(len(ws)):
        LW.lars_apply_(lmap, buf, ti, ws[ti], gs[ti], accs[ti], shadows[ti], lr, hp["momentum"], gscale, hp["wd"],
                       nesterov, dyn=dyn)


# hand-made layouts: (decay flags, pieces per target, target sizes).  Layer 1 of the three-target layout is split in
# two adjacent pieces; 8 elements of padding follow some pieces (never covered by a piece, or zeros inside one)
_LAYOUTS = {
    1: ([True, False, True], [[(0, 64, 0), (64, 8, 1), (72, 120, 2)]], [192]),
    3: ([True, True, False, True, True],
        [[(0, 32, 0), (32, 16, 1), (48, 16, 1)], [(0, 12, 2), (16, 48, 3)], [(8, 100, 4)]], [64, 64, 128]),
}


def _state(sizes, pieces, seed, device="cpu", gscale=1.0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda f: [f(n) for n in sizes]                                                # noqa: E731
    ws = mk(lambda n: torch.randn(n, generator=g))
    gs = mk(lambda n: torch.randn(n, generator=g) * gscale)
    ms = mk(lambda n: torch.randn(n, generator=g) * gscale)
    vs = mk(lambda n: (0.5 + torch.rand(n, generator=g)) * gscale * gscale)
    accs = mk(lambda n: torch.randn(n, generator=g) * 0.01)
    # everything outside the pieces, and the last 4 elements of every piece, is zero padding
    for ti, ps in enumerate(pieces):
        keep = torch.zeros(sizes[ti], dtype=torch.bool)
        for o, n, _ in ps:
            keep[o:o + n - 4] = True
        for t in (ws, gs, ms, vs, accs):
            t[ti][~keep] = 0
    return [[x.to(device) for x in t] for t in (ws, gs, ms, vs, accs)]


# ------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("ntargets", [1, 3])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_reference_path_math(kind, ntargets):
    decay, pieces, sizes = _LAYOUTS[ntargets]
    lr, gscale = 0.1, 0.3
    for split in (False, True):
        ws, gs, ms, vs, accs = _state(sizes, pieces, 3)
        ws0 = [w.clone() for w in ws]
        lmap = LW.LayerMap(decay, pieces, "cpu")
        buf = LW.LayerBuffers(lmap)
        assert not lmap.native and lmap.num_layers == len(decay)
        if kind == "lamb":
            hp = LH.LAMB_HP
            W, M, Vv, sums, ratios = LH.lamb_fp64(pieces, decay, ws, gs, ms, vs, lr, hp["b1"], hp["b2"], hp["eps"],
                                                   gscale, hp["wd"])
            _run_lamb(lmap, buf, ws, gs, ms, vs, [None] * len(ws), lr, hp, gscale, split=split)
            for ti in range(len(ws)):
                assert _rel(ms[ti], M[ti]) < 1e-6 and _rel(vs[ti], Vv[ti]) < 1e-6
        else:
            hp = LH.LARS_HP
            W, A, sums, ratios = LH.lars_fp64(pieces, decay, ws, gs, accs, lr, hp["momentum"], gscale, hp["wd"],
                                              hp["eeta"], hp["eps"])
            _run_lars(lmap, buf, ws, gs, accs, [None] * len(ws), lr, hp, gscale, split=split)
            for ti in range(len(ws)):
                assert _rel(accs[ti], A[ti]) < 1e-6
        assert buf.ratio.tolist() == pytest.approx(ratios, rel=1e-5)
        assert buf.sums.view(-1, 2).tolist() == [pytest.approx(s, rel=1e-5) for s in sums]
        assert all(r == 1.0 for r, d in zip(buf.ratio.tolist(), decay) if not d)
        assert len({round(r, 3) for r, d in zip(ratios, decay) if d}) > 1 or ntargets == 1
        for ti in range(len(ws)):
            assert _rel(ws[ti], W[ti]) < 1e-6
            assert not torch.equal(ws[ti], ws0[ti])
            # padding stays zero
            assert torch.equal(ws[ti] == 0, ws0[ti] == 0)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_reference_path_edges(kind):
    decay, pieces, sizes = _LAYOUTS[3]

    def ratios(mutate, lamb_hp=LH.LAMB_HP):
        ws, gs, ms, vs, accs = _state(sizes, pieces, 4)
        ms = [torch.zeros_like(m) for m in ms]
        vs = [torch.zeros_like(v) for v in vs]
        mutate(ws, gs)
        lmap = LW.LayerMap(decay, pieces, "cpu")
        buf = LW.LayerBuffers(lmap)
        if kind == "lamb":
            _run_lamb(lmap, buf, ws, gs, ms, vs, [None] * 3, 0.1, lamb_hp, 1.0)
        else:
            _run_lars(lmap, buf, ws, gs, accs, [None] * 3, 0.1, LH.LARS_HP, 1.0)
        return buf.ratio.tolist(), ws

    base, _ = ratios(lambda ws, gs: None)
    assert all(math.isfinite(r) for r in base) and base[0] != 1.0 and base[1] != 1.0 and base[2] == 1.0
    # zero weights (layer 0: target 0, [0, 32)): ratio exactly 1
    r, _ = ratios(lambda ws, gs: ws[0][0:32].zero_())
    assert r[0] == 1.0 and r[1] == base[1]
    # zero gradient (layer 1: two pieces; m = v = 0): ratio exactly 1.  LAMB's u still holds the decay term wd * w,
    # so its zero-gradient case is the one without weight decay; with it the ratio is |w| / |wd w|
    r, _ = ratios(lambda ws, gs: gs[0][32:64].zero_(), dict(LH.LAMB_HP, wd=0.0))
    assert r[1] == 1.0 and r[0] != 1.0
    if kind == "lamb":
        r, _ = ratios(lambda ws, gs: gs[0][32:64].zero_())
        assert r[1] == pytest.approx(1.0 / LH.f32(LH.LAMB_HP["wd"]), rel=1e-5)
    # zero gradient AND zero weights: 1
    r, _ = ratios(lambda ws, gs: (gs[0][32:64].zero_(), ws[0][32:64].zero_()))
    assert r[1] == 1.0
    # a non-finite gradient: NaN ratio, the layer's weights NaN, the other layers untouched by it
    for bad in (float("inf"), float("nan")):
        def poison(ws, gs):
            gs[1][20] = bad
        r, ws = ratios(poison)
        assert math.isnan(r[3]) and r[0] == base[0] and r[4] == base[4], bad
        assert torch.isnan(ws[1][16:60]).all() and not torch.isnan(ws[0]).any() and not torch.isnan(ws[2]).any()
    # a non-adjacent or overlapping piece list is refused
    with pytest.raises(ValueError):
        LW.LayerMap([True, True], [[(0, 8, 0), (8, 8, 1), (16, 8, 0)]], "cpu")
    with pytest.raises(ValueError):
        LW.LayerMap([True, True], [[(0, 8, 0), (4, 8, 1)]], "cpu")
    with pytest.raises(ValueError):
        LW.LayerMap([True], [[(0, 6, 0)]], "cpu")


def _train(kind, steps, xs, ys, clip_norm=None, nesterov=False, sync_kwargs=None):
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    Lin, MSE, _, _, x_ph, y_ph = CH.linear_setup(1, xs.shape[0])
    op, loss, opt, base = LH.build_train(kind, x_ph, y_ph, Lin, MSE, xs.shape[0], clip_norm, sync_kwargs, nesterov)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    ratios = []
    for _ in range(steps):
        sess.run(op, feed_dict={x_ph: xs, y_ph: ys})
        names = [mdtf.runtime.tower.strip_tower_prefix(n) for n in base.last_layer_names]
        ratios.append(dict(zip(names, base.last_ratios.tolist())))
    return LH.weights(), ratios, op, sess, (x_ph, y_ph)


@pytest.mark.parametrize("kind,nesterov", [("lamb", False), ("lars", False), ("lars", True)])
def test_end_to_end_matches_plain_torch(kind, nesterov):
    _, _, xs, ys, _, _ = CH.linear_setup(1, 8)
    steps = 5
    w_ref, n_ref, r_ref = LH.torch_reference(kind, xs, ys, steps, nesterov=nesterov)
    w, ratios, op, _, _ = _train(kind, steps, xs, ys, nesterov=nesterov)
    assert op.optimizer.layerwise and op.reducer.eager_update is None and op.clip is None
    assert op._layer_buf is not None and op._layer_map.num_layers == 3
    for name, ref in w_ref.items():
        assert _rel(w[name], ref) < 1e-6, name
    for got, want in zip(ratios, r_ref):
        assert got["dense/b"] == 1.0                                   # non-decay: exactly the plain step
        for name in ("dense/w", "dense2/w"):
            assert got[name] == pytest.approx(want[name], rel=1e-5) and got[name] != 1.0
    # dense/b (3 elements, non-decay) moved by exactly the ratio-1 formula: replay it alone from the reference's
    # gradients (the reference applies r = 1 to it by construction) and compare after ONE step, where both see the
    # same weights
    w1_ref, _, _ = LH.torch_reference(kind, xs, ys, 1, nesterov=nesterov)
    w1, _, _, _, _ = _train(kind, 1, xs, ys, nesterov=nesterov)
    assert _rel(w1["dense/b"], w1_ref["dense/b"]) < 1e-6 and float(w1["dense/b"].abs().sum()) > 0
    # the ratios matter: the same run with every ratio forced to 1 ends elsewhere
    assert any(abs(r["dense/w"] - 1.0) > 0.1 for r in ratios)
    # once more with a clip between the smallest and largest unclipped norm: the coefficient reaches g^
    clip = LH.clip_between(kind, xs, ys, steps)
    w_ref_c, n_c, _ = LH.torch_reference(kind, xs, ys, steps, clip, nesterov=nesterov)
    assert any(n > clip for n in n_c) and any(n <= clip for n in n_c), (clip, n_c)     # both branches taken
    w_c, _, op, _, _ = _train(kind, steps, xs, ys, clip_norm=clip, nesterov=nesterov)
    assert op.clip is not None and op.clip.clip_norm == clip
    for name, ref in w_ref_c.items():
        assert _rel(w_c[name], ref) < 1e-6, name
    assert _rel(w_c["dense/w"], w_ref["dense/w"]) > 1e-5               # and the clip did something


def test_layer_map_tiles_slots_across_ranks():
    """bucket_bytes=64, world 2: the pieces of rank 0 and rank 1 tile each variable's slot exactly once, and at
    least one variable is cut by a shard boundary."""
    from mdtf.parallel.flat import FlatParamSpace
    from mdtf.train import variables as V
    store = V.get_store()
    shapes = {"a": [8, 3], "b": [3], "c": [3, 1], "d": [10, 20], "e": [70]}
    vs = [V.get_variable(n, s, initializer=V.constant_initializer(0.1)) for n, s in shapes.items()]
    vs = [store.vars[n] for n in shapes]
    world = 2
    space = FlatParamSpace(vs, torch.device("cpu"), None, 64, pad_to=world)
    cut = 0
    for g in space.groups:
        for b in g.buckets:
            b.shard_len = b.numel // world
        off = 0
        for b in g.buckets:
            b.shard_offset = off
            off += b.shard_len
        full, names = LW.group_pieces(g)
        assert names == [v.name for v in g.variables]
        assert [o for o, _, _ in full] == list(g.offsets) and sum(n for _, n, _ in full) == g.numel
        cover = torch.zeros(g.numel, dtype=torch.int64)
        owner = torch.full((g.numel,), -1, dtype=torch.int64)
        per_layer_ranks = {}
        for rank in range(world):
            ps, _ = LW.shard_pieces(g, rank)
            LW.LayerMap([g.decay] * len(g.variables), [ps], "cpu")            # adjacent, aligned, no overlap
            for so, n, l in ps:
                b = [b for b in g.buckets if b.shard_offset <= so < b.shard_offset + b.shard_len][0]
                go = b.start + rank * b.shard_len + (so - b.shard_offset)
                cover[go:go + n] += 1
                assert (owner[go:go + n] == -1).all()
                owner[go:go + n] = l
                per_layer_ranks.setdefault(l, set()).add(rank)
        assert (cover == 1).all()
        for o, n, l in full:
            assert (owner[o:o + n] == l).all()
        # cut by a shard boundary: both ranks hold a piece, and the variable's own elements (not only its
        # padding) reach past its bucket's first shard
        cut += sum(1 for l, r in per_layer_ranks.items()
                   if len(r) == 2 and g.variables[l].numel() > g.variables[l].bucket.shard_len)
    assert cut >= 1


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_two_rank_gloo_training(mode, kind, tmp_path):
    import torch.multiprocessing as mp
    from mdtf.cluster.launcher import free_port
    world, steps, batch = 2, 5, 4
    _, _, xs, ys, _, _ = CH.linear_setup(world, batch)
    w_ref, _, r_ref = LH.torch_reference(kind, xs, ys, steps)
    mp.start_processes(LH.worker, args=(world, free_port(), mode, kind, steps, str(tmp_path), batch),
                       nprocs=world, join=True, start_method="spawn")
    res = [json.load(open(os.path.join(str(tmp_path), "rank%d.json" % r))) for r in range(world)]
    assert res[0]["collective"]
    assert res[0]["weights"] == res[1]["weights"]                      # bitwise (hex floats)
    assert res[0]["ratios"] == res[1]["ratios"] and len(res[0]["ratios"]) == steps
    if mode == "sharded":
        # a shard boundary cuts a variable: both ranks hold a piece of it
        assert any(res[0]["pieces"][l] and res[1]["pieces"][l] for l in range(len(res[0]["names"])))
    for r in res:
        for name, ref in w_ref.items():
            key = "tower_0/" + name if "tower_0/" + name in r["weights"] else name
            got = torch.tensor([float.fromhex(x) for x in r["weights"][key]]).view(ref.shape)
            assert _rel(got, ref) < 1e-6, (mode, name)
        names = [n[len("tower_0/"):] if n.startswith("tower_0/") else n for n in r["names"]]
        for got, want in zip(r["ratios"], r_ref):
            for n, x in zip(names, got):
                assert float.fromhex(x) == pytest.approx(want[n], rel=1e-5), (mode, n)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_checkpoint_resume_bitwise(kind, tmp_path):
    from mdtf.ckpt.tensor_bundle import BundleReader
    from mdtf.train.saver import Saver
    _, _, xs, ys, _, _ = CH.linear_setup(1, 8)
    w5, _, _, _, _ = _train(kind, 5, xs, ys)
    _, _, op, sess, (x_ph, y_ph) = _train(kind, 3, xs, ys)
    path = Saver().save(sess, str(tmp_path / "ckpt"))
    keys = set(BundleReader(path).keys())
    names = [v.name for v in op.variables]
    slots = ("adam_m", "adam_v") if kind == "lamb" else ("Momentum",)
    for n in names:
        for s in slots:
            assert "%s/%s" % (n, s) in keys, (n, s, sorted(keys))
    assert keys == set(names) | {"%s/%s" % (n, s) for n in names for s in slots} | {"global_step"}   # no extras
    # reset everything, rebuild, restore, two more steps
    _, _, op2, sess2, (x_ph, y_ph) = _train(kind, 0, xs, ys)
    op2.finalize()
    Saver().restore(sess2, path)
    assert op2.step_count == 3
    for _ in range(2):
        sess2.run(op2, feed_dict={x_ph: xs, y_ph: ys})
    w = LH.weights()
    for name in w5:
        assert torch.equal(w[name], w5[name]), name


def test_api():
    from mdtf.parallel.async_ps import AsyncWorker
    assert mdtf.train.Optimizer.layerwise is False and not mdtf.train.MomentumOptimizer(0.1).layerwise
    for kind in ("lamb", "lars"):
        opt = LH.make_optimizer(kind)
        assert opt.layerwise and opt.last_ratios is None
        assert mdtf.train.SyncReplicasOptimizer(opt).layerwise is True
        with pytest.raises(NotImplementedError):
            opt.update_multi(None, [], [])
        with pytest.raises(NotImplementedError):
            mdtf.train.SyncReplicasOptimizer(opt).update_multi(None, [], [])
        with pytest.raises(NotImplementedError, match="ps_mode"):
            AsyncWorker(types.SimpleNamespace(optimizer=opt), None, None, [], 10)
        with pytest.raises(NotImplementedError, match="ps_mode"):
            AsyncWorker(types.SimpleNamespace(optimizer=mdtf.train.SyncReplicasOptimizer(opt)), None, None, [], 10,
                        sync=True)
        assert LH.make_optimizer(kind, clip_norm=1.5).global_clipnorm == 1.5
    assert not mdtf.train.SyncReplicasOptimizer(mdtf.train.AdamOptimizer(0.1)).layerwise
    lamb = mdtf.train.LAMBOptimizer(1e-3)
    assert (lamb.weight_decay, lamb.beta1, lamb.beta2, lamb.epsilon, lamb.get_name()) == (0.0, 0.9, 0.999, 1e-6,
                                                                                          "LAMBOptimizer")
    assert lamb.slot_checkpoint_names() == [("m", "adam_m"), ("v", "adam_v")] and not lamb.extra_checkpoint_scalars(3)
    lars = mdtf.train.LARSOptimizer(0.1)
    assert (lars.momentum, lars.weight_decay, lars.eeta, lars.epsilon, lars.use_nesterov, lars.get_name()) == (
        0.9, 1e-4, 1e-3, 0.0, False, "LARSOptimizer")
    assert lars.slot_checkpoint_names() == [("momentum", "Momentum")] and not lars.extra_checkpoint_scalars(3)
    # a Momentum train op has no layer buffers
    _, _, xs, ys, _, _ = CH.linear_setup(1, 8)
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    Lin, MSE, _, _, x_ph, y_ph = CH.linear_setup(1, 8)
    op, _, _, _ = CH.build_train(xs, x_ph, y_ph, Lin, MSE, None, None, 8)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    sess.run(op, feed_dict={x_ph: xs, y_ph: ys})
    assert op._layer_buf is None and op._layer_map is None and getattr(op.reducer, "layer_state", None) is None


# ------------------------------------------------------------------------------------------------------ GPU
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mdtf.ops import _native
    _native.lib()


# target 0: less than a wave of float4s | the same | several layer boundaries inside one chunk | one full chunk plus
# a ragged item | many items | a non-decay layer; target 1: two layers (layer_finalize spans targets)
_GPU_SIZES = [64, 64, 192, 4160, (1 << 20) + 64, 64]
_GPU_DECAY = [True, True, True, True, True, False, True, True]
_GPU_T1 = [320, 4096 + 128]


def _gpu_layout(cut=None):
    """Pieces of the two targets.  cut: None (one piece per layer) | "both" (layer 3 as two adjacent pieces of 2080)
    | 0 / 1 (the "rank 0 / rank 1 of 2" lists: layers 0..2 and the first half of layer 3 | the rest)."""
    pieces0, off = [], 0
    for l, n in enumerate(_GPU_SIZES):
        if l == 3 and cut is not None:
            halves = [(off, n // 2, l), (off + n // 2, n // 2, l)]
            pieces0 += halves if cut == "both" else [halves[cut]]
        elif cut in (None, "both") or (cut == 0) == (l < 3):
            pieces0.append((off, n, l))
        off += n
    t1 = [(0, _GPU_T1[0], 6), (_GPU_T1[0], _GPU_T1[1], 7)]
    pieces1 = t1 if cut in (None, "both") else [t1[cut]]
    return [pieces0, pieces1], [off, sum(_GPU_T1)]


def _gpu_state(gscale, seed=11):
    pieces, sizes = _gpu_layout()
    ws, gs, ms, vs, accs = _state(sizes, pieces, seed, gscale=gscale)
    scale = 1.0
    for ps, w in zip(pieces, ws):           # w scaled per layer by 1, 3, 9, ...: neighbouring ratios differ ~3x
        for o, n, _ in ps:
            w[o:o + n] *= scale
            scale *= 3.0
    return pieces, sizes, [[x.cuda() for x in t] for t in (ws, gs, ms, vs, accs)]


# Relative tolerance of ``sums`` and ``ratio`` against fp64, from the kernel's arithmetic.  A sum of k non-negative
# fp32 terms has relative error <= k * 2^-24.  Longest path of one item (the cross-item sum is fp64): 4 float4 x 4 =
# 16 per-thread fma accumulations + 6 wave-shuffle levels + 2 LDS levels = 24 additions.  Roundings of u per element
# (lamb_moments): g * gs (1); m = b1 * m + c1 * g (3); v = b2 * v + c2 * g * g (4); sqrt (1); + eps (1); the
# division (1); the wd * w fma (1) = 12.  (24 + 12) * 2^-24; the square root halves it for the ratio, LARS has no u.
_K = 24 + 12
_RTOL = _K * 2.0 ** -24


def _gpu_run(kind, pieces, state, lr, gscale, split_lists=None, dyn=None, scalars=None):
    """One full three-launch sequence on clones of ``state``.  split_lists: the "rank r of 2" piece lists, run with
    the reduce-only finalize, ``sums`` added on the device, then the coefficient half on each."""
    ws, gs, ms, vs, accs = [[x.clone() for x in t] for t in state]
    shadows = [torch.zeros(w.numel(), dtype=torch.bfloat16, device="cuda") for w in ws]
    hp = LH.LAMB_HP if kind == "lamb" else LH.LARS_HP
    s_lr, s_gs = scalars if scalars is not None else (lr, gscale)
    if split_lists is None:
        lmap = LW.LayerMap(_GPU_DECAY, pieces, "cuda")
        buf = LW.LayerBuffers(lmap)
        assert lmap.native
        if kind == "lamb":
            _run_lamb(lmap, buf, ws, gs, ms, vs, shadows, s_lr, hp, s_gs, dyn=dyn)
        else:
            _run_lars(lmap, buf, ws, gs, accs, shadows, s_lr, hp, s_gs, dyn=dyn)
        return dict(w=ws, m=ms, v=vs, acc=accs, shadow=shadows, ratio=buf.ratio.clone(), sums=buf.sums.clone(),
                    partials=buf.partials.clone(), lmap=lmap)
    maps = [LW.LayerMap(_GPU_DECAY, ps, "cuda") for ps in split_lists]
    bufs = [LW.LayerBuffers(m) for m in maps]
    fin = dict(grad_scale=s_gs, dyn=dyn)
    if kind == "lars":
        fin.update(eeta=hp["eeta"], weight_decay=hp["wd"], epsilon=hp["eps"])
    code = LW.LAMB if kind == "lamb" else LW.LARS
    for lmap, buf in zip(maps, bufs):
        for ti in range(2):
            if kind == "lamb":
                LW.lamb_moments_(lmap, buf, ti, ws[ti], gs[ti], ms[ti], vs[ti], hp["b1"], hp["b2"], hp["eps"], s_gs,
                                 hp["wd"], dyn=dyn)
            else:
                LW.lars_norms_(lmap, buf, ti, ws[ti], gs[ti])
        LW.layer_finalize_(lmap, buf, code, mode=LW.REDUCE, **fin)
    total = bufs[0].sums + bufs[1].sums                  # what the all-reduce gives every rank
    for lmap, buf in zip(maps, bufs):
        buf.sums.copy_(total)
        LW.layer_finalize_(lmap, buf, code, mode=LW.COEF, **fin)
        for ti in range(2):
            if kind == "lamb":
                LW.lamb_apply_(lmap, buf, ti, ws[ti], ms[ti], vs[ti], shadows[ti], s_lr, hp["eps"], hp["wd"], dyn=dyn)
            else:
                LW.lars_apply_(lmap, buf, ti, ws[ti], gs[ti], accs[ti], shadows[ti], s_lr, hp["momentum"], s_gs,
                               hp["wd"], False, dyn=dyn)
    assert torch.equal(bufs[0].ratio, bufs[1].ratio)
    return dict(w=ws, m=ms, v=vs, acc=accs, shadow=shadows, ratio=bufs[0].ratio.clone(), sums=total)


def _fp64(kind, pieces, state, lr, gscale):
    ws, gs, ms, vs, accs = [[x.cpu() for x in t] for t in state]
    if kind == "lamb":
        hp = LH.LAMB_HP
        W, M, Vv, sums, ratios = LH.lamb_fp64(pieces, _GPU_DECAY, ws, gs, ms, vs, lr, hp["b1"], hp["b2"], hp["eps"],
                                               gscale, hp["wd"])
        return dict(w=W, m=M, v=Vv, sums=sums, ratio=ratios)
    hp = LH.LARS_HP
    W, A, sums, ratios = LH.lars_fp64(pieces, _GPU_DECAY, ws, gs, accs, lr, hp["momentum"], gscale, hp["wd"],
                                      hp["eeta"], hp["eps"])
    return dict(w=W, acc=A, sums=sums, ratio=ratios)


@pytest.mark.gpu
@pytest.mark.parametrize("gscale", [1e-3, 1e3])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_gpu_kernels_match_fp64(kind, gscale):
    _gpu()
    lr, gs_arg = 0.1, 0.5
    pieces, sizes, state = _gpu_state(gscale)
    ref = _fp64(kind, pieces, state, lr, gs_arg)
    got = _gpu_run(kind, pieces, state, lr, gs_arg)
    lmap = got["lmap"]
    assert lmap.count[2] == 1 and lmap.count[3] == 2 and lmap.count[4] == 257 and lmap.num_items == 257 + 6 + 1 + 2
    sums = got["sums"].view(-1, 2).tolist()
    ratio = got["ratio"].tolist()
    for l in range(len(_GPU_DECAY)):
        for a, b in zip(sums[l], ref["sums"][l]):
            assert abs(a - b) <= _RTOL * b, (l, a, b)
        assert abs(ratio[l] - ref["ratio"][l]) <= _RTOL * ref["ratio"][l], (l, ratio[l], ref["ratio"][l])
    assert ratio[5] == 1.0
    decayed = [r for r, d in zip(ref["ratio"], _GPU_DECAY) if d]
    if kind == "lamb":
        assert all(b / a > 2 for a, b in zip(decayed[:5], decayed[1:5])), decayed   # neighbours differ ~3x
    for key in ("w", "m", "v") if kind == "lamb" else ("w", "acc"):
        for ti in range(2):
            assert _rel(got[key][ti], ref[key][ti]) < 1e-6, (key, ti)
            # per layer too: a ratio taken from the wrong layer moves w by tens of percent
            for o, n, l in pieces[ti]:
                assert _rel(got[key][ti][o:o + n], ref[key][ti][o:o + n]) < 1e-6, (key, ti, l)
    for ti in range(2):
        assert _rel(got["shadow"][ti], ref["w"][ti]) < 1e-2
        assert not torch.equal(got["w"][ti], state[0][ti])
        # padding elements (the last 4 of every piece) are still exactly zero, in every buffer
        for o, n, _ in pieces[ti]:
            for key in ("w", "m", "v", "acc", "shadow"):
                assert not got[key][ti][o + n - 4:o + n].any(), (key, ti, o)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_gpu_split_finalize(kind):
    """"Rank 0 of 2" and "rank 1 of 2" piece lists over the same buffers, the 4160 layer cut in the middle: reduce
    only on both, sums added on the device, then the coefficient half.  The unsplit run over the same items (the
    4160 layer as two adjacent pieces, so the split points are item boundaries) gives bitwise the same ratios and
    weights; the one-piece run agrees within the fp32 tolerance."""
    _gpu()
    lr, gs_arg = 0.1, 0.5
    pieces, sizes, state = _gpu_state(1.0)
    both, _ = _gpu_layout("both")
    whole = _gpu_run(kind, both, state, lr, gs_arg)
    split = _gpu_run(kind, both, state, lr, gs_arg, split_lists=[_gpu_layout(0)[0], _gpu_layout(1)[0]])
    assert torch.equal(split["ratio"].view(torch.int32), whole["ratio"].view(torch.int32))
    assert torch.equal(split["sums"], whole["sums"])
    for key in ("w", "m", "v", "acc", "shadow"):
        for ti in range(2):
            assert torch.equal(split[key][ti], whole[key][ti]), (key, ti)
    one = _gpu_run(kind, pieces, state, lr, gs_arg)
    for a, b in zip(split["ratio"].tolist(), one["ratio"].tolist()):
        assert abs(a - b) <= 2 * _RTOL * b
    for ti in range(2):
        assert _rel(split["w"][ti], one["w"][ti]) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_gpu_repeatable_bitwise(kind):
    _gpu()
    pieces, sizes, state = _gpu_state(1.0, seed=12)
    a = _gpu_run(kind, pieces, state, 0.1, 0.5)
    b = _gpu_run(kind, pieces, state, 0.1, 0.5)
    assert torch.equal(a["partials"].view(torch.int32), b["partials"].view(torch.int32))
    assert torch.equal(a["sums"], b["sums"]) and torch.equal(a["ratio"].view(torch.int32), b["ratio"].view(torch.int32))
    for key in ("w", "m", "v", "acc", "shadow"):
        for ti in range(2):
            assert torch.equal(a[key][ti], b[key][ti]), (key, ti)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_gpu_dyn_overrides_scalars(kind):
    _gpu()
    pieces, sizes, state = _gpu_state(1.0, seed=13)
    want = _gpu_run(kind, pieces, state, 0.1, 0.5)
    dyn = torch.tensor([0.1, 123.0, 0.5], dtype=torch.float32, device="cuda")
    got = _gpu_run(kind, pieces, state, 0.1, 0.5, dyn=dyn, scalars=(9.0, 7.0))
    assert torch.equal(got["ratio"], want["ratio"])
    for key in ("w", "m", "v", "acc", "shadow"):
        for ti in range(2):
            assert torch.equal(got[key][ti], want[key][ti]), (key, ti)
    with pytest.raises(ValueError):
        lmap = want["lmap"]
        LW.lars_norms_(lmap, LW.LayerBuffers(lmap), 0, state[0][0][:64], state[1][0][:64])     # buffer too short


def _tinyres_run(batches, kind, clip_norm=None, hip_graph=False, mode="allreduce", probe=False):
    """The _TinyRes model of tests/test_hip_graph.py (bf16) under LAMB / LARS with a step-dependent LR."""
    from test_hip_graph import _TinyRes
    from mdtf.models import SoftmaxCrossEntropyLoss
    from mdtf.runtime import Model, Net, Tower
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device = torch.device("cuda")
    store.compute_dtype = torch.bfloat16
    store.generator.manual_seed(7)
    x0, _ = batches[0]
    xp = mdtf.placeholder(torch.float32, [None] + list(x0.shape[1:]))
    yp = mdtf.placeholder(torch.int64, [None])
    if kind == "lamb":
        base = LH.make_optimizer("lamb", clip_norm, lr=lambda step: 2e-3 / (1 + 0.5 * step))
    else:
        base = LH.make_optimizer("lars", clip_norm, lr=lambda step: 0.5 / (1 + step))
    tg = []
    M = type("TinyResModel", (_TinyRes, Model), {})
    t = Tower(Net(M()), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), base, batch_size=x0.shape[0])
    _, loss, _ = t.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, hip_graph=hip_graph, mode=mode, bucket_bytes=1 << 18)
    gv = Tower.average_gradients(tg)
    gnorm = mdtf.train.global_norm([g for g, _ in gv]) if probe else None
    op = opt.apply_gradients(gv, global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    losses, ratios, norms = [], [], []
    for x, y in batches:
        if probe:
            _, lv, n = sess.run([op, loss, gnorm], feed_dict={xp: x, yp: y})
            norms.append(n)
        else:
            _, lv = sess.run([op, loss], feed_dict={xp: x, yp: y})
        losses.append(lv)
        ratios.append(base.last_ratios.clone())
    losses, norms = [float(v) for v in losses], [float(n) for n in norms]
    coefs = [] if op.clip is None else None
    weights = {v.name: v.value().detach().float().cpu().clone() for v in store.trainable_variables()}
    return dict(losses=losses, ratios=[r.cpu() for r in ratios], weights=weights, op=op, norms=norms, coefs=coefs)


def _assert_same_run(e, g):
    assert e["losses"] == g["losses"], (e["losses"], g["losses"])
    for a, b in zip(e["ratios"], g["ratios"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for k in e["weights"]:
        assert torch.equal(e["weights"][k], g["weights"][k]), k
    # per-step ratios do not repeat from step to step (no stale replayed value)
    for a, b in zip(g["ratios"], g["ratios"][1:]):
        assert not torch.equal(a, b)
    assert all(torch.isfinite(r).all() for r in g["ratios"]) and any((r != 1).any() for r in g["ratios"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_gpu_graph_replay_equals_eager(kind):
    _gpu()
    from mdtf.ops import _native
    torch.manual_seed(0)
    batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(6)]
    _native.set_deterministic(True)
    try:
        clip = None
        if kind == "lamb":                  # LAMB runs with global_clipnorm (BERT's recipe), LARS without
            probe = _tinyres_run(batches, kind, probe=True)
            clip = 0.5 * (min(probe["norms"]) + max(probe["norms"]))
        e = _tinyres_run(batches, kind, clip, hip_graph=False)
        g = _tinyres_run(batches, kind, clip, hip_graph=True)
    finally:
        _native.set_deterministic(False)
    sg = g["op"].graph
    assert sg is not None and sg.graph is not None and sg.replays == 4 and sg.fallbacks == 0, vars(sg)
    assert e["op"].graph is None
    assert (g["op"].clip is not None) == (kind == "lamb")
    _assert_same_run(e, g)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_gpu_graph_captures_lamb_with_rccl(mode, monkeypatch):
    """A 1-rank nccl group with collectives forced on (as test_gpu_graph_captures_clip_with_rccl): the LAMB step
    captures and replays and equals eager; in sharded mode the fp64 ``sums`` all-reduce is inside the capture."""
    _gpu()
    import socket
    import torch.distributed as dist
    from mdtf.ops import _native
    from mdtf.parallel import reducer as R
    from mdtf.train import step as S
    monkeypatch.setenv("MDTF_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("TORCH_FR_BUFFER_SIZE", "2000")
    monkeypatch.setenv("NCCL_DEBUG", os.environ.get("NCCL_DEBUG", "WARN"))
    calls = []
    orig = R.GradReducer.all_reduce_sum

    def counted(self, t):
        calls.append((t.dtype, t.numel(), torch.cuda.is_current_stream_capturing()))
        return orig(self, t)
    monkeypatch.setattr(R.GradReducer, "all_reduce_sum", counted)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(5)]
        _native.set_deterministic(True)
        try:
            e = _tinyres_run(batches, "lamb", hip_graph=False, mode=mode)
            eager_calls = list(calls)
            del calls[:]
            g = _tinyres_run(batches, "lamb", hip_graph=True, mode=mode)
        finally:
            _native.set_deterministic(False)
        assert e["op"].reducer.collective and g["op"].reducer.collective
        assert g["op"].graph.replays == 3 and g["op"].graph.fallbacks == 0
        nl = g["op"]._layer_map.num_layers
        if mode == "sharded":
            assert len(eager_calls) == 5 and not any(c[2] for c in eager_calls)
            assert [c[2] for c in calls] == [False, False, True], calls
            assert all(c[0] == torch.float64 and c[1] == 2 * nl for c in calls)
        else:
            assert calls == [] and eager_calls == []
        _assert_same_run(e, g)
    finally:
        S.release_graphs()                 # the captured RCCL collectives go before their communicator
        dist.destroy_process_group()
