"""Device-side global-norm gradient clipping (``mdtf.train.clip_by_global_norm`` / ``global_norm`` /
``global_clipnorm=``), ``csrc/gradnorm.hip`` and ``mdtf.train.polynomial_decay``.

norm = grad_scale * sqrt(sum of squares of the reduced gradient), coef = clip_norm / max(norm, clip_norm); the
fused update kernels apply grad_scale * coef.  CPU tests run the PyTorch reference path, GPU tests the HIP kernels.
"""
import json
import math
import os
import sys
import types

import pytest
import torch

import mdtf
from mdtf.ops import gradnorm as GN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_helpers as CH  # noqa: E402


def _norm_clip(grads, clip_norm, lr=0.05, lr_t=0.04, gs=0.3, dyn=None, split=False):
    buf = GN.NormBuffers(grads)
    GN.grad_sumsq_(grads, buf)
    if split:
        GN.clip_finalize_(buf, clip_norm, lr, lr_t, gs, dyn=dyn, mode=GN.REDUCE)
        GN.clip_finalize_(buf, clip_norm, lr, lr_t, gs, dyn=dyn, mode=GN.COEF)
    else:
        GN.clip_finalize_(buf, clip_norm, lr, lr_t, gs, dyn=dyn)
    return buf


def _formula(grads, clip_norm, gs):
    """The explicit fp64 formula: (norm, coef)."""
    ss = sum(float(g.double().pow(2).sum()) for g in grads)
    norm = gs * math.sqrt(ss)
    if clip_norm <= 0:
        return norm, 1.0
    if not math.isfinite(norm):
        return norm, float("nan")
    return norm, clip_norm / max(norm, clip_norm)


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("nseg", [1, 3])
def test_reference_path_math(nseg):
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(n, generator=g) for n in (64, 192, 1024)[:nseg]]
    gs = 0.3
    norm, _ = _formula(grads, 0.0, gs)
    # norm < clip: coef exactly 1, effective scale bitwise the input scale
    buf = _norm_clip(grads, 2.0 * norm, gs=gs)
    assert float(buf.stats[1]) == 1.0
    assert torch.equal(buf.eff, torch.tensor([0.05, 0.04, gs], dtype=torch.float32))
    assert float(buf.stats[0]) == pytest.approx(norm, rel=1e-6)
    # norm > clip
    clip = 0.25 * norm
    for split in (False, True):
        buf = _norm_clip(grads, clip, gs=gs, split=split)
        want_norm, want_coef = _formula(grads, clip, gs)
        assert want_coef < 1
        assert float(buf.stats[0]) == pytest.approx(want_norm, rel=1e-6)
        assert float(buf.stats[1]) == pytest.approx(want_coef, rel=1e-6)
        assert float(buf.eff[2]) == pytest.approx(gs * want_coef, rel=1e-6)
        assert torch.equal(buf.eff[:2], torch.tensor([0.05, 0.04], dtype=torch.float32))
    # all-zero gradient: coef 1, nothing NaN
    buf = _norm_clip([torch.zeros_like(x) for x in grads], 1.0, gs=gs)
    assert float(buf.stats[0]) == 0.0 and float(buf.stats[1]) == 1.0
    assert torch.equal(buf.eff[2], _f32(gs)) and not torch.isnan(buf.eff).any()
    # one inf / one nan element: coef NaN (every update turns NaN)
    for bad in (float("inf"), float("nan")):
        gb = [x.clone() for x in grads]
        gb[-1][5] = bad
        buf = _norm_clip(gb, 1.0, gs=gs)
        assert math.isnan(float(buf.stats[1])) and math.isnan(float(buf.eff[2])), bad
        assert not math.isfinite(float(buf.stats[0]))
    # clip_norm = 0: norm only
    buf = _norm_clip(grads, 0.0, gs=gs)
    assert float(buf.stats[1]) == 1.0 and torch.equal(buf.eff[2], _f32(gs))
    assert float(buf.stats[0]) == pytest.approx(norm, rel=1e-6)
    # a dyn base overrides the scalar arguments
    buf = _norm_clip(grads, clip, lr=9.0, lr_t=9.0, gs=9.0, dyn=torch.tensor([0.05, 0.04, gs]))
    assert float(buf.stats[0]) == pytest.approx(norm, rel=1e-6)
    assert torch.equal(buf.eff[:2], torch.tensor([0.05, 0.04], dtype=torch.float32))


def _setup(batch=8):
    Lin, MSE, xs, ys, x_ph, y_ph = CH.linear_setup(1, batch)
    return Lin, MSE, xs, ys, x_ph, y_ph


def test_handle_api():
    from mdtf.runtime import Net, Tower
    from mdtf.train import step as S
    Lin, MSE, xs, ys, x_ph, y_ph = _setup()
    opt = mdtf.train.MomentumOptimizer(0.1, 0.9)
    tg = []
    tower = Tower(Net(Lin()), "tower_0/", tg, x_ph, y_ph, MSE(), opt, batch_size=8)
    _, loss, _ = tower.process()
    # the canonical TF1 flow
    gv = opt.compute_gradients(loss)
    grads, vs = zip(*gv)
    clipped, gnorm = mdtf.train.clip_by_global_norm(grads, 1.0)
    assert mdtf.clip_by_global_norm is mdtf.train.clip_by_global_norm and mdtf.global_norm is mdtf.train.global_norm
    assert [c.var for c in clipped] == list(vs) and all(c.program is g.program for c, g in zip(clipped, grads))
    assert len({id(c.clip) for c in clipped}) == 1
    train_op = opt.apply_gradients(zip(clipped, vs), mdtf.train.get_or_create_global_step())
    assert isinstance(train_op, S.TrainOp) and train_op.clip is clipped[0].clip and train_op.clip.clip_norm == 1.0
    assert isinstance(gnorm, S.Fetchable)
    # partially clipped
    with pytest.raises(ValueError):
        opt.apply_gradients([(clipped[0], vs[0])] + list(zip(grads[1:], vs[1:])))
    # two clip calls mixed
    other, _ = mdtf.train.clip_by_global_norm(grads, 2.0)
    with pytest.raises(ValueError):
        opt.apply_gradients([(clipped[0], vs[0])] + list(zip(other[1:], vs[1:])))
    with pytest.raises(ValueError):
        mdtf.train.SyncReplicasOptimizer(opt).apply_gradients([(clipped[0], vs[0])] + list(zip(other[1:], vs[1:])))
    # the norm belongs to a training step: fetching it without the train op raises
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    with pytest.raises(RuntimeError):
        sess.run(gnorm, feed_dict={x_ph: xs, y_ph: ys})
    _, lv, n = sess.run([train_op, loss, gnorm], feed_dict={x_ph: xs, y_ph: ys})
    assert isinstance(n, float) and n > 0 and lv == lv
    assert float(opt.last_global_norm[0]) == n and train_op.last_global_norm is opt.last_global_norm
    # the keyword reaches every optimizer, and through SyncReplicasOptimizer the wrapped one
    for cls in (mdtf.train.GradientDescentOptimizer, mdtf.train.MomentumOptimizer, mdtf.train.AdamOptimizer,
                mdtf.train.AdamWeightDecayOptimizer):
        o = cls(0.1, global_clipnorm=1.5)
        assert o.global_clipnorm == 1.5 and cls(0.1).global_clipnorm is None
        assert mdtf.train.SyncReplicasOptimizer(o).global_clipnorm == 1.5
    base = mdtf.train.AdamOptimizer(0.1)
    assert mdtf.train.SyncReplicasOptimizer(base, global_clipnorm=0.5).global_clipnorm == 0.5
    assert base.global_clipnorm == 0.5
    assert mdtf.FLAGS.clip_norm == 0.0


def _train(how, clip_norm, steps, xs, ys):
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    Lin, MSE, _, _, x_ph, y_ph = CH.linear_setup(1, xs.shape[0])
    op, loss, gnorm, opt = CH.build_train(xs, x_ph, y_ph, Lin, MSE, clip_norm, how, xs.shape[0])
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    norms = []
    for _ in range(steps):
        if gnorm is not None:
            _, n = sess.run([op, gnorm], feed_dict={x_ph: xs, y_ph: ys})
            norms.append(n)
        else:
            sess.run(op, feed_dict={x_ph: xs, y_ph: ys})
            if op.last_global_norm is not None:
                norms.append(float(op.last_global_norm[0]))
    w = {mdtf.runtime.tower.strip_tower_prefix(v.name): v.master.detach().clone()
         for v in V.get_store().trainable_variables()}
    return w, norms, op


def test_end_to_end_matches_plain_torch():
    _, _, xs, ys, _, _ = _setup()
    steps = 5
    clip = CH.clip_between(xs, ys, steps)
    w_ref, n_ref = CH.torch_reference(xs, ys, steps, clip)
    assert any(n > clip for n in n_ref) and any(n <= clip for n in n_ref), (clip, n_ref)   # both branches taken
    w, norms, op = _train("call", clip, steps, xs, ys)
    assert op.clip is not None and op.reducer.eager_update is None
    assert norms == pytest.approx(n_ref, rel=1e-6)
    for name, ref in w_ref.items():
        assert torch.allclose(w[name], ref, atol=1e-6, rtol=0), name
    # and the clip did something: the unclipped run ends elsewhere
    w_un, _ = CH.torch_reference(xs, ys, steps, None)
    assert not torch.allclose(w["dense/w"], w_un["dense/w"], atol=1e-4, rtol=0)


def test_keyword_equals_explicit_call_bitwise():
    _, _, xs, ys, _, _ = _setup()
    clip = CH.clip_between(xs, ys, 5)
    w_call, n_call, _ = _train("call", clip, 5, xs, ys)
    w_kw, n_kw, op = _train("keyword", clip, 5, xs, ys)
    assert op.clip is not None and op.clip.clip_norm == clip
    assert n_call == n_kw and len(n_kw) == 5
    for name in w_call:
        assert torch.equal(w_call[name], w_kw[name]), name
    # no clip requested: no norm machinery at all
    _, n_none, op = _train(None, None, 2, xs, ys)
    assert op.clip is None and op._norm_buf is None and n_none == []


def test_norm_over_raw_buffers_equals_norm_over_variables():
    """Alignment gaps, pad_rows and bucket padding of the flat buffers are zero, so the sum over the raw buffers is
    the sum over the variables (3, 65, 1000 elements and one variable with pad_rows)."""
    from mdtf.runtime import Loss, Model, Net, Tower
    from mdtf.train import variables as V

    class Odd(Model):
        def inference(self, x):
            a = V.get_variable("a", [3], initializer=V.constant_initializer(0.3))
            b = V.get_variable("b", [65], initializer=V.constant_initializer(0.05))
            c = V.get_variable("c", [10, 100], initializer=V.constant_initializer(0.01))
            e = V.get_variable("e", [5, 8], initializer=V.constant_initializer(0.2))
            V.find_variable("e").pad_rows = 3
            y = (x @ e.t()).sum(1, keepdim=True) + (a * x[:, :3]).sum(1, keepdim=True)
            return y + (b * b).sum() * x[:, 3:4] + (c.sum(0)[:8] * x).sum(1, keepdim=True)

    class MSE(Loss):
        def loss(self, p, t):
            return ((p - t) ** 2).mean()

    g = torch.Generator().manual_seed(1)
    xs, ys = torch.randn(6, 8, generator=g), torch.randn(6, 1, generator=g)
    x_ph = mdtf.placeholder(torch.float32, [None, 8])
    y_ph = mdtf.placeholder(torch.float32, [None, 1])
    opt = mdtf.train.GradientDescentOptimizer(0.01)
    tg = []
    Tower(Net(Odd()), "tower_0/", tg, x_ph, y_ph, MSE(), opt, batch_size=6).process()
    gv = Tower.average_gradients(tg)
    gnorm = mdtf.train.global_norm([gr for gr, _ in gv])
    op = opt.apply_gradients(gv, global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    _, n = sess.run([op, gnorm], feed_dict={x_ph: xs, y_ph: ys})
    vs = V.get_store().trainable_variables()
    assert sorted(v.numel() for v in vs) == [3, 40, 65, 1000]
    assert any(int(getattr(v, "pad_rows", 0) or 0) == 3 for v in vs)
    per_var = sum(float(v.grad.double().pow(2).sum()) for v in vs)
    raw = sum(float(gr.grad.double().pow(2).sum()) for gr in op.space.groups)
    assert sum(gr.numel for gr in op.space.groups) > sum(v.numel() for v in vs)          # there IS padding
    assert sum(int((gr.grad != 0).sum()) for gr in op.space.groups) == sum(int((v.grad != 0).sum()) for v in vs)
    assert all(int((v.grad != 0).sum()) > 0 for v in vs)
    assert raw == pytest.approx(per_var, rel=1e-12)
    assert n == pytest.approx(math.sqrt(per_var), rel=1e-6)


@pytest.mark.slow
@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_two_rank_gloo_clipped_training(mode, tmp_path):
    import torch.multiprocessing as mp
    from mdtf.cluster.launcher import free_port
    world, steps, batch = 2, 5, 4
    _, _, xs, ys, _, _ = CH.linear_setup(world, batch)
    clip = CH.clip_between(xs, ys, steps)
    w_ref, n_ref = CH.torch_reference(xs, ys, steps, clip)
    assert any(n > clip for n in n_ref) and any(n <= clip for n in n_ref)
    mp.start_processes(CH.clip_worker, args=(world, free_port(), mode, steps, str(tmp_path), clip, batch),
                       nprocs=world, join=True, start_method="spawn")
    res = [json.load(open(os.path.join(str(tmp_path), "rank%d.json" % r))) for r in range(world)]
    assert res[0]["collective"]
    assert res[0]["norms"] == res[1]["norms"] and len(res[0]["norms"]) == steps        # bitwise (hex floats)
    assert res[0]["coefs"] == res[1]["coefs"]
    assert any(float.fromhex(c) < 1 for c in res[0]["coefs"]) and any(float.fromhex(c) == 1 for c in res[0]["coefs"])
    assert [float.fromhex(n) for n in res[0]["norms"]] == pytest.approx(n_ref, rel=1e-5)
    for r in res:
        for name, ref in w_ref.items():
            got = torch.tensor(r["weights"]["tower_0/" + name] if "tower_0/" + name in r["weights"]
                               else r["weights"][name])
            assert torch.allclose(got, ref, atol=1e-5, rtol=0), (mode, name)


def test_async_ps_with_clip_is_not_implemented():
    from mdtf.parallel.async_ps import AsyncWorker
    from mdtf.train import step as S
    runner = types.SimpleNamespace(optimizer=mdtf.train.MomentumOptimizer(0.1, 0.9, global_clipnorm=1.0))
    with pytest.raises(NotImplementedError, match="ps_mode"):
        AsyncWorker(runner, None, None, [], 10)
    plain = types.SimpleNamespace(optimizer=mdtf.train.MomentumOptimizer(0.1, 0.9))
    var = types.SimpleNamespace(name="v")
    clipped, _ = mdtf.train.clip_by_global_norm([S.GradRef(var)], 1.0)
    with pytest.raises(NotImplementedError, match="ps_mode"):
        AsyncWorker(plain, None, None, [(clipped[0], var)], 10, sync=True)


def test_polynomial_decay_closed_form():
    lr0, end, decay, warm, power = 1e-4, 1e-6, 1000, 100, 2.0
    f = mdtf.train.polynomial_decay(lr0, decay, end_learning_rate=end, power=power, warmup_steps=warm)

    def closed(step):
        if step < warm:
            return lr0 * step / warm
        return (lr0 - end) * (1 - min(step, decay) / decay) ** power + end
    for step in (0, 37, warm, 550, decay, decay + 500):
        assert f(step) == pytest.approx(closed(step), rel=1e-12, abs=0), step
    assert f(0) == 0.0 and f(50) == pytest.approx(0.5 * lr0)
    assert f(decay) == pytest.approx(end) and f(10 * decay) == pytest.approx(end)
    g = mdtf.train.polynomial_decay(0.5, 10)                       # defaults: linear to 0, no warm-up
    assert g(0) == 0.5 and g(5) == pytest.approx(0.25) and g(10) == 0.0
    opt = mdtf.train.AdamWeightDecayOptimizer(f, global_clipnorm=1.0)
    assert opt.learning_rate(550) == pytest.approx(closed(550))


# ------------------------------------------------------------------------------------------------------ GPU
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mdtf.ops import _native
    _native.lib()


# sizes: less than one wave of float4s | ragged last block | many blocks | above the grid cap (blocks loop over
# chunks: 2049 chunks of 4096 elements on 2048 blocks -> 2 chunks per block)
_SIZES = [64, 4160, (1 << 20) + 64, (1 << 23) + 64]
# fp32 sum of k non-negative terms: relative error <= k * 2^-24.  k for the largest size: 2 chunks x 4 float4 x 4
# = 32 per-thread terms + 6 wave-shuffle levels + 2 LDS levels = 40 (the cross-block sum is fp64); doubled for
# margin, halved by the square root: 40 * 2^-24
_K = 40
_RTOL = _K * 2.0 ** -24


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_gpu_kernel_matches_fp64(scale):
    _gpu()
    g = torch.Generator(device="cuda").manual_seed(5)
    bufs = [torch.randn(n, device="cuda", generator=g) * scale for n in _SIZES]
    assert GN.num_partials([bufs[-1]]) < math.ceil(_SIZES[-1] / 4096)          # the largest size loops
    cases = [[b] for b in bufs] + [bufs[:3], [bufs[3], bufs[0], bufs[1]]]
    for grads in cases:
        want = math.sqrt(sum(float(b.double().pow(2).sum()) for b in grads))
        buf = _norm_clip(grads, 0.0, gs=1.0)
        got = float(buf.stats[0])
        assert abs(got - want) <= _RTOL * want, ([b.numel() for b in grads], got, want)
        clip = 0.5 * want
        buf = _norm_clip(grads, clip, gs=1.0, split=True)
        assert float(buf.stats[1]) == pytest.approx(0.5, rel=4 * _RTOL)


@pytest.mark.gpu
def test_gpu_repeatable_bitwise():
    _gpu()
    from mdtf.ops import _native
    assert not _native.deterministic()
    g = torch.Generator(device="cuda").manual_seed(6)
    grads = [torch.randn(n, device="cuda", generator=g) for n in ((1 << 20) + 64, 4160, (1 << 23) + 64)]
    a = _norm_clip(grads, 1.0)
    b = _norm_clip(grads, 1.0)
    assert torch.equal(a.stats, b.stats) and torch.equal(a.eff, b.eff) and torch.equal(a.partials, b.partials)
    assert torch.equal(a.stats.view(torch.int32), b.stats.view(torch.int32))


@pytest.mark.gpu
def test_gpu_edge_values():
    _gpu()
    g = torch.Generator(device="cuda").manual_seed(7)
    grads = [torch.randn(4160, device="cuda", generator=g), torch.randn(64, device="cuda", generator=g)]
    gs = 0.3
    norm, _ = _formula(grads, 0.0, gs)
    buf = _norm_clip(grads, 2.0 * norm, gs=gs)
    assert float(buf.stats[1]) == 1.0
    assert torch.equal(buf.eff.cpu(), torch.tensor([0.05, 0.04, gs], dtype=torch.float32))
    buf = _norm_clip(grads, 0.25 * norm, gs=gs)
    assert float(buf.stats[1]) == pytest.approx(0.25, rel=1e-5)
    assert float(buf.eff[2]) == pytest.approx(gs * 0.25, rel=1e-5)
    for bad in (float("inf"), float("nan")):
        gb = [x.clone() for x in grads]
        gb[0][4159] = bad
        buf = _norm_clip(gb, 1.0, gs=gs)
        assert math.isnan(float(buf.stats[1])) and math.isnan(float(buf.eff[2])), bad
    buf = _norm_clip([torch.zeros_like(x) for x in grads], 1.0, gs=gs)
    assert float(buf.stats[0]) == 0.0 and float(buf.stats[1]) == 1.0
    assert torch.equal(buf.eff[2].cpu(), _f32(gs))
    # a base dyn pointer overrides the scalar arguments
    dyn = torch.tensor([0.05, 0.04, gs], dtype=torch.float32, device="cuda")
    buf = _norm_clip(grads, 0.25 * norm, lr=9.0, lr_t=8.0, gs=7.0, dyn=dyn)
    assert float(buf.stats[0]) == pytest.approx(norm, rel=1e-5)
    assert torch.equal(buf.eff[:2].cpu(), torch.tensor([0.05, 0.04], dtype=torch.float32))
    assert float(buf.eff[2]) == pytest.approx(gs * 0.25, rel=1e-5)
    with pytest.raises(ValueError):
        GN.num_partials([torch.zeros(66, device="cuda")])


def _tinyres_run(batches, how, clip_norm=None, opt_kind="sgd", hip_graph=False, mode="allreduce", lr=1e-2):
    """The _TinyRes model of tests/test_hip_graph.py (bf16).  Returns losses, norms, weights, the op."""
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
    kw = dict(global_clipnorm=clip_norm) if how == "keyword" else {}
    if opt_kind == "sgd":
        base = mdtf.train.GradientDescentOptimizer(lr, **kw)
    elif opt_kind == "momentum":
        base = mdtf.train.MomentumOptimizer(lambda step: 0.05 / (1 + step), 0.9, weight_decay=1e-4, **kw)
    else:
        base = mdtf.train.AdamOptimizer(lambda step: 1e-3 / (1 + 0.5 * step), **kw)
    tg = []
    M = type("TinyResModel", (_TinyRes, Model), {})
    t = Tower(Net(M()), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), base, batch_size=x0.shape[0])
    _, loss, _ = t.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, hip_graph=hip_graph, mode=mode, bucket_bytes=1 << 18)
    gv = Tower.average_gradients(tg)
    if how == "call":
        grads, vs = zip(*gv)
        clipped, gnorm = mdtf.train.clip_by_global_norm(grads, clip_norm)
        gv = list(zip(clipped, vs))
    else:
        gnorm = mdtf.train.global_norm([g for g, _ in gv])
    op = opt.apply_gradients(gv, global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    before = {v.name: v.master.detach().clone() for v in store.trainable_variables()}
    losses, norms, coefs = [], [], []
    for x, y in batches:
        _, lv, n = sess.run([op, loss, gnorm], feed_dict={xp: x, yp: y})
        losses.append(lv)
        norms.append(n)
        coefs.append(op.last_global_norm[1].clone())
    assert all(isinstance(n, torch.Tensor) and n.is_cuda and n.dim() == 0 for n in norms)
    losses, norms, coefs = [float(v) for v in losses], [float(v) for v in norms], [float(v) for v in coefs]
    weights = {v.name: v.value().detach().float().cpu().clone() for v in store.trainable_variables()}
    delta = math.sqrt(sum(float((v.master.detach().double() - before[v.name].double()).pow(2).sum())
                          for v in store.trainable_variables()))
    return dict(losses=losses, norms=norms, coefs=coefs, weights=weights, op=op, delta=delta)


@pytest.mark.gpu
def test_gpu_step_moves_masters_by_lr_times_clip_norm():
    """SGD without decay: ||delta master|| = lr * min(norm, clip_norm).  No clip, a clip applied twice or the norm
    of the unscaled sum would be off by a factor of two or more."""
    _gpu()
    torch.manual_seed(0)
    batch = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,)))]
    lr = 1e-2
    first = _tinyres_run(batch, "norm", lr=lr)
    norm = first["norms"][0]
    assert norm > 0 and first["coefs"] == [1.0]
    assert first["delta"] == pytest.approx(lr * norm, rel=1e-3)
    clip = 0.5 * norm
    second = _tinyres_run(batch, "call", clip, lr=lr)
    assert second["norms"][0] == pytest.approx(norm, rel=1e-5)
    assert second["coefs"][0] == pytest.approx(0.5, rel=1e-5)
    assert second["delta"] == pytest.approx(lr * clip, rel=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("opt_kind", ["momentum", "adam"])
def test_gpu_graph_replay_equals_eager_with_clip(opt_kind):
    _gpu()
    from mdtf.ops import _native
    torch.manual_seed(0)
    batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(6)]
    _native.set_deterministic(True)
    try:
        probe = _tinyres_run(batches, "norm", opt_kind=opt_kind)
        clip = 0.5 * (min(probe["norms"]) + max(probe["norms"]))
        e = _tinyres_run(batches, "keyword", clip, opt_kind=opt_kind, hip_graph=False)
        g = _tinyres_run(batches, "keyword", clip, opt_kind=opt_kind, hip_graph=True)
    finally:
        _native.set_deterministic(False)
    sg = g["op"].graph
    assert sg is not None and sg.graph is not None and sg.replays == 4 and sg.fallbacks == 0, vars(sg)
    assert e["op"].graph is None
    assert e["losses"] == g["losses"], (e["losses"], g["losses"])
    assert e["norms"] == g["norms"], (e["norms"], g["norms"])
    assert e["coefs"] == g["coefs"]
    assert len(set(g["norms"])) == len(g["norms"])                  # no stale replayed scalar
    assert any(c < 1 for c in g["coefs"]), g["coefs"]
    for k in e["weights"]:
        assert torch.equal(e["weights"][k], g["weights"][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_gpu_graph_captures_clip_with_rccl(mode, monkeypatch):
    """A 1-rank nccl group with collectives forced on (as test_hip_graph_captures_rccl_collectives): eager ==
    replay with the clip on; in sharded mode the fp64 sum-of-squares all-reduce is inside the capture."""
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
            probe = _tinyres_run(batches[:2], "norm", opt_kind="momentum", mode=mode)
            clip = 0.5 * max(probe["norms"])
            del calls[:]
            e = _tinyres_run(batches, "keyword", clip, opt_kind="momentum", hip_graph=False, mode=mode)
            eager_calls = list(calls)
            del calls[:]
            g = _tinyres_run(batches, "keyword", clip, opt_kind="momentum", hip_graph=True, mode=mode)
        finally:
            _native.set_deterministic(False)
        assert e["op"].reducer.collective and g["op"].reducer.collective
        assert g["op"].graph.replays == 3 and g["op"].graph.fallbacks == 0
        if mode == "sharded":
            assert len(eager_calls) == 5 and not any(c[2] for c in eager_calls)
            # two warm-up steps eagerly, then ONE call while capturing; replays run no Python of the step
            assert [c[2] for c in calls] == [False, False, True], calls
            assert all(c[0] == torch.float64 and c[1] == 1 for c in calls)
        else:
            assert calls == [] and eager_calls == []
        assert e["losses"] == g["losses"] and e["norms"] == g["norms"] and e["coefs"] == g["coefs"]
        assert any(c < 1 for c in g["coefs"])
        for k in e["weights"]:
            assert torch.equal(e["weights"][k], g["weights"][k]), k
    finally:
        S.release_graphs()                 # the captured RCCL collectives go before their communicator
        dist.destroy_process_group()
