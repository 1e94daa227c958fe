"""``mdtf.train.ExponentialMovingAverage``: the update kernel (``mdtf.ops.ema`` / ``csrc/ema.hip``) against an
independent fp64 reference, element by element, and the average through the train op, checkpoints, the run loop,
gloo replicas and hipGraph replay.

Kernel tests take a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.ema`` (the bound of ``ema_helpers`` must
hold for it too), ``cuda`` the HIP kernel.  Tensors are slices [4 : 4 + n] of sentinel-filled buffers.
"""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import mdtf
from mdtf.ops import ema as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_helpers as EH  # noqa: E402
import optim_helpers as OH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]

# one block owns E.CHUNK = 4 * 256 threads * 4 float4s consecutive elements and the grid is not capped (no second
# trip).  4: one float4, one thread | 64: a wave is not filled | CHUNK - 4, CHUNK, CHUNK + 4: the block's chunk short
# by one float4 (the ``i < n4`` guard of its last quarter), exactly full, and one float4 into a second block |
# 2 * CHUNK + 4 * 257: two full chunks and a third with a full first quarter and one float4 in its second
SIZES = [4, 64, E.CHUNK - 4, E.CHUNK, E.CHUNK + 4, 2 * E.CHUNK + 4 * 257]
N = 2 * E.CHUNK + 4 * 257
K = EH.K_EMA


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from mdtf.ops import _native
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _inputs(n, seed, k=1):
    """w (k of them, all different) and an ema of the same magnitude."""
    inp = OH.make_inputs(n, seed, k=k)
    gen = torch.Generator().manual_seed(seed + 1000)
    ema = torch.randn(n, generator=gen)
    ws = [inp["w"]] + [torch.randn(n, generator=gen) for _ in range(k - 1)]
    return ws, ema


class Bufs(object):
    def __init__(self, device, w, ema):
        self.w = OH.Guarded(w, device)
        self.ema = OH.Guarded(ema, device)

    def set_w(self, w):
        self.w.t.copy_(w)
        self.w.before = self.w.buf.clone()

    def assert_contained(self, what):
        assert self.ema.guards_intact(), "%s: wrote outside ema[0:n]" % what
        assert self.w.unchanged(), "%s: w modified" % what


# ------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_every_size_against_fp64(device, n):
    device = _device(device)
    (w,), ema = _inputs(n, n % 1000 + 1)
    omd = E.one_minus_decay(0.9)
    assert omd == OH.f32(omd)
    b = Bufs(device, w, ema)
    E.ema_update_(b.ema.t, b.w.t, omd)
    st = EH.ref_start(w, ema)
    EH.ref_step(st, w, omd)
    what = "%s/ema n=%d" % (device, n)
    b.assert_contained(what)
    OH.check(b.ema.t, st, "ema", K, what)
    assert not torch.equal(b.ema.t.cpu(), ema)


def test_chunk_constants_match_the_kernel_source():
    src = open(os.path.join(os.path.dirname(E.__file__), "..", "csrc", "ema.hip")).read()
    assert "constexpr int kThreads = %d;" % E.THREADS in src and "constexpr int kEmaVpt = %d;" % E.VPT in src
    assert E.CHUNK == 4 * E.THREADS * E.VPT and EH.VARIANT_N == N


@pytest.mark.parametrize("device", DEVICES)
def test_device_buffer_overrides_the_scalar(device):
    """A wrong scalar + the right buffer is bitwise the call with the right scalar; rewriting the buffer between
    two calls, no other argument changed, changes the decay of the second."""
    device = _device(device)
    (w,), ema = _inputs(N, 61)
    o1, o2 = E.one_minus_decay(0.9), E.one_minus_decay(0.75)
    want = Bufs(device, w, ema)
    E.ema_update_(want.ema.t, want.w.t, o1)
    want1 = want.ema.t.clone()
    E.ema_update_(want.ema.t, want.w.t, o2)
    got = Bufs(device, w, ema)
    dev = torch.tensor([o1], dtype=torch.float32, device=device)
    args = (got.ema.t, got.w.t, 0.77)
    E.ema_update_(*args, omd_dev=dev)
    got.assert_contained("omd_dev")
    assert OH.bits_equal(got.ema.t, want1)
    dev.fill_(o2)
    E.ema_update_(*args, omd_dev=dev)
    assert OH.bits_equal(got.ema.t, want.ema.t)
    assert dev.tolist() == [o2]
    # and the scalar alone does matter
    off = Bufs(device, w, ema)
    E.ema_update_(off.ema.t, off.w.t, 0.77)
    assert not torch.equal(off.ema.t, want1)


@pytest.mark.parametrize("device", DEVICES)
def test_omd_zero_keeps_ema(device):
    device = _device(device)
    (w,), ema = _inputs(N, 62)
    b = Bufs(device, w, ema)
    E.ema_update_(b.ema.t, b.w.t, 0.0)
    b.assert_contained("omd=0")
    assert OH.bits_equal(b.ema.t.cpu(), ema)
    dev = torch.zeros(1, device=device)
    E.ema_update_(b.ema.t, b.w.t, 0.5, omd_dev=dev)
    assert OH.bits_equal(b.ema.t.cpu(), ema)


@pytest.mark.parametrize("device", DEVICES)
def test_five_updates_carry_the_average(device):
    """Five updates with five decays and a new w each time, compared once under 5 * K."""
    device = _device(device)
    ws, ema = _inputs(N, 63, k=5)
    omds = [E.one_minus_decay(d) for d in (0.9, 0.999, 0.5, 0.9999, 0.0)]
    b = Bufs(device, ws[0], ema)
    st = EH.ref_start(ws[0], ema)
    for w, omd in zip(ws, omds):
        b.set_w(w)
        E.ema_update_(b.ema.t, b.w.t, omd)
        EH.ref_step(st, w, omd)
    b.assert_contained("x5")
    OH.check(b.ema.t, st, "ema", 5 * K, "%s/ema x5" % device)


@pytest.mark.parametrize("device", DEVICES)
def test_inf_and_nan_stay_in_their_elements(device):
    device = _device(device)
    n, bad = 64, {5: float("inf"), 18: float("nan")}
    (w,), ema = _inputs(n, 64)
    for i, x in bad.items():
        w[i] = x
    omd = E.one_minus_decay(0.9)
    b = Bufs(device, w, ema)
    E.ema_update_(b.ema.t, b.w.t, omd)
    st = EH.ref_start(w, ema)
    EH.ref_step(st, w, omd)
    assert torch.equal(b.w.buf.view(torch.int32), b.w.before.view(torch.int32))
    assert b.ema.guards_intact()
    OH.check(b.ema.t, st, "ema", K, "%s/ema special" % device)       # non-finite exactly where the reference is
    assert (~torch.isfinite(b.ema.t)).nonzero().flatten().tolist() == sorted(bad)


@pytest.mark.parametrize("device", GPU_ONLY)
def test_repeatable_and_variants_bitwise_equal(device, tmp_path):
    """Two GPU runs from the same inputs are bitwise equal; MDTF_NT_OPT=0 (cached loads / stores) changes the
    memory access only.  It is read once per process, so it runs in a fresh child."""
    _device(device)
    assert os.environ.get("MDTF_NT_OPT", "1") != "0"
    want = EH.variant_outputs()
    again = EH.variant_outputs()
    assert sorted(want) == ["ema%d" % i for i in range(5)]
    for name in want:
        assert OH.bits_equal(again[name], want[name]), name
    for i, extra in enumerate([{"MDTF_NT_OPT": "0"}]):
        env = {k: v for k, v in os.environ.items() if k != "MDTF_NT_OPT"}
        env.update(extra)
        out = str(tmp_path / ("variant%d.pt" % i))
        r = subprocess.run([sys.executable, os.path.abspath(EH.__file__), "variant", out], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, "child %r exited %d:\n%s" % (extra, r.returncode, r.stdout[-4000:])
        got = torch.load(out)
        assert sorted(got) == sorted(want)
        for name in want:
            assert OH.bits_equal(got[name], want[name]), (extra, name)


@pytest.mark.parametrize("device", GPU_ONLY)
def test_rejects_bad_arguments(device):
    """n not a multiple of 4 and a pointer off 16 bytes are refused before any launch."""
    _device(device)
    buf = torch.full((24,), 0.5, device="cuda")
    w = torch.full((24,), 0.25, device="cuda")
    before = buf.clone()
    for e, x in ((buf[4:10], w[4:10]), (buf[5:13], w[4:12]), (buf[4:12], w[5:13])):
        with pytest.raises(RuntimeError, match="invalid argument"):
            E.ema_update_(e, x, 0.1)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ------------------------------------------------------------------------------------------------------ train op
STEPS = 6
SCHEDULES = {"constant": (dict(decay=0.9), [EH.omd_of(0.9)] * STEPS),
             "num_updates": (dict(decay=0.999, num_updates="global_step"),
                             [EH.omd_of(0.999, t) for t in range(1, STEPS + 1)])}


def _check_recurrence(run, omds, what):
    st = EH.recurrence(run["w0"], run["ws"], omds)
    OH.check(run["avg"], st, "ema", len(omds) * K, what)
    return st


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_average_follows_the_recurrence(schedule):
    """Six steps of momentum SGD: average(v) is e_0 = w_0, e_t = e_{t-1} - omd_t (e_{t-1} - w_t) over the weights
    recorded after every step; with num_updates the first update uses n = 1 (n is read after the increment)."""
    kw, omds = SCHEDULES[schedule]
    run = EH.train(STEPS, kw)
    assert len(set(omds)) == (1 if schedule == "constant" else STEPS)
    _check_recurrence(run, omds, "cpu/%s" % schedule)
    assert not torch.equal(run["avg"], run["ws"][-1]) and not torch.equal(run["avg"], run["w0"])
    ema = run["ema"]
    from mdtf.train import variables as V
    for v in V.get_store().trainable_variables():
        a = ema.average(v)
        assert a.dtype == torch.float32 and tuple(a.shape) == v.shape
        assert ema.average_name(v) == v.name + "/ExponentialMovingAverage"
    assert sorted(k[0] for g in run["op"].space.groups for k in g.state) == ["full/ema", "full/ema", "full/momentum",
                                                                              "full/momentum"]


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_average_with_a_global_norm_clip(schedule):
    """The clip rebinds the step's hyper-parameter buffer on every step, eager ones too: the average still takes the
    scalar decay there and follows the recurrence over the clipped run's weights."""
    import clip_helpers as CH
    kw, omds = SCHEDULES[schedule]
    _, _, xs, ys, _, _ = EH.linear_setup(1, 8)
    clip = CH.clip_between(xs, ys, STEPS)
    run = EH.train(STEPS, kw, clip_norm=clip)
    assert run["op"].clip is not None and run["ema"].omd_buf is None
    _check_recurrence(run, omds, "cpu/clip/%s" % schedule)
    plain = EH.train(STEPS, kw)
    assert not torch.equal(run["ws"][-1], plain["ws"][-1])          # the clip did act
    clipped_alone = EH.train(STEPS, None, clip_norm=clip)
    for a, b in zip(run["ws"], clipped_alone["ws"]):
        assert OH.bits_equal(a, b)                                   # and the average does not perturb it


def test_step_is_not_perturbed(monkeypatch):
    with_avg = EH.train(STEPS, dict(decay=0.9))
    monkeypatch.setattr(E, "ema_update_", lambda *a, **k: pytest.fail("ema_update_ entered without an average"))
    plain = EH.train(STEPS, None)
    assert plain["op"].ema is None
    assert not any("ema" in k[0] for g in plain["op"].space.groups for k in g.state)
    assert with_avg["losses"] == plain["losses"]
    for a, b in zip(with_avg["ws"], plain["ws"]):
        assert OH.bits_equal(a, b)


def test_argument_errors():
    with pytest.raises(NotImplementedError, match="zero_debias"):
        mdtf.train.ExponentialMovingAverage(0.9, zero_debias=True)
    EH.fresh()
    op, _, _, _, _, _, _ = EH.build(8)
    from mdtf.train import variables as V
    vs = V.get_store().trainable_variables()
    with pytest.raises(NotImplementedError, match="subset"):
        mdtf.train.ExponentialMovingAverage(0.9).apply(var_list=vs[:2], train_op=op)
    assert op.ema is None
    ema = mdtf.train.ExponentialMovingAverage(0.9)
    assert ema.apply(var_list=vs) is op                   # None: exactly one train op is registered
    with pytest.raises(ValueError, match="already"):
        mdtf.train.ExponentialMovingAverage(0.9).apply(train_op=op)
    # a second train op: train_op=None is ambiguous
    mdtf.train.MomentumOptimizer(0.1, 0.9).apply_gradients(op.grads_and_vars)
    with pytest.raises(ValueError, match="exactly one"):
        mdtf.train.ExponentialMovingAverage(0.9).apply()


def test_async_ps_is_not_implemented():
    from mdtf.parallel.async_ps import AsyncWorker, reject_moving_average
    reject_moving_average(0.0)
    reject_moving_average(None)
    with pytest.raises(NotImplementedError, match="ps_mode"):
        reject_moving_average(0.9)
    runner = types.SimpleNamespace(optimizer=mdtf.train.MomentumOptimizer(0.1, 0.9), moving_average_decay=0.9)
    with pytest.raises(NotImplementedError, match="moving_average"):
        AsyncWorker(runner, None, None, [], 10)


# ---------------------------------------------------------------------------------------------------- checkpoint
def _names():
    from mdtf.train import variables as V
    return [v.name for v in V.get_store().trainable_variables()]


def test_checkpoint_carries_the_averages(tmp_path):
    from mdtf.train import saver as SV
    from mdtf.train import variables as V
    kw = dict(decay=0.999, num_updates="global_step")
    run = EH.train(3, kw)
    store = V.get_store()
    store.vars["dense/moving_mean"].assign(torch.tensor([1.0, 2.0, 3.0]))
    path = mdtf.train.Saver(save_optimizer_state=False).save(run["sess"], str(tmp_path / "noslots.ckpt"))
    assert not any(k.endswith("/Momentum") for k in SV.read_all(path))
    path = mdtf.train.Saver().save(run["sess"], str(tmp_path / "model.ckpt"))
    saved = SV.read_all(path)
    avg3 = {}
    for v in store.trainable_variables():
        for p in (path, str(tmp_path / "noslots.ckpt")):      # written whatever save_optimizer_state says
            t = SV.read_all(p)[v.name + "/ExponentialMovingAverage"]
            assert tuple(t.shape) == v.shape and OH.bits_equal(torch.as_tensor(t), run["ema"].average(v))
        avg3[v.name] = run["ema"].average(v)
        assert not torch.equal(avg3[v.name], v.master)
    assert int(saved["global_step"]) == 3
    for _ in range(3):
        run["sess"].run(run["op"], feed_dict=run["feed"])
    w6, a6 = EH.flat_weights(), EH.flat_averages(run["ema"])

    # restore into a fresh store, three more steps == six uninterrupted steps
    EH.fresh()
    op, _, ema, xs, ys, x_ph, y_ph = EH.build(8, ema_kwargs=kw)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    mdtf.train.Saver().restore(sess, path)
    for v in V.get_store().trainable_variables():
        assert OH.bits_equal(ema.average(v), avg3[v.name])
    for _ in range(3):
        sess.run(op, feed_dict={x_ph: xs, y_ph: ys})
    assert OH.bits_equal(EH.flat_weights(), w6) and OH.bits_equal(EH.flat_averages(ema), a6)

    # Saver(variables_to_restore()) into a fresh model without an average: the averages land in the variables
    EH.fresh()
    op, _, _, _, _, _, _ = EH.build(8)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    names = mdtf.train.ExponentialMovingAverage(0.999).variables_to_restore()
    assert sorted(names) == sorted([n + "/ExponentialMovingAverage" for n in _names()]
                                   + ["dense/moving_mean", "global_step"])
    assert mdtf.train.Saver(names).restore(sess, path) == []
    store = V.get_store()
    for v in store.trainable_variables():
        assert OH.bits_equal(v.master, avg3[v.name])
    assert store.vars["dense/moving_mean"].master.tolist() == [1.0, 2.0, 3.0]
    assert V.get_global_step().value() == 3
    # and a dict saver writes exactly its keys
    again = mdtf.train.Saver(names).save(sess, str(tmp_path / "avg_only.ckpt"))
    assert sorted(SV.read_all(again)) == sorted(names)


def test_restore_without_averages_starts_from_the_weights(tmp_path):
    from mdtf.train import saver as SV
    from mdtf.train import variables as V
    run = EH.train(3, None)
    path = mdtf.train.Saver().save(run["sess"], str(tmp_path / "plain.ckpt"))
    assert not any("ExponentialMovingAverage" in k for k in SV.read_all(path))
    w3 = EH.flat_weights()
    EH.fresh()
    op, _, ema, _, _, _, _ = EH.build(8, ema_kwargs=dict(decay=0.9))
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    assert not torch.equal(EH.flat_weights(), w3)
    mdtf.train.Saver().restore(sess, path)
    assert OH.bits_equal(EH.flat_weights(), w3) and OH.bits_equal(EH.flat_averages(ema), w3)


# ------------------------------------------------------------------------------------------------ average_weights
def _snapshot(op):
    out = []
    for g in op.space.groups:
        out += [g.master.clone(), g.shadow.clone(), g.state_buffer("full/ema", g.numel).clone()]
    return out


def test_average_weights_exchanges_in_place():
    from mdtf.train import variables as V
    kw = dict(decay=0.9)
    run = EH.train(3, kw, compute_dtype=torch.bfloat16)
    op, ema = run["op"], run["ema"]
    vs = V.get_store().trainable_variables()
    assert all(v.shadow is not None and v.shadow.dtype == torch.bfloat16 for v in vs)
    before = _snapshot(op)
    ptrs = [t.data_ptr() for g in op.space.groups for t in (g.master, g.shadow)]
    avg = {v.name: ema.average(v) for v in vs}
    raw = {v.name: v.master.clone() for v in vs}
    with ema.average_weights():
        for v in vs:
            assert OH.bits_equal(v.master, avg[v.name]) and not torch.equal(v.master, raw[v.name])
            assert OH.bits_equal(v.shadow, avg[v.name].bfloat16())
            assert OH.bits_equal(ema.average(v), raw[v.name])
    assert ptrs == [t.data_ptr() for g in op.space.groups for t in (g.master, g.shadow)]
    for a, b in zip(_snapshot(op), before):
        assert OH.bits_equal(a, b)
    run["sess"].run(op, feed_dict=run["feed"])
    w4, a4 = EH.flat_weights(), EH.flat_averages(ema)
    never = EH.train(4, kw, compute_dtype=torch.bfloat16)
    assert OH.bits_equal(w4, never["ws"][-1]) and OH.bits_equal(a4, never["avg"])


# ------------------------------------------------------------------------------------------------- flag and Eval
def _operator(cls, tmp_path, **extra):
    """A run-loop operator with what the annotation entry point injects, on a one-replica stand-in for the server."""
    from mdtf.data.loaders import InputOptions, SyntheticDataLoader
    from mdtf.runtime import Net
    Lin, MSE, _, _, _, _ = EH.linear_setup(1, 8)
    server = types.SimpleNamespace(is_chief=True, local_rank=0, target="", worker_group=None, store=None,
                                   layout=types.SimpleNamespace(num_worker_ranks=1),
                                   device=lambda: torch.device("cpu"), signal_done=lambda: None)
    from mdtf.cluster import ClusterSpec
    cluster = ClusterSpec({"worker": ["127.0.0.1:1"]})
    loader = SyntheticDataLoader(shape=(8,), num_classes=1, label_shape=(1,), label_dtype=torch.float32)
    loader.batch_size = 8
    op = cls.__new__(cls)
    attrs = dict(task_index=0, job_name="worker", optimizer=mdtf.train.MomentumOptimizer(0.1, 0.9), server=server,
                 cluster=cluster, data_loader=loader, input_mode=InputOptions.SYNTHETIC, batch_size=8, epoch_num=1,
                 sample_number=8 * 5, model_dir=str(tmp_path / "model"), data_dir="", net=Net(Lin()), loss=MSE(),
                 gpu_num=0, ps_mode="allreduce")
    attrs.update(extra)
    for k, v in attrs.items():
        setattr(op, k, v)
    return op, loader, MSE


def _flag(monkeypatch, value):
    from mdtf.config.flags import FLAGS
    monkeypatch.setattr(FLAGS, "moving_average_decay", value)


def test_flag_attaches_the_average_and_eval_reads_it(tmp_path, monkeypatch):
    from mdtf.runtime.eval import Eval
    from mdtf.runtime.train import Train
    from mdtf.train import saver as SV
    from mdtf.train import variables as V
    EH.fresh()
    _flag(monkeypatch, 0.9)
    t, _, _ = _operator(Train, tmp_path)
    t.run()
    ema = t.train_op.ema
    assert isinstance(ema, mdtf.train.ExponentialMovingAverage) and ema.decay == 0.9 and ema.op is t.train_op
    assert ema.num_updates is V.get_global_step() and V.get_global_step().value() == 5
    ckpt = SV.latest_checkpoint(str(tmp_path / "model"))
    saved = SV.read_all(ckpt)
    names = _names()
    assert all(n + "/ExponentialMovingAverage" in saved for n in names)

    def loss_of(weights, loader):
        x, y = loader._next()
        w, b, h = (torch.as_tensor(weights[n]) for n in ("dense/w", "dense/b", "dense2/w"))
        return float(((torch.tanh(x @ w + b) @ h - y) ** 2).mean())

    def evaluate(flag):
        EH.fresh()
        _flag(monkeypatch, flag)
        e, loader, _ = _operator(Eval, tmp_path, eval_steps=2)
        m = e.run()
        return m, loader, e

    m, loader, e = evaluate(0.9)
    want_avg = loss_of({n: saved[n + "/ExponentialMovingAverage"] for n in names}, loader)
    want_raw = loss_of({n: saved[n] for n in names}, loader)
    assert abs(want_avg - want_raw) > 1e-3 * abs(want_raw)
    assert e.evaluated_averages and m["global_step"] == 5
    assert m["loss"] == pytest.approx(want_avg, rel=1e-5)
    m, _, e = evaluate(0.0)                                 # without the flag Eval is unchanged: the raw weights
    assert not e.evaluated_averages and m["loss"] == pytest.approx(want_raw, rel=1e-5)


def test_eval_falls_back_to_raw_weights(tmp_path, monkeypatch):
    """A checkpoint written without averages: Eval with the flag warns and evaluates the raw weights."""
    from mdtf.runtime.eval import Eval
    from mdtf.runtime.train import Train
    EH.fresh()
    _flag(monkeypatch, 0.0)
    t, _, _ = _operator(Train, tmp_path)
    t.run()
    assert t.train_op.ema is None
    losses = []
    for flag in (0.0, 0.9):
        EH.fresh()
        _flag(monkeypatch, flag)
        e, _, _ = _operator(Eval, tmp_path, eval_steps=2)
        losses.append(e.run()["loss"])
        assert not e.evaluated_averages
    assert losses[0] == losses[1]


# ------------------------------------------------------------------------------------------------- two-rank gloo
@pytest.mark.slow
@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_two_rank_gloo(mode, tmp_path):
    """Each rank's averages follow the fp64 recurrence over the weights that rank recorded after every step, and
    the recurrence over the single-process reference's weights, both under the bound of the single-process test;
    identical on both ranks; a checkpoint round-trips."""
    import torch.multiprocessing as mp
    from mdtf.cluster.launcher import free_port
    world, batch = 2, 4
    omds = [EH.omd_of(0.999, t) for t in range(1, STEPS + 1)]
    mp.start_processes(EH.ema_worker, args=(world, free_port(), mode, STEPS, str(tmp_path), batch), nprocs=world,
                       join=True, start_method="spawn")
    res = [json.load(open(os.path.join(str(tmp_path), "rank%d.json" % r))) for r in range(world)]
    ref = EH.train(STEPS, dict(decay=0.999, num_updates="global_step"), batch=world * batch)
    st_ref = EH.recurrence(ref["w0"], ref["ws"], omds)
    key = "shard/ema" if mode == "sharded" else "full/ema"
    for r in res:
        assert r["collective"] and r["buckets"] > 1 and key in r["state_keys"]
        run = dict(w0=torch.tensor(r["w0"]), ws=[torch.tensor(w) for w in r["ws"]], avg=torch.tensor(r["avg"]))
        _check_recurrence(run, omds, "gloo/%s" % mode)
        OH.check(run["avg"], st_ref, "ema", STEPS * K, "gloo/%s against the single process" % mode)
        assert r["avg_after"] != r["avg"]
        assert r["restored_avg"] == r["avg"] and r["restored_w"] == r["ws"][-1] and r["restored_step"] == STEPS
    assert res[0]["avg"] == res[1]["avg"] and res[0]["ws"] == res[1]["ws"]


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_gpu_average_follows_the_recurrence(schedule):
    """The CPU recurrence test on cuda: the kernel's averages against fp64 over the weights the GPU run recorded,
    and the PyTorch branch driven over the same weights lands within the same bound of the same reference."""
    _device("cuda")
    kw, omds = SCHEDULES[schedule]
    run = EH.train(STEPS, kw, device="cuda")
    assert run["op"].space.groups[0].master.is_cuda
    st = _check_recurrence(run, omds, "cuda/%s" % schedule)
    e = run["w0"].clone()
    for w, omd in zip(run["ws"], omds):
        E.ema_update_(e, w, omd)
    OH.check(e, st, "ema", len(omds) * K, "cpu branch over the cuda weights/%s" % schedule)


@pytest.mark.gpu
def test_hip_graph_replay_equals_eager():
    """Two eager warm-ups, four replays, the decay changing every replay (num_updates = global step): averages
    bitwise equal to the all-eager run, one capture, no fallback."""
    _device("cuda")
    from mdtf.ops import _native
    torch.manual_seed(0)
    batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(6)]
    assert len(set(EH.omd_of(0.999, t) for t in range(1, 7))) == 6
    _native.set_deterministic(True)
    try:
        l_e, w_e, a_e, op_e = EH.run_resnetish(batches, hip_graph=False)
        l_g, w_g, a_g, op = EH.run_resnetish(batches, hip_graph=True)
    finally:
        _native.set_deterministic(False)
    g = op.graph
    assert op_e.graph is None
    assert g is not None and g.graph is not None and g.replays == 4 and g.fallbacks == 0 and not g.disabled, vars(g)
    assert l_e == l_g, (l_e, l_g)
    for k in w_e:
        assert torch.equal(w_e[k], w_g[k]), k
        assert OH.bits_equal(a_e[k], a_g[k]), k
        assert not torch.equal(a_e[k], w_e[k]), k
    assert op.ema.omd_buf.tolist() == [EH.omd_of(0.999, 6)]


@pytest.mark.gpu
def test_hip_graph_replay_with_a_global_norm_clip():
    """Clip plus average: two eager steps (the clip's effective buffer is not the graph's: the scalar decay), then
    four replays reading the average's own buffer; bitwise the all-eager run."""
    _device("cuda")
    from mdtf.ops import _native
    torch.manual_seed(0)
    batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(6)]
    _native.set_deterministic(True)
    try:
        _, w_p, _, _ = EH.run_resnetish(batches, hip_graph=False)
        l_e, w_e, a_e, op_e = EH.run_resnetish(batches, hip_graph=False, clip_norm=0.5)
        l_g, w_g, a_g, op = EH.run_resnetish(batches, hip_graph=True, clip_norm=0.5)     # last: a reset drops graphs
    finally:
        _native.set_deterministic(False)
    g = op.graph
    assert op_e.ema.omd_buf is None and op_e.clip is not None
    assert float(op_e.last_global_norm[1]) < 1.0                     # the last step was clipped
    assert g is not None and g.graph is not None and g.replays == 4 and g.fallbacks == 0 and not g.disabled, vars(g)
    assert l_e == l_g, (l_e, l_g)
    assert any(not torch.equal(w_e[k], w_p[k]) for k in w_e)
    for k in w_e:
        assert torch.equal(w_e[k], w_g[k]), k
        assert OH.bits_equal(a_e[k], a_g[k]), k
    assert op.ema.omd_buf.tolist() == [EH.omd_of(0.999, 6)]


@pytest.mark.gpu
def test_sharded_one_rank_group_equals_allreduce(monkeypatch):
    """Sharded mode on a forced 1-rank RCCL group keeps its in-backward update (update_targets() is empty) and
    still averages every shard: bitwise the all-reduce mode's averages."""
    _device("cuda")
    import socket
    import torch.distributed as dist
    from mdtf.ops import _native
    monkeypatch.setenv("MDTF_FORCE_COLLECTIVES", "1")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(4)]
        _native.set_deterministic(True)
        try:
            l_a, w_a, a_a, op_a = EH.run_resnetish(batches, hip_graph=False, mode="allreduce")
            l_s, w_s, a_s, op_s = EH.run_resnetish(batches, hip_graph=False, mode="sharded")
        finally:
            _native.set_deterministic(False)
        red = op_s.reducer
        assert red.collective and red.overlap and len(op_s.space.buckets) > 1
        assert red.eager_update is not None and red.update_targets() == [] and len(red.all_targets()) > 0
        assert any(k[0] == "shard/ema" for gr in op_s.space.groups for k in gr.state)
        assert op_a.reducer.eager_update is None and len(op_a.reducer.update_targets()) > 0
        assert l_a == l_s, (l_a, l_s)
        for k in w_a:
            assert torch.equal(w_a[k], w_s[k]), k
            assert OH.bits_equal(a_a[k], a_s[k]), k
    finally:
        from mdtf.train import step as S
        S.release_graphs()
        dist.destroy_process_group()
