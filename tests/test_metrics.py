"""``mdtf.metrics`` and ``mdtf.nn.in_top_k`` (``mdtf.ops.metrics`` / ``csrc/metrics.hip``): the hits kernel element by
element and exactly against the definition, the fp64 reduction against correctly rounded sums, accumulation, hipGraph
replay, and the metrics through ``Eval``, BERT's loss and the Estimator.

Kernel tests take a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.metrics``, ``cuda`` the HIP kernels.
"""
import json
import os
import sys

import pytest
import torch

import mdtf
from mdtf import metrics as M
from mdtf.ops import metrics as OM

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_helpers as MH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from mdtf.ops import _native
        _native.lib()
        assert _native.mode() != "torch"
    return device


# ------------------------------------------------------------------------------------------------------- in_top_k
BF, FP = torch.bfloat16, torch.float32
# (rows per launch, K, row stride, element offset of the base, dtype)
# one wave per row, four rows per block: 5 rows are a full block and a block of one row
WAVE = [(5, kk, kk, 0, dt) for kk in (1, 2, 63, 64, 65, 1000) for dt in (BF, FP)]
WAVE.append((5, 2049, 2049, 0, BF))           # a wide bf16 row with odd K: no vector form fits, the wave form again
PAIR = [(5, 2050, 2050, 2, BF)]               # K and stride even, the base 4 bytes off a 16-byte boundary
# 16-byte vectors, 256 threads, four loads in flight: 2048 = 256 vectors, one each | 6163 = 770 vectors (two threads
# run the four-deep loop, everyone the single-vector loop) and 3 columns in a masked last vector, stride 6168 |
# the masked-LM head, 3815 vectors + 2 columns
V8 = [(3, 2048, 2048, 0, BF), (3, 6163, 6168, 0, BF), (3, 30522, 30720, 0, BF)]
SHAPES = WAVE + PAIR + V8
KS = ["1", "2", "5", "K", "K+3"]


def _shape_id(s):
    return "n%d-K%d-ld%d-off%d-%s" % (s[0], s[1], s[2], s[3], "bf16" if s[4] == BF else "fp32")


@pytest.mark.parametrize("kname", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("device", DEVICES)
def test_in_top_k_is_the_definition(device, shape, kname):
    """Every row of every launch, exactly.  The rows (metrics_helpers.scenario_rows): ties with the target that
    straddle the boundary (k - 1 greater plus 3 equal), k and k - 1 strictly greater, a NaN / +inf / -inf target,
    NaN / +inf / -inf elsewhere beside a finite target, labels -1 and K, a row of weight 0 (the skipped rows are all
    NaN), the greatest element and the target in column 0 and in column K - 1.  Pad columns hold +inf."""
    device = _device(device)
    n, kk, ld, off, dt = shape
    k = {"K": kk, "K+3": kk + 3}.get(kname) or int(kname)
    gen = torch.Generator().manual_seed(kk * 7 + k)
    rows, labels, weights = MH.scenario_rows(kk, k, gen)
    seen = set()
    for x, lab, w in MH.launches(rows, labels, weights, n, ld, off, dt, device):
        assert x.shape == (n, kk) and x.stride() == (ld, 1) and x.dtype == dt
        assert x.storage_offset() == off
        cpu = x.cpu()
        want_w, want = MH.oracle_hits(cpu, lab, w, k), MH.oracle_hits(cpu, lab, None, k)
        got_w = OM.in_top_k_hits(x, lab.to(device), k, w.to(device))
        assert got_w.dtype == torch.float32 and torch.equal(got_w.cpu(), want_w), (got_w.tolist(), want_w.tolist())
        # the public form: no weights (the NaN row of weight 0 is read, and is False), int32 [N, 1] targets
        got = mdtf.nn.in_top_k(x, lab.to(device, torch.int32).reshape(n, 1), k)
        assert got.dtype == torch.bool and torch.equal(got.cpu(), want != 0)
        seen.update(want_w.tolist())
    if kk >= 8 and k < kk:
        assert seen == {0.0, 1.0}


@pytest.mark.parametrize("device", DEVICES)
def test_in_top_k_other_layouts_and_dtypes(device):
    """A column-strided view and fp16 / fp64 logits are copied or converted first; the result is the definition's."""
    device = _device(device)
    gen = torch.Generator().manual_seed(11)
    rows, labels, weights = MH.scenario_rows(40, 3, gen)
    want = MH.oracle_hits(rows, labels, weights, 3)
    wide = torch.full((rows.shape[0], 80), MH.INF)
    wide[:, ::2] = rows
    dev = rows.to(device)
    for x in (wide.to(device)[:, ::2], dev.half(), dev.double(), dev.t().contiguous().t()):
        got = OM.in_top_k_hits(x, labels.to(device), 3, weights.to(device))
        assert torch.equal(got.cpu(), want)
    with pytest.raises(ValueError):
        OM.in_top_k_hits(rows.to(device), labels.to(device), 0)
    with pytest.raises(ValueError):
        OM.in_top_k_hits(rows.to(device), labels[:-1].to(device), 1)
    assert mdtf.nn.in_top_k(rows[:0].to(device), labels[:0].to(device), 1).shape == (0,)


# --------------------------------------------------------------------------------------------------------- reduce
SIZES = [1, 5, 255, 256, 257, 1280]            # one block of 256 threads: below, at and above one trip, five trips
DYADIC = torch.tensor([0.0, 0.5, 1.0, 2.5])


def _dyadic(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (n,), generator=g).float(), DYADIC[torch.randint(0, 4, (n,), generator=g)], g)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_reduce_and_the_four_functions_exact(device, n):
    """Weights from {0, 0.5, 1, 2.5} and 0 / 1 values: every product and partial sum is exact in fp64, so ``pair``
    equals the oracle bit for bit, in any order of summation."""
    device = _device(device)
    v, w, g = _dyadic(n, n)
    pair = OM.metric_reduce(v.to(device), w.to(device))
    assert pair.dtype == torch.float64 and pair.shape == (2,) and pair.device.type == device
    assert pair.tolist() == MH.oracle_pair(v, w)
    assert OM.metric_reduce(v.to(device)).tolist() == MH.oracle_pair(v)
    assert M.mean(v.to(device), w.to(device)).pair.tolist() == MH.oracle_pair(v, w)
    # accuracy: class ids that agree where v is 1
    labels = torch.randint(0, 7, (n,), generator=g)
    preds = torch.where(v != 0, labels, (labels + 1) % 7)
    assert M.accuracy(labels.to(device), preds.to(device), w.to(device)).pair.tolist() == MH.oracle_pair(v, w)
    assert M.accuracy(labels.to(device), preds.to(device)).pair.tolist() == MH.oracle_pair(v)
    # mean_squared_error: predictions off by 1 where v is 1
    y = torch.randint(-3, 4, (n, 1), generator=g).float()
    p = y + v.reshape(n, 1)
    assert M.mean_squared_error(y.to(device), p.to(device), w.reshape(n, 1).to(device)).pair.tolist() \
        == MH.oracle_pair(v, w)
    # top_k_accuracy: the hits are the oracle's, the weights reach both launches
    x = torch.randint(-8, 9, (n, 7), generator=g).float() / 4.0
    hits = MH.oracle_hits(x, labels, w, 2)
    mv = M.top_k_accuracy(labels.to(device), x.to(device), 2, w.to(device))
    assert mv.pair.tolist() == MH.oracle_pair(hits, w)
    want = MH.oracle_pair(hits, w)
    assert mv.value() == (want[0] / want[1] if want[1] else 0.0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_mean_of_random_values_within_the_rounding_bound(device, n):
    device = _device(device)
    g = torch.Generator().manual_seed(100 + n)
    v, w = torch.randn(n, generator=g), torch.rand(n, generator=g)
    w[::7] = 0.0
    total, count = M.mean(v.to(device), w.to(device)).pair.tolist()
    want_t, want_c = MH.oracle_pair(v, w)
    bt, bc = MH.bound(v, w, n)
    print("n=%d total err %.3e (bound %.3e) count err %.3e (bound %.3e)"
          % (n, abs(total - want_t), bt, abs(count - want_c), bc))
    assert abs(total - want_t) <= bt and abs(count - want_c) <= bc
    assert want_c > 0 or n == 1


@pytest.mark.parametrize("device", DEVICES)
def test_zero_weights_skip_and_scalar_weights_scale(device):
    device = _device(device)
    v, w, _ = _dyadic(257, 9)
    w[0], w[5] = 0.0, 0.0
    bad = v.clone()
    bad[0], bad[5] = MH.NAN, MH.INF
    assert M.mean(bad.to(device), w.to(device)).pair.tolist() == MH.oracle_pair(v, w)      # finite, and unchanged
    none = M.mean(bad.to(device), torch.zeros(257).to(device))
    assert none.pair.tolist() == [0.0, 0.0] and none.value() == 0.0
    one, two = M.mean(v.to(device), w.to(device)), M.mean(v.to(device), 2.0)
    assert two.pair.tolist() == [2.0 * float(v.sum()), 2.0 * 257] and two.value() == M.mean(v.to(device)).value()
    assert M.mean(bad.to(device), 0.0).pair.tolist() == [0.0, 0.0]
    assert one.value() == MH.oracle_pair(v, w)[0] / MH.oracle_pair(v, w)[1]
    # a weight that broadcasts over the values
    m = v[:256].reshape(64, 4)
    col = DYADIC.reshape(1, 4)
    assert M.mean(m.to(device), col.to(device)).pair.tolist() == MH.oracle_pair(m, col.expand(64, 4))


# ---------------------------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize("device", DEVICES)
def test_three_batches_into_one_accumulator(device):
    device = _device(device)
    acc = M.Accumulator()
    assert acc.result() == 0.0
    acc = M.Accumulator(device)
    vs, ws = [], []
    for i, n in enumerate((5, 257, 64)):
        v, w, _ = _dyadic(n, 20 + i)
        mv = M.mean(v.to(device), w.to(device), accumulator=acc)
        assert mv.pair.tolist() == MH.oracle_pair(v, w)                 # still that batch alone
        vs.append(v)
        ws.append(w)
    want = MH.oracle_pair(torch.cat(vs), torch.cat(ws))
    assert acc.tensor.device.type == device and acc.tensor.tolist() == want
    assert acc.result() == want[0] / want[1]
    acc.reset()
    assert acc.tensor.tolist() == [0.0, 0.0] and acc.result() == 0.0

    # random values: the bound of the single call over the concatenation
    g = torch.Generator().manual_seed(30)
    vs = [torch.randn(n, generator=g) for n in (300, 7, 129)]
    ws = [torch.rand(n, generator=g) for n in (300, 7, 129)]
    lazy = M.Accumulator()                                               # made on the device of its first update
    for v, w in zip(vs, ws):
        acc.update(M.mean(v.to(device), w.to(device)))                   # a MetricValue added on the device
        lazy.update(v.to(device), w.to(device))                          # mean's arguments, the fused form
    want = MH.oracle_pair(torch.cat(vs), torch.cat(ws))
    bt, bc = MH.bound(torch.cat(vs), torch.cat(ws), 436)
    for a in (acc, lazy):
        total, count = a.tensor.tolist()
        assert a.tensor.device.type == device
        assert abs(total - want[0]) <= bt and abs(count - want[1]) <= bc
    with pytest.raises(ValueError):
        OM.metric_reduce(vs[0].to(device), accum=torch.zeros(2, device=device))        # fp32 state


@pytest.mark.parametrize("device", GPU_ONLY)
def test_hip_graph_replay_accumulates(device):
    """``top_k_accuracy(..., accumulator=acc)`` captured once on a side stream (two launches in a chain, static input
    buffers), replayed three times over three different batches: ``acc`` is the oracle over all three."""
    _device(device)
    n, kk, k = 37, 300, 3
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randint(-40, 41, (n, kk), generator=g).float() / 8.0, torch.randint(0, kk, (n,), generator=g),
                DYADIC[torch.randint(0, 4, (n,), generator=g)]) for _ in range(3)]
    for bx, bl, _ in batches:
        bl[::2] = bx[::2].argmax(-1)                                  # hits among the (mostly) missing random labels
    x = torch.zeros(n, kk, device="cuda", dtype=torch.bfloat16)
    lab = torch.zeros(n, device="cuda", dtype=torch.int64)
    w = torch.ones(n, device="cuda")
    acc = M.Accumulator("cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.top_k_accuracy(lab, x, k, w, accumulator=acc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    acc.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        mv = M.top_k_accuracy(lab, x, k, w, accumulator=acc)
    hits, weights = [], []
    for bx, bl, bw in batches:
        x.copy_(bx)
        lab.copy_(bl)
        w.copy_(bw)
        graph.replay()
        torch.cuda.synchronize()
        hits.append(MH.oracle_hits(x.cpu(), bl, bw, k))
        weights.append(bw)
        assert mv.pair.tolist() == MH.oracle_pair(hits[-1], bw)
    assert acc.tensor.tolist() == MH.oracle_pair(torch.cat(hits), torch.cat(weights))
    assert 0.0 < acc.result() < 1.0
    del graph


# ------------------------------------------------------------------------------------------------------------ Eval
def _trained(tmp_path):
    """Five steps of Train on the 10-class linear model; the checkpoint's variables."""
    from mdtf.runtime.train import Train
    from mdtf.train import saver as SV
    MH.fresh()
    Lin10, Xent = MH.classifier()
    t = MH.operator(Train, tmp_path / "model", Lin10(), Xent(), MH.ListLoader(MH.class_batches(5, 8, seed=1)))
    t.run()
    saved = SV.read_all(SV.latest_checkpoint(str(tmp_path / "model")))
    return torch.as_tensor(saved["dense/w"]).float(), torch.as_tensor(saved["dense/b"]).float()


def _expected(w, b, batches, top_k):
    losses, correct, hits, count = [], 0, 0.0, 0
    for x, y in batches:
        logits = x @ w + b
        losses.append(float(torch.nn.functional.cross_entropy(logits.double(), y)))
        correct += int((logits.argmax(-1) == y).sum())
        hits += float(MH.oracle_hits(logits, y, None, top_k).sum())
        count += y.numel()
    return sum(losses) / len(losses), correct / count, hits / count


def _eval(tmp_path, batches, **extra):
    from mdtf.runtime.eval import Eval
    MH.fresh()
    Lin10, Xent = MH.classifier()
    loader = MH.ListLoader(batches)
    e = MH.operator(Eval, tmp_path / "model", Lin10(), Xent(), loader, eval_steps=2, **extra)
    return e.run(), loader


def test_eval_reports_top_k_beside_loss_and_accuracy(tmp_path, monkeypatch):
    from mdtf.config.flags import FLAGS
    w, b = _trained(tmp_path)
    batches = MH.class_batches(3, 8, seed=2)
    m, loader = _eval(tmp_path, batches)
    assert len(loader.served) == 2 and FLAGS.eval_top_k == 5
    loss, acc, top5 = _expected(w, b, loader.served, 5)
    assert m["steps"] == 2 and m["global_step"] == 5
    assert m["loss"] == pytest.approx(loss, rel=1e-5)
    assert m["accuracy"] == pytest.approx(acc, rel=1e-5) and m["accuracy"] == acc
    assert m["top_5_accuracy"] == top5 and acc < top5 < 1.0
    assert sorted(m) == ["accuracy", "global_step", "loss", "steps", "top_5_accuracy"]
    # the attribute wins over the flag; 0 and a k that is not below the number of classes drop the key
    for k in (0, 10):
        m, _ = _eval(tmp_path, batches, eval_top_k=k)
        assert sorted(m) == ["accuracy", "global_step", "loss", "steps"]
        assert m["loss"] == pytest.approx(loss, rel=1e-5) and m["accuracy"] == acc
    m, loader = _eval(tmp_path, batches, eval_top_k=3)
    assert m["top_3_accuracy"] == _expected(w, b, loader.served, 3)[2] and "top_5_accuracy" not in m
    monkeypatch.setattr(FLAGS, "eval_top_k", 2)
    m, loader = _eval(tmp_path, batches)
    assert m["top_2_accuracy"] == _expected(w, b, loader.served, 2)[2]
    monkeypatch.setattr(FLAGS, "eval_top_k", 0)
    assert "top_2_accuracy" not in _eval(tmp_path, batches)[0]


def test_eval_of_tuple_logits_reports_the_loss_hook(tmp_path):
    """A Net that returns a tuple and a Loss with ``metrics``: the loss plus the named metrics."""
    from mdtf.runtime import Loss, Model
    from mdtf.runtime.eval import Eval
    from mdtf.train import variables as V

    class Two(Model):
        def inference(self, x):
            w = V.get_variable("w", [8, 4], initializer=V.random_normal_initializer(stddev=0.5))
            return x @ w, x.sum(-1)

    class TwoLoss(Loss):
        def loss(self, p, t):
            return ((p[1] - t.float()) ** 2).mean()

        def metrics(self, p, t):
            return {"top_2": M.top_k_accuracy(t, p[0], 2), "mse": M.mean_squared_error(t, p[1]),
                    "class_is_zero": M.accuracy(torch.zeros_like(t), t)}

    assert Loss.metrics(TwoLoss(), None, None) is None
    MH.fresh()
    g = torch.Generator().manual_seed(8)
    batches = [(torch.randn(n, 8, generator=g), torch.randint(0, 4, (n,), generator=g)) for n in (6, 6)]
    loader = MH.ListLoader(batches)
    e = MH.operator(Eval, tmp_path / "none", Two(), TwoLoss(), loader, eval_steps=2)
    m = e.run()
    w = V.get_store().vars["w"].master.detach().float()
    hits = sum(float(MH.oracle_hits(x @ w, y, None, 2).sum()) for x, y in loader.served)
    sq = torch.cat([(x.sum(-1) - y.float()) ** 2 for x, y in loader.served])
    assert sorted(m) == ["accuracy", "class_is_zero", "global_step", "loss", "mse", "steps", "top_2"]
    assert m["accuracy"] is None and m["steps"] == 2
    assert m["top_2"] == hits / 12
    assert m["mse"] == pytest.approx(float(sq.double().mean()), rel=1e-6)
    assert m["loss"] == pytest.approx(float(sum(s.double().mean() for s in sq.split(6)) / 2), rel=1e-5)
    assert m["class_is_zero"] == sum(int((y == 0).sum()) for _, y in loader.served) / 12


def test_pack_and_unpack_of_the_all_reduced_vector():
    from mdtf.runtime.eval import pack_sums, unpack_sums
    loss, correct, a, b = M.Accumulator(), M.Accumulator("cpu"), M.Accumulator("cpu"), M.Accumulator()
    M.mean(torch.tensor([1.5, 2.5]), accumulator=loss)
    M.mean(torch.tensor([1.0, 0.0, 1.0]), accumulator=correct)
    M.mean(torch.tensor([4.0]), 0.5, accumulator=a)
    t = pack_sums(7, loss, correct, [a, b], torch.device("cpu"))
    assert t.dtype == torch.float64 and t.tolist() == [4.0, 2.0, 3.0, 7.0, 2.0, 0.5, 0.0, 0.0]
    two = t + t                                                       # what two equal replicas all-reduce to
    assert unpack_sums(two, ["a", "b"]) == (8.0, 4.0, 6.0, 14.0, {"a": (4.0, 1.0), "b": (0.0, 0.0)})
    with pytest.raises(ValueError):
        unpack_sums(t, ["a"])


@pytest.mark.slow
def test_two_rank_gloo_eval_equals_the_union(tmp_path):
    """Two gloo ranks evaluate two different batches each: every rank reports the single-process metrics over all
    four."""
    import torch.multiprocessing as mp
    from mdtf.cluster.launcher import free_port
    w, b = _trained(tmp_path)
    world, per_rank = 2, 2
    mp.start_processes(MH.eval_worker, args=(world, free_port(), str(tmp_path / "model"), str(tmp_path), per_rank),
                       nprocs=world, join=True, start_method="spawn")
    batches = MH.class_batches(world * per_rank, 8, seed=3)
    loss, acc, top3 = _expected(w, b, batches, 3)
    for r in range(world):
        m = json.load(open(os.path.join(str(tmp_path), "rank%d.json" % r)))
        assert m["steps"] == world * per_rank
        assert m["loss"] == pytest.approx(loss, rel=1e-5)
        assert m["accuracy"] == acc and m["top_3_accuracy"] == top3


# ------------------------------------------------------------------------------------------------------------ BERT
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("device", DEVICES)
def test_bert_pretraining_metrics(device, weighted):
    from mdtf.models.bert import BertPretrainingLoss
    device = _device(device)
    B, P, vocab = 3, 4, 16
    g = torch.Generator().manual_seed(12)
    mlm = torch.randn(B * P, vocab, generator=g)
    nsp = torch.randn(B, 2, generator=g)
    ids = torch.randint(0, vocab, (B, P), generator=g)
    ids[0, 0], ids[1, 1] = int(mlm[0].argmax()), int(mlm[P + 1].argmax())       # two certain hits among the misses
    ns = torch.randint(0, 2, (B, 1), generator=g)
    if weighted:
        w = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]])
        gt = torch.cat([ids * w, ns, w], 1)
        mlm[w.reshape(-1) == 0] = MH.NAN                                         # padding slots: never read
    else:
        w = torch.ones(B, P, dtype=torch.long)
        gt = torch.cat([ids, ns], 1)
    live = w.reshape(-1) != 0
    loss = BertPretrainingLoss(P, weighted=weighted)
    m = loss.metrics((mlm.to(device), nsp.to(device)), gt.to(device))
    assert sorted(m) == ["masked_lm_accuracy", "masked_lm_loss", "next_sentence_accuracy", "next_sentence_loss"]
    assert all(isinstance(v, M.MetricValue) and v.pair.device.type == device for v in m.values())
    xent = torch.nn.functional.cross_entropy
    lm, li = mlm[live].double(), ids.reshape(-1)[live]
    assert m["masked_lm_accuracy"].pair.tolist() == [float((lm.argmax(-1) == li).sum()), float(live.sum())]
    assert 0.0 < m["masked_lm_accuracy"].value() < 1.0
    assert m["masked_lm_loss"].value() == pytest.approx(float(xent(lm, li)), rel=1e-5)
    assert m["masked_lm_loss"].pair[1].item() == float(live.sum())
    assert m["next_sentence_accuracy"].pair.tolist() == [float((nsp.argmax(-1) == ns[:, 0]).sum()), float(B)]
    assert m["next_sentence_loss"].value() == pytest.approx(float(xent(nsp.double(), ns[:, 0])), rel=1e-5)
    # and the same through [B, P, vocab] logits
    m3 = loss.metrics((mlm.reshape(B, P, vocab).to(device), nsp.to(device)), gt.to(device))
    assert m3["masked_lm_accuracy"].pair.tolist() == m["masked_lm_accuracy"].pair.tolist()


# ------------------------------------------------------------------------------------------------------- Estimator
def test_estimator_evaluates_metric_values_beside_tuples(tmp_path):
    import mdtf.layers  # noqa: F401
    from mdtf.estimator import Estimator, EstimatorSpec, ModeKeys, RunConfig
    seen = []

    def model_fn(features, labels, mode, params):
        with mdtf.variable_scope("out"):
            w = mdtf.get_variable("weights", [8, 6], initializer=mdtf.train.variables.xavier_initializer())
        logits = mdtf.nn.matmul(features, w)
        loss = mdtf.nn.sparse_softmax_cross_entropy_with_logits(labels, logits).mean()
        if mode == ModeKeys.EVAL:
            seen.append((logits.detach().clone(), labels.clone()))
            return EstimatorSpec(mode, loss=loss, eval_metric_ops={
                "top2": mdtf.metrics.top_k_accuracy(labels, logits, 2),
                "acc": mdtf.estimator.metrics.accuracy(labels, logits.argmax(-1))})
        train_op = mdtf.train.AdamOptimizer(1e-2).minimize(loss, global_step=mdtf.train.get_global_step())
        return EstimatorSpec(mode, loss=loss, train_op=train_op)

    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(80, 8, generator=g), torch.randint(0, 6, (80,), generator=g)

    def input_fn():
        for i in range(0, 80, 32):                                  # 32, 32, 16 rows
            yield x[i:i + 32], y[i:i + 32]

    est = Estimator(model_fn, model_dir=str(tmp_path), config=RunConfig(log_step_count_steps=0, tf_random_seed=1))
    est.train(input_fn)
    r = est.evaluate(input_fn)
    batches = [b for b in seen if b[0].shape[0] in (32, 16)][-3:]
    assert [b[0].shape[0] for b in batches] == [32, 32, 16]
    hits = sum(float(MH.oracle_hits(lg, lb, None, 2).sum()) for lg, lb in batches)
    right = sum(float((lg.argmax(-1) == lb).float().mean()) * lb.numel() for lg, lb in batches)
    assert sorted(r) == ["acc", "global_step", "loss", "top2"]
    assert r["top2"] == hits / 80 and 0.0 < r["top2"] < 1.0
    assert r["acc"] == right / 80
