"""``mdtf.losses`` (``ops/losses.py``, ``csrc/losses.hip``): label-smoothed, weighted sparse softmax cross entropy and
the ``tf.losses`` reductions against an fp64 oracle written here from the definition, element by element.

Every numeric test takes a device as ``test_nhwc_kernels.py`` does: ``cpu`` runs the PyTorch reference path on fp32
tensors of bf16-representable values, ``cuda`` the HIP kernels on bf16 (or fp32) tensors.

Definition (``eps`` = label smoothing, ``w`` = weights)::

    effw_r = w_r, 0 for an ignored row (label outside [0, K) or w_r == 0)
    loss_r = lse_r - (1 - eps) x[r, label_r] - (eps / K) sum_k x[r, k]          (0 for an ignored row)
    value  = sum_r effw_r loss_r / den,  den = 1 | N | sum effw | #{effw != 0}   (0 when den == 0)
    dx[r, k] = c_r (softmax(x_r)[k] - (1 - eps) [k == label_r] - eps / K),  c_r = upstream effw_r / den

Bounds (``U = 2^-24``; ``chain`` = the longest path of a row's sums, ``_chain``):

* row loss ``e_r``: ``nhwc_helpers.lse_bound``'s ``e_lse``; the fp32 sum of the K logits, ``gamma(chain + 3)``
  relative to ``(eps / K) sum|x_k|`` (the sum, ``eps / K`` and their product); three roundings (the product with
  ``1 - eps`` and the two subtractions) of ``|lse| + |x_label| + (eps / K) |sum x|``.
* reduced value: the rows' errors through the exact (fp64) weighted sum, ``sum effw_r e_r / den``, plus the one
  rounding of the result to fp32.  ``NONE``: ``effw_r e_r`` plus the rounding of the product.
* gradient: ``c_r`` is the fp32 product ``upstream * (1 / den) * effw_r`` of fp32-rounded factors: at most three
  roundings, ``gamma(3)`` relative to the gradient.  ``eps == 0`` and bf16 logits: ``check_neighbour`` at its 1 % cap
  (an error of a few U moves one element in thousands).  ``eps == 0`` and fp32 logits: the fp32 bound of
  ``test_nhwc_kernels._xent`` plus that ``gamma(3)``.  ``eps > 0``: ``p - eps / K`` cancels where ``p`` is about
  ``eps / K``, so the bound is absolute: ``|c_r|`` times the fp32 bound on ``p``, plus ``gamma(3)`` (two subtractions
  and the product) and the ``gamma(3)`` of ``c_r`` on the magnitudes ``|c_r| (p + (1 - eps) [k == label] + eps / K)``;
  ``out_bound`` adds the rounding to bf16.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import mdtf
from mdtf import losses as L
from mdtf.ops import _native
from mdtf.ops import losses as OL

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import U, gamma  # noqa: E402

R = L.Reduction
DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
WEIGHTS = [1.0, 0.0, 2.5, 1.0, 0.5]
UPSTREAM = -1.5                   # the scalar handed to backward() of a reduced loss


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _chain(K):
    # a lane's K / 64 terms (one wave per row; the row kernels' 256 threads have fewer), each an add and, in the
    # online form, a rescale; then 6 + 4 merges of three roundings each
    return 2 * -(-K // 64) + 30


def _case(n, K, seed):
    """``NH.xent_case(n, K, seed)``; below K = 5 (its third row puts a peak in column 4) rows of two-row cases."""
    if K >= 5:
        return NH.xent_case(n, K, seed)
    parts = [NH.xent_case(2, K, seed + 10 * i) for i in range(-(-n // 2))]
    return tuple(torch.cat([p[j] for p in parts])[:n] for j in range(3))


def _weights(n):
    return torch.tensor((WEIGHTS * -(-n // 5))[:n], dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------ oracle
def oracle(x, labels, w, eps, reduction, upstream, den_eps=0.0):
    """fp64.  x [N, K], labels [N], w [N]; upstream: a float (reduced forms) or [N] (NONE).  Extends ``NH.xent_ref``
    with eps, weights, ignored rows and the reductions."""
    n, k = x.shape
    valid = (labels >= 0) & (labels < k)
    effw = torch.where(valid, w, torch.zeros_like(w))
    live = effw != 0
    xs = torch.where(live[:, None], x, torch.zeros_like(x))
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    lse, _, _, p = NH.xent_ref(xs, lab, torch.ones(n, dtype=torch.float64))
    xl = xs.gather(1, lab[:, None]).squeeze(1)
    zero = torch.zeros_like(lse)
    st = (eps / k) * xs.sum(1) if eps > 0 else zero          # eps == 0: no smoothing term, also for a -inf logit
    loss = torch.where(live, lse - (1.0 - eps) * xl - st, zero)
    # bound of the fp32 row loss
    e_lse, _ = NH.lse_bound(xs, lab, lse, _chain(k))
    e_row = e_lse + 3 * U * (lse.abs() + xl.abs() + st.abs())
    if eps > 0:
        e_row = e_row + gamma(_chain(k) + 3) * (eps / k) * xs.abs().sum(1)
    e_row = torch.where(live, e_row, zero)
    if reduction == R.NONE:
        value = effw * loss
        e_value = effw.abs() * e_row + U * value.abs() + NH.TINY
        c = upstream * effw
        inv = 1.0
    else:
        den = {R.SUM: 1.0, R.SUM_OVER_BATCH_SIZE: float(n), R.MEAN: float(effw.sum()),
               R.SUM_BY_NONZERO_WEIGHTS: float(live.sum())}[reduction] + den_eps
        inv = 0.0 if den == 0 else 1.0 / den
        value = (effw * loss).sum() * inv
        e_value = (effw.abs() * e_row).sum() * abs(inv) + U * value.abs() + NH.TINY
        c = upstream * inv * effw
    onehot = torch.zeros_like(x).scatter_(1, lab[:, None], 1.0)
    dl = torch.where(live[:, None], c[:, None] * (p - (1.0 - eps) * onehot - eps / k), torch.zeros_like(x))
    # fp32 bound on p = exp(x - lse): as test_nhwc_kernels._xent
    a = (xs - lse[:, None]).abs()
    e_p = p * (e_lse[:, None] + NH.INTRINSIC_FACTOR * U * (1.4427 * a + 2.0))
    mag = c.abs()[:, None] * (p + (1.0 - eps) * onehot + eps / k)
    return dict(loss=loss, e_row=e_row, value=value, e_value=e_value, dl=dl, c=c, e_p=e_p, mag=mag, live=live,
                lab=lab, valid=valid, inv=inv)


def check_grad(got, o, eps, bf16_logits, bf16_out, what):
    live = o["live"]
    assert not bool(got[~live].any()), what + ": gradient rows of ignored examples are not exact zeros"
    if eps == 0 and bf16_logits:
        NH.check_neighbour(got, o["dl"], what)
    elif eps == 0:
        NH.check_bound(got, o["dl"], o["c"].abs()[:, None] * o["e_p"] * (1 + 4 * U)
                       + (gamma(2) + gamma(3)) * o["dl"].abs() + NH.TINY, what)
    else:
        acc = o["c"].abs()[:, None] * o["e_p"] * (1 + 4 * U) + 2 * gamma(3) * o["mag"]
        NH.check_bound(got, o["dl"], NH.out_bound(o["dl"], acc, bf16_out), what)


# ------------------------------------------------------------------------------------------------------ runner
def _layout(x, device, dtype, ld, offset):
    """The logits as a [N, K] view of a leaf buffer of row stride ld that starts ``offset`` elements in."""
    n, k = x.shape
    buf = torch.zeros(n * ld + offset, dtype=dtype, device=device)
    with torch.no_grad():
        buf[offset:].view(n, ld)[:, :k].copy_(x)
    buf.requires_grad_(True)
    return buf, buf[offset:].view(n, ld)[:, :k]


def run(device, x, labels, w, eps, reduction, dloss, bf16_logits=True, ld=None, offset=0, den_eps=0.0):
    """value and d(buffer) of ``sparse_softmax_cross_entropy`` on the layout; returns (value, grad [N, ld], base of the
    gradient handed to the logits view, loss tensor)."""
    n, k = x.shape
    ld = k if ld is None else ld
    dtype = torch.bfloat16 if (device == "cuda" and bf16_logits) else torch.float32
    buf, view = _layout(x, device, dtype, ld, offset)
    seen = []
    view.register_hook(lambda g: seen.append(g))
    loss = L.sparse_softmax_cross_entropy(labels.to(device), view, weights=w.to(device) if w is not None else 1.0,
                                          reduction=reduction, label_smoothing=eps, denominator_epsilon=den_eps)
    if reduction == R.NONE:
        loss.backward(dloss.to(device))
    else:
        loss.backward(torch.tensor(UPSTREAM, device=device))
    return loss.detach(), buf.grad[offset:].view(n, ld), seen[0], loss


def sweep(device, x, labels, w, eps, dloss, bf16_logits=True, ld=None, offset=0, reductions=None, what=""):
    n, k = x.shape
    gpu = device == "cuda"
    ldv = k if ld is None else ld
    what = "%s/%s K=%d ld=%d off=%d eps=%g %s" % (device, "bf16" if bf16_logits else "fp32", k, ldv, offset, eps, what)
    for reduction in reductions or R.all():
        tag = "%s %s" % (what, reduction)
        up = dloss.double() if reduction == R.NONE else UPSTREAM
        o = oracle(x.double(), labels, w.double(), eps, reduction, up)
        value, grad, g_view, _ = run(device, x, labels, w, eps, reduction, dloss, bf16_logits, ld, offset)
        assert value.dtype == torch.float32
        NH.check_bound(value, o["value"], o["e_value"], tag + " value")
        assert not bool(grad[:, k:].any()), tag + ": pad columns of the gradient"
        check_grad(grad[:, :k], o, eps, bf16_logits, gpu and bf16_logits, tag + " dlogits")
        if gpu and ldv != k and bf16_logits and ldv % 8 == 0:
            base = g_view._base
            assert base is not None and tuple(base.shape) == (n, ldv), tag + ": gradient is no view of padded rows"
            assert not bool(base[:, k:].any()), tag + ": pad columns behind the returned view"
    if not gpu:
        # a correct fp32 implementation meets the row bound: PyTorch's own smoothed cross entropy
        o = oracle(x.double(), labels, torch.ones(n, dtype=torch.float64), eps, R.NONE, torch.ones(n).double())
        ce = F.cross_entropy(x, o["lab"], label_smoothing=eps, reduction="none").double()
        ce = torch.where(o["valid"], ce, torch.zeros_like(ce))
        NH.check_bound(ce, o["loss"], o["e_row"] + NH.TINY, what + " F.cross_entropy rows")


CONTIG_K = [2, 10, 65, 1000, 2048, 2050, 8200]


@pytest.mark.parametrize("oor", [False, True], ids=["labels-in-range", "row3-label-K"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", CONTIG_K)
@pytest.mark.parametrize("device", DEVICES)
def test_sparse_contiguous(device, K, eps, oor):
    """2: the smallest row | 10: lanes without a term | 65: one lane with two | 1000: the one-wave kernel's batches of
    four | 2048: the row kernels' threshold, one vector per thread | 2050: the pair kernel | 8200: the
    four-loads-in-flight loops and their tails"""
    device = _device(device)
    x, labels, dloss = _case(5, K, 2000 + K)
    if oor:
        labels = labels.clone()
        labels[3] = K
    sweep(device, x, labels, _weights(5), eps, dloss)


# 2052 of 2056: a v8 row whose last vector is half masked | 8199 of 8208: odd K on the v8 kernels, 7 of the last
# vector's 8 live, a whole vector of pad to zero
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K,ld", [(2052, 2056), (8199, 8208)])
@pytest.mark.parametrize("device", DEVICES)
def test_sparse_strided_rows(device, K, ld, eps):
    device = _device(device)
    x, labels, dloss = _case(5, K, 2100 + K)
    labels[3] = K
    sweep(device, x, labels, _weights(5), eps, dloss, ld=ld)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("device", DEVICES)
def test_sparse_two_byte_offset_view(device, eps):
    """Rows that start 2 bytes past a 4-byte boundary: the one-wave forward and the generic backward, which stores
    the pad columns of the [N, 1008] gradient itself."""
    device = _device(device)
    x, labels, dloss = _case(5, 1000, 2200)
    sweep(device, x, labels, _weights(5), eps, dloss, ld=1008, offset=1)


# (K, ld, first masked column, one past the last), as test_nhwc_kernels.XENT_MASKED: the first 16-byte vector of every
# thread of the v8 kernel | the first pair of threads 0-7 of the pair kernel | the first vector of threads 0-1 of the
# v8 kernel on a strided row | the one-wave kernel
MASKED = [(8200, 8200, 0, 2048), (2050, 2050, 0, 16), (2050, 2056, 0, 16), (1000, 1000, 0, 16)]


@pytest.mark.parametrize("K,ld,lo,hi", MASKED)
@pytest.mark.parametrize("device", DEVICES)
def test_sparse_masked_classes(device, K, ld, lo, hi):
    """Classes a caller masked out are -inf: a thread whose first pair / vector is all -inf must not accumulate
    exp(-inf - (-inf)) = NaN, and without smoothing no 0 * (-inf) is formed either."""
    device = _device(device)
    x, labels, dloss = _case(5, K, 3000 + K)
    x[:, lo:hi] = float("-inf")
    x[:, hi] = x[:, hi].abs() + 3.0
    labels = torch.tensor([hi, K - 1, (K // 2) | 1, K - 2, hi + 1])
    sweep(device, NH.bf16_exact(x), labels, _weights(5), 0.0, dloss, ld=ld, reductions=[R.MEAN, R.NONE],
          what="masked [%d,%d)" % (lo, hi))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("device", DEVICES)
def test_sparse_fp32_logits(device, eps):
    device = _device(device)
    x, labels, dloss = _case(5, 1000, 2300)
    gen = torch.Generator().manual_seed(1000)
    x = x + torch.rand(x.shape, generator=gen) * 2.0 ** -6       # not bf16-representable
    labels[3] = 1000
    sweep(device, x, labels, _weights(5), eps, dloss, bf16_logits=False)


@pytest.mark.parametrize("device", DEVICES)
def test_sparse_backward_second_grid_stride_trip(device):
    """513 rows of 2049 (odd: no vector path): 4096 * 256 + 2561 elements, a second trip of the generic backward's
    grid-stride loop, and more rows than the reduction's 256 threads."""
    device = _device(device)
    x, labels, dloss = _case(513, 2049, 2400)
    labels[3] = 2049
    sweep(device, x, labels, _weights(513), 0.1, dloss, reductions=[R.MEAN, R.NONE])


@pytest.mark.parametrize("device", DEVICES)
def test_sparse_rank3_logits_are_flattened(device):
    device = _device(device)
    K = 10
    x, labels, dloss = _case(6, K, 2500)
    w = _weights(6)
    xd = NH.put(x, device).view(2, 3, K).requires_grad_(True)
    for reduction in (R.NONE, R.SUM_BY_NONZERO_WEIGHTS):
        o = oracle(x.double(), labels, w.double(), 0.1, reduction, dloss.double() if reduction == R.NONE else 1.0)
        xd.grad = None
        loss = L.sparse_softmax_cross_entropy(labels.view(2, 3).to(device), xd, weights=w.view(2, 3).to(device),
                                              reduction=reduction, label_smoothing=0.1)
        if reduction == R.NONE:
            assert tuple(loss.shape) == (2, 3)
            loss.backward(dloss.view(2, 3).to(device))
            NH.check_bound(loss.detach().reshape(-1), o["value"], o["e_value"], "rank 3 rows")
        else:
            assert loss.dim() == 0
            loss.backward()
            NH.check_bound(loss.detach(), o["value"], o["e_value"], "rank 3 value")
        assert tuple(xd.grad.shape) == (2, 3, K)
        check_grad(xd.grad.reshape(6, K), o, 0.1, True, device == "cuda", "%s rank 3 %s dlogits" % (device, reduction))


# ------------------------------------------------------------------------------------------------ ignored rows
@pytest.mark.parametrize("K,ld", [(1000, 1000), (2052, 2056), (2049, 2049)])
@pytest.mark.parametrize("device", DEVICES)
def test_ignored_rows_are_not_read(device, K, ld):
    """A zero-weight row and a row whose label is out of range hold NaN: loss and the other rows' gradients keep
    their bits, the two rows' gradients are exact zeros, and so are the pad columns."""
    device = _device(device)
    x, labels, dloss = _case(5, K, 2600 + K)
    labels[3] = K
    w = _weights(5)
    xn = x.clone()
    xn[1] = float("nan")
    xn[3] = float("nan")
    for reduction in (R.MEAN, R.NONE):
        v0, g0, _, _ = run(device, x, labels, w, 0.1, reduction, dloss, ld=ld)
        v1, g1, _, _ = run(device, xn, labels, w, 0.1, reduction, dloss, ld=ld)
        assert bool(torch.isfinite(v1).all()) and bool(torch.isfinite(g1).all()), reduction
        assert NH.bits_equal(v0, v1), reduction
        assert NH.bits_equal(g0, g1), reduction
        assert not bool(g1[1].any()) and not bool(g1[3].any())
        assert bool(g1[0, :K].any()) and bool(g1[2, :K].any()) and bool(g1[4, :K].any())
        assert not bool(g1[:, K:].any())


# ------------------------------------------------------------------------------------------------ API semantics
def _small():
    x, labels, dloss = _case(5, 10, 2700)
    return x, labels, dloss, _weights(5)


def test_reduction_names_are_tf1():
    assert (R.NONE, R.SUM, R.MEAN, R.SUM_OVER_BATCH_SIZE, R.SUM_BY_NONZERO_WEIGHTS) == (
        "none", "weighted_sum", "weighted_mean", "weighted_sum_over_batch_size", "weighted_sum_by_nonzero_weights")
    assert mdtf.losses is L
    with pytest.raises(ValueError):
        L.sparse_softmax_cross_entropy(torch.zeros(2, dtype=torch.long), torch.zeros(2, 3), reduction="mean")


@pytest.mark.parametrize("reduction", R.all())
def test_scalar_weight(reduction):
    """weights=0.5 is a weight of 0.5 on every row (and [N, 1] weights are [N] weights)."""
    x, labels, dloss, _ = _small()
    half = torch.full((5,), 0.5, dtype=torch.float64)
    up = dloss.double() if reduction == R.NONE else 1.0
    o = oracle(x.double(), labels, half, 0.1, reduction, up)
    for weights in (0.5, half.float().view(5, 1)):
        xd = x.clone().requires_grad_(True)
        loss = L.sparse_softmax_cross_entropy(labels, xd, weights=weights, reduction=reduction, label_smoothing=0.1)
        loss.backward(dloss if reduction == R.NONE else None)
        NH.check_bound(loss.detach(), o["value"], o["e_value"], "scalar weight %s value" % reduction)
        check_grad(xd.grad, o, 0.1, True, False, "scalar weight %s dlogits" % reduction)


@pytest.mark.parametrize("reduction", R.all())
def test_all_zero_weights_give_zero(reduction):
    x, labels, dloss, _ = _small()
    for weights in (torch.zeros(5), 0.0):
        xd = x.clone().requires_grad_(True)
        loss = L.sparse_softmax_cross_entropy(labels, xd, weights=weights, reduction=reduction)
        loss.backward(dloss if reduction == R.NONE else None)
        assert not bool(loss.detach().any()) and bool(torch.isfinite(loss).all())
        assert not bool(xd.grad.any())


def test_loss_collection():
    from mdtf.train import variables as V
    x, labels, _, w = _small()
    V.reset_default_graph()
    L.sparse_softmax_cross_entropy(labels, x, w)
    L.softmax_cross_entropy(F.one_hot(labels, 10), x, w)
    assert V.get_collection("losses") == []
    a = L.sparse_softmax_cross_entropy(labels, x, w, loss_collection="losses")
    assert [id(t) for t in V.get_collection("losses")] == [id(a)]
    b = L.softmax_cross_entropy(F.one_hot(labels, 10), x, w, loss_collection=V.GraphKeys.LOSSES)
    assert [id(t) for t in V.get_collection("losses")] == [id(a), id(b)]
    V.reset_default_graph()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("reduction", R.all())
def test_dense_form_equals_sparse(device, reduction):
    """softmax_cross_entropy(one_hot, label_smoothing=0.1) is the sparse form: value within the sparse bound plus the
    dense expression's own sum over K (gamma(K + 2) of sum_k |t_k log p_k|); gradient within the eps > 0 bound, whose
    p term also carries the fp32 sum of the K targets that log_softmax's backward multiplies it with (gamma(K))."""
    device = _device(device)
    x, labels, dloss, w = _small()
    up = dloss.double() if reduction == R.NONE else UPSTREAM
    o = oracle(x.double(), labels, w.double(), 0.1, reduction, up)
    xd = x.to(device).requires_grad_(True)          # fp32 logits on both devices: the dense rows are a torch expression
    loss = L.softmax_cross_entropy(F.one_hot(labels, 10).to(device), xd, weights=w.to(device), label_smoothing=0.1,
                                   reduction=reduction)
    loss.backward(dloss.to(device) if reduction == R.NONE else torch.tensor(UPSTREAM, device=device))
    x64 = x.double()
    logp = x64 - torch.logsumexp(x64, 1, keepdim=True)
    t = F.one_hot(labels, 10).double() * 0.9 + 0.01
    e_dense = gamma(10 + 2) * (t * logp).abs().sum(1) * w.double()
    extra = e_dense if reduction == R.NONE else e_dense.sum() * abs(o["inv"])
    NH.check_bound(loss.detach(), o["value"], o["e_value"] + extra, "%s dense %s value" % (device, reduction))
    acc = o["c"].abs()[:, None] * o["e_p"] * (1 + 4 * U) + (2 * gamma(3) + gamma(10 + 2)) * o["mag"]
    NH.check_bound(xd.grad, o["dl"], NH.out_bound(o["dl"], acc, False), "%s dense %s dlogits" % (device, reduction))


def test_label_smoothing_flag_reaches_the_loss():
    from mdtf.config.flags import FLAGS
    from mdtf.models import SoftmaxCrossEntropyLoss
    x, labels, _, _ = _small()
    assert SoftmaxCrossEntropyLoss().label_smoothing == 0.0
    plain = SoftmaxCrossEntropyLoss().loss(x, labels)
    old = FLAGS.label_smoothing
    FLAGS.label_smoothing = 0.1
    try:
        crit = SoftmaxCrossEntropyLoss()
    finally:
        FLAGS.label_smoothing = old
    assert abs(crit.label_smoothing - 0.1) < 1e-12
    assert SoftmaxCrossEntropyLoss(0.0).label_smoothing == 0.0        # an argument wins over the flag
    o = oracle(x.double(), labels, torch.ones(5, dtype=torch.float64), 0.1, R.SUM_OVER_BATCH_SIZE, 1.0)
    got = crit.loss(x, labels)
    NH.check_bound(got, o["value"], o["e_value"], "flag-built smoothed loss")
    assert float(got) != float(plain)


class _SpyLoss(object):
    """Mixin: records (predict, ground truth, loss) of every call."""

    def loss(self, predict, ground_truth):
        out = super(_SpyLoss, self).loss(predict, ground_truth)
        det = tuple(p.detach().clone() for p in predict) if isinstance(predict, tuple) else predict.detach().clone()
        self.calls = getattr(self, "calls", []) + [(det, ground_truth.detach().clone(), out.detach().clone())]
        return out


def _bert_tiny(dev, dt, hip_graph, steps, spy=False, hook=None, P=5, vocab=1000, batch=8, seq=32):
    from mdtf.models import Bert, BertPretrainingLoss, SyntheticBertLoader
    from mdtf.runtime import Net, Tower
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device = torch.device(dev)
    store.compute_dtype = dt
    store.generator.manual_seed(7)
    ld = SyntheticBertLoader(seq_len=seq, max_predictions=P, vocab=vocab, seed=3, variable_predictions=True)
    ld.batch_size = batch
    raw, gt = ld.load_train_batch()
    base = mdtf.train.GradientDescentOptimizer(0.05)
    cls = type("SpyBertLoss", (_SpyLoss, BertPretrainingLoss), {}) if spy else BertPretrainingLoss
    crit = cls(P, weighted=True)
    if hook is not None:
        inner = crit.loss
        crit.loss = lambda predict, ground_truth: inner(hook(predict), ground_truth)
    tg = []
    t = Tower(Net(Bert("tiny", vocab_size=vocab, seq_len=seq, max_predictions=P, dropout=0.0)), "tower_0/", tg, raw, gt,
              crit, base, batch_size=batch)
    _, loss, _ = t.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, hip_graph=hip_graph)
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    ls = [sess.run([op, loss])[1] for _ in range(steps)]
    ls = [float(v) for v in ls]
    weights = {v.name: v.value().detach().float().cpu().clone() for v in store.trainable_variables()}
    return ls, weights, op, crit, ld


def test_synthetic_loader_variable_predictions():
    from mdtf.models import SyntheticBertLoader
    from mdtf.train import variables as V
    V.reset_default_graph()
    P = 6
    plain = SyntheticBertLoader(16, P, vocab=1000, seed=5)
    var = SyntheticBertLoader(16, P, vocab=1000, seed=5, variable_predictions=True)
    plain.batch_size = var.batch_size = 64
    (raw0, gt0), (raw1, gt1) = plain._make(), var._make()
    assert tuple(gt0.shape) == (64, P + 1) and tuple(gt1.shape) == (64, 2 * P + 1)
    assert torch.equal(raw0, raw1) and torch.equal(gt0[:, P], gt1[:, P])
    w = gt1[:, P + 1:]
    count = w.sum(1)
    assert set(w.unique().tolist()) <= {0, 1} and int(count.min()) >= 1 and int(count.max()) <= P
    assert len(count.unique()) > 1
    assert torch.equal(w, (torch.arange(P)[None, :] < count[:, None]).long())         # padding at the end
    assert torch.equal(gt1[:, :P], gt0[:, :P] * w)                                     # padding ids are 0
    assert torch.equal(var._make()[1], gt1)                                            # seeded


def test_weighted_bert_loss_is_the_recipe():
    """BertPretrainingLoss(P, weighted=True) on a BERT-tiny forward = sum(w l) / (sum(w) + 1e-5) + mean(nsp), written
    out in fp64 on the recorded logits; the bound is the two reduced values' (chain of K = 1000, and of K = 2)."""
    P = 5
    ls, _, _, crit, _ = _bert_tiny("cpu", None, False, 1, spy=True, P=P)
    (mlm, nsp), gt, got = crit.calls[-1]
    assert float(got) == ls[0]
    assert tuple(gt.shape) == (8, 2 * P + 1) and tuple(mlm.shape) == (8 * P, 1000)
    ids, w = gt[:, :P].reshape(-1), gt[:, P + 1:].reshape(-1).double()
    assert 0 < int((w == 0).sum()) < w.numel()
    x = mlm.double()
    l = torch.logsumexp(x, 1) - x.gather(1, ids[:, None]).squeeze(1)
    n64 = nsp.double()
    l2 = (torch.logsumexp(n64, 1) - n64.gather(1, gt[:, P][:, None]).squeeze(1)).mean()
    want = (w * l).sum() / (w.sum() + 1e-5) + l2
    o1 = oracle(x, ids, w, 0.0, R.MEAN, 1.0, den_eps=1e-5)
    o2 = oracle(n64, gt[:, P], torch.ones(8, dtype=torch.float64), 0.0, R.SUM_OVER_BATCH_SIZE, 1.0)
    assert abs(float(o1["value"] + o2["value"]) - float(want)) <= 1e-12 * abs(float(want))
    bound = float(o1["e_value"] + o2["e_value"]) + U * abs(float(want))       # and the fp32 sum of the two
    assert abs(float(got) - float(want)) <= bound, (float(got), float(want), bound)
    # the unweighted loss of the same logits trains on the padding: a different number
    print("weighted %.9g unweighted %.9g bound %.3g" % (float(want), float(l.mean() + l2), bound))
    assert abs(float(l.mean() + l2) - float(want)) > bound


# ===================================================================================================== GPU only
def _raw(name, *args):
    _native.check(_native.fn(name)(*args, _native.stream_ptr()), name)
    torch.cuda.synchronize()


def _p(g):
    return _native.ptr(g.t if isinstance(g, NH.Guarded) else g)


@pytest.mark.gpu
@pytest.mark.parametrize("K,ld,offset", [(1000, 1000, 0), (2048, 2048, 0), (2052, 2056, 0), (1000, 1008, 1)])
def test_raw_entry_points_on_guarded_buffers(K, ld, offset):
    """mdtf_xent_w_fwd / mdtf_loss_reduce / mdtf_xent_w_bwd with every buffer between sentinel guard bands: guards
    intact, inputs unchanged, every output element stored (the pad columns as zeros), values within the bounds."""
    device = _device("cuda")
    n, eps = 5, 0.1
    x, labels, dloss = _case(n, K, 2800 + K)
    labels[3] = K
    w = _weights(n)
    what = "raw K=%d ld=%d off=%d" % (K, ld, offset)
    flat = torch.zeros(n * ld + offset + (8 - offset) % 8, dtype=torch.bfloat16)
    flat[offset:offset + n * ld].view(n, ld)[:, :K].copy_(x)
    g_x = NH.Guarded(flat, device)
    src = g_x.t[offset:offset + n * ld].view(n, ld)[:, :K]
    g_lab, g_w = NH.Guarded(labels, device), NH.Guarded(w, device)
    g_loss, g_lse, g_effw = (NH.Guarded(None, device, torch.float32, (n,)) for _ in range(3))
    _raw("mdtf_xent_w_fwd", _native.ptr(src), 1, _p(g_lab), _p(g_w), 1.0, n, K, ld, eps, 0, _p(g_loss), _p(g_lse),
         _p(g_effw))
    NH.assert_contained(what + " fwd", [g_x, g_lab, g_w], [g_loss, g_lse, g_effw])
    o = oracle(x.double(), labels, w.double(), eps, R.MEAN, UPSTREAM)
    NH.check_bound(g_loss.t, o["loss"], o["e_row"] + NH.TINY, what + " rows")
    assert torch.equal(g_effw.t.cpu(), torch.tensor([1.0, 0.0, 2.5, 0.0, 0.5]))
    assert float(g_lse.t[1]) == 0.0 and float(g_lse.t[3]) == 0.0
    g_out = NH.Guarded(None, device, torch.float32, (2,))
    g_loss_in, g_effw_in = NH.Guarded(g_loss.t, device), NH.Guarded(g_effw.t, device)
    _raw("mdtf_loss_reduce", _p(g_loss_in), _p(g_effw_in), n, OL.MEAN, 0.0, 1.0, _p(g_out))
    NH.assert_contained(what + " reduce", [g_loss_in, g_effw_in], [g_out])
    NH.check_bound(g_out.t[0], o["value"], o["e_value"], what + " value")
    NH.check_bound(g_out.t[1], torch.tensor(0.25, dtype=torch.float64), U * 0.25, what + " 1 / den")
    ldo = ld if (ld != K and ld % 8 == 0) else K
    g_dl = NH.Guarded(None, device, torch.bfloat16, (n, ldo))
    g_lse_in, g_up = NH.Guarded(g_lse.t, device), NH.Guarded(torch.tensor([UPSTREAM]), device)
    g_coef = NH.Guarded(g_out.t, device)
    _raw("mdtf_xent_w_bwd", _native.ptr(src), 1, _p(g_lab), _p(g_lse_in), _p(g_effw_in), _native.ptr(g_coef.t[1:]),
         _p(g_up), _p(g_dl), n, K, ld, ldo, eps)
    NH.assert_contained(what + " bwd", [g_x, g_lab, g_lse_in, g_effw_in, g_coef, g_up], [g_dl])
    assert not bool(g_dl.t[:, K:].any()), what + ": pad columns"
    check_grad(g_dl.t[:, :K], o, eps, True, True, what + " dlogits")
    # Reduction.NONE: one upstream value per row, no coefficient
    g_dl2 = NH.Guarded(None, device, torch.bfloat16, (n, ldo))
    g_dloss = NH.Guarded(dloss, device)
    _raw("mdtf_xent_w_bwd", _native.ptr(src), 1, _p(g_lab), _p(g_lse_in), _p(g_effw_in), _native.ptr(None), _p(g_dloss),
         _p(g_dl2), n, K, ld, ldo, eps)
    NH.assert_contained(what + " bwd rows", [g_x, g_lab, g_lse_in, g_effw_in, g_dloss], [g_dl2])
    o2 = oracle(x.double(), labels, w.double(), eps, R.NONE, dloss.double())
    assert not bool(g_dl2.t[:, K:].any()), what + ": pad columns (rows)"
    check_grad(g_dl2.t[:, :K], o2, eps, True, True, what + " dlogits (rows)")


@pytest.mark.gpu
def test_loss_reduce_modes_and_div_no_nan():
    device = _device("cuda")
    rows = torch.tensor([1.5, 2.0, -3.0, 0.25], device=device)
    effw = torch.tensor([1.0, 0.0, 2.0, 0.5], device=device)
    num = 1.5 - 6.0 + 0.125
    for mode, den in ((OL.SUM, 1.0), (OL.SUM_OVER_BATCH_SIZE, 4.0), (OL.MEAN, 3.5), (OL.SUM_BY_NONZERO_WEIGHTS, 3.0)):
        out = OL._reduce_native(rows, effw, mode, 0.5, 2.0).cpu().double()
        want = torch.tensor([2.0 * num / (den + 0.5), 2.0 / (den + 0.5)], dtype=torch.float64)
        NH.check_bound(out, want, U * want.abs(), "reduce mode %d" % mode)
    zeros = torch.zeros(4, device=device)
    for mode in (OL.MEAN, OL.SUM_BY_NONZERO_WEIGHTS):
        assert not bool(OL._reduce_native(rows, zeros, mode, 0.0, 1.0).any())


@pytest.mark.gpu
@pytest.mark.parametrize("K,ld,offset", [(1000, 1000, 0), (8199, 8208, 0), (1000, 1008, 1)])
def test_bitwise_repeatable(K, ld, offset):
    device = _device("cuda")
    x, labels, dloss = _case(5, K, 2900 + K)
    w = _weights(5)
    for reduction in (R.MEAN, R.NONE):
        a = run(device, x, labels, w, 0.1, reduction, dloss, ld=ld, offset=offset)
        b = run(device, x, labels, w, 0.1, reduction, dloss, ld=ld, offset=offset)
        assert NH.bits_equal(a[0], b[0]) and NH.bits_equal(a[1], b[1])
        if reduction == R.MEAN:                   # out = {value, scale / den}: the reduced loss is a view of it
            assert a[3]._base is not None and a[3]._base.numel() == 2
            assert NH.bits_equal(a[3]._base.detach(), b[3]._base.detach())


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


def _run_resnetish(batches, hip_graph, spy=False):
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
    base = mdtf.train.MomentumOptimizer(lambda step: 0.05 / (1 + step), 0.9, weight_decay=1e-4)
    tg = []
    M = type("TinyResModel", (_TinyRes, Model), {})
    cls = type("SpySmoothedLoss", (_SpyLoss, SoftmaxCrossEntropyLoss), {}) if spy else SoftmaxCrossEntropyLoss
    crit = cls(label_smoothing=0.1)
    t = Tower(Net(M()), "tower_0/", tg, xp, yp, crit, base, batch_size=x0.shape[0])
    _, loss, _ = t.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, hip_graph=hip_graph, bucket_bytes=1 << 18)
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    losses = []
    for x, y in batches:
        _, lv = sess.run([op, loss], feed_dict={xp: x, yp: y})
        losses.append(lv)
    losses = [float(v) for v in losses]
    weights = {v.name: v.value().detach().float().cpu().clone() for v in store.trainable_variables()}
    return losses, weights, op, crit


@pytest.mark.gpu
def test_hip_graph_smoothed_resnet_step_bitwise_equals_eager(monkeypatch):
    """Four steps of the tiny ResNet with SoftmaxCrossEntropyLoss(label_smoothing=0.1): the captured step replays the
    loss kernels (nothing reads the denominator back), losses and final weights equal the eager run's bit for bit.

    The first step's loss is also compared with ``MDTF_KERNELS=torch``.  A whole step under that setting runs other
    convolution and BatchNorm kernels, whose bf16 logits differ from the native ones by far more than any bound on
    the loss, so the comparison is made where it says something about the loss: on the logits the native first step
    produced, both paths lie within the reduced value's bound of the fp64 oracle."""
    _device("cuda")
    torch.manual_seed(0)
    batches = [(torch.randn(16, 16, 16, 8), torch.randint(0, 16, (16,))) for _ in range(4)]
    _native.set_deterministic(True)
    try:
        l_e, w_e, _, crit = _run_resnetish(batches, hip_graph=False, spy=True)
        l_g, w_g, op, _ = _run_resnetish(batches, hip_graph=True)
    finally:
        _native.set_deterministic(False)
    g = op.graph
    assert g is not None and g.graph is not None and g.replays == 2 and g.fallbacks == 0, vars(g)
    assert l_e == l_g, (l_e, l_g)
    for k in w_e:
        assert torch.equal(w_e[k], w_g[k]), k
    logits, labels, got = crit.calls[-4]
    assert float(got) == l_e[0] and logits.dtype == torch.bfloat16
    o = oracle(logits.double().cpu(), labels.cpu(), torch.ones(16, dtype=torch.float64), 0.1, R.SUM_OVER_BATCH_SIZE,
               1.0)
    NH.check_bound(got, o["value"], o["e_value"], "first step, native")
    from mdtf.models import SoftmaxCrossEntropyLoss
    monkeypatch.setenv("MDTF_KERNELS", "torch")
    ref = SoftmaxCrossEntropyLoss(label_smoothing=0.1).loss(logits, labels)
    monkeypatch.delenv("MDTF_KERNELS")
    NH.check_bound(ref, o["value"], o["e_value"], "first step, MDTF_KERNELS=torch")
    assert abs(float(ref) - float(got)) <= 2 * float(o["e_value"])


@pytest.mark.gpu
def test_hip_graph_weighted_bert_step_bitwise_equals_eager():
    """BERT-tiny with the weighted masked-LM loss: the captured step (weights, denominator and the upstream gradient
    stay on the device) equals the eager one bit for bit in deterministic mode."""
    _device("cuda")
    _native.set_deterministic(True)
    try:
        l_e, w_e, _, _, _ = _bert_tiny("cuda", torch.bfloat16, False, 4)
        l_g, w_g, op, _, _ = _bert_tiny("cuda", torch.bfloat16, True, 4)
    finally:
        _native.set_deterministic(False)
    g = op.graph
    assert g is not None and g.graph is not None and g.replays == 2 and g.fallbacks == 0, vars(g)
    assert l_e == l_g, (l_e, l_g)
    assert all(v == v for v in l_e)
    for k in w_e:
        assert torch.equal(w_e[k], w_g[k]), k


@pytest.mark.gpu
def test_tied_decoder_gets_the_padded_gradient():
    """The MLM logits reach the op as the [rows, vocab] view of the decoder's padded rows; the gradient goes back as
    the same view of a buffer whose pad columns are zero, which the decoder's backward then reads whole."""
    _device("cuda")
    from mdtf.ops import gemm
    vocab = 1000
    vp = vocab + gemm.decoder_pad_rows(vocab)
    assert vp > vocab and vp % 8 == 0
    seen = {}

    def hook(predict):
        mlm, nsp = predict
        if mlm.requires_grad:
            seen["logits"] = (tuple(mlm.shape), mlm.stride(), mlm.dtype)
            mlm.register_hook(lambda grad: seen.__setitem__("grad", grad))
        return predict
    ls, _, _, _, _ = _bert_tiny("cuda", torch.bfloat16, False, 1, hook=hook, vocab=vocab)
    assert ls[0] == ls[0]
    assert seen["logits"] == ((8 * 5, vocab), (vp, 1), torch.bfloat16), seen["logits"]
    grad = seen["grad"]
    base = grad._base
    assert base is not None and tuple(base.shape) == (8 * 5, vp) and base.data_ptr() == grad.data_ptr()
    assert tuple(grad.shape) == (8 * 5, vocab) and grad.stride() == (vp, 1)
    assert not bool(base[:, vocab:].any()) and bool(grad.any())
