"""``tf.losses``: the two softmax cross entropies with ``weights`` and ``reduction`` (TF 1.x names).

Both reduce on the device (``ops.losses``, ``csrc/losses.hip``).  Differences from TF 1.x:

* ``loss_collection`` defaults to ``None``, not ``GraphKeys.LOSSES``: ``runtime.Tower`` already adds what a ``Loss``
  returns to ``"losses"``, so TF's default would count it twice.  Pass ``"losses"`` in code that sums the collection
  itself (an Estimator ``model_fn``).
* In the sparse form a row whose weight is 0 or whose label lies outside ``[0, K)`` is skipped: it contributes an exact
  0 to the loss and an exact zero row to the gradient, even where its logits are NaN (TF multiplies by the weight).
* ``sparse_softmax_cross_entropy`` takes two extensions: ``label_smoothing`` (TF smooths only dense one-hot labels,
  a ``[N, K]`` tensor that the sparse form exists to avoid) and ``denominator_epsilon``, added to the denominator of
  the reduction (BERT's ``sum(w * l) / (sum(w) + 1e-5)``).

No gradient flows to ``weights``.
"""
import numbers

import torch

from .ops import losses as _L
from .ops import nn as _nn
from .train import variables as _V


class Reduction(object):
    """``tf.losses.Reduction``."""
    NONE = "none"
    SUM = "weighted_sum"
    MEAN = "weighted_mean"
    SUM_OVER_BATCH_SIZE = "weighted_sum_over_batch_size"
    SUM_BY_NONZERO_WEIGHTS = "weighted_sum_by_nonzero_weights"

    @classmethod
    def all(cls):
        return (cls.NONE, cls.SUM, cls.MEAN, cls.SUM_OVER_BATCH_SIZE, cls.SUM_BY_NONZERO_WEIGHTS)

    @classmethod
    def validate(cls, key):
        if key not in cls.all():
            raise ValueError("Invalid Reduction Key %s." % key)


_MODES = {Reduction.NONE: _L.NONE, Reduction.SUM: _L.SUM, Reduction.MEAN: _L.MEAN,
          Reduction.SUM_OVER_BATCH_SIZE: _L.SUM_OVER_BATCH_SIZE,
          Reduction.SUM_BY_NONZERO_WEIGHTS: _L.SUM_BY_NONZERO_WEIGHTS}


def _split_weights(weights, reduction):
    """(tensor weights or None, scalar factor).  A Python scalar ``s`` is a weight of ``s`` on every row: a factor on
    the sums, which MEAN (``sum(s l) / sum(s)``) cancels again unless ``s`` is 0."""
    if weights is None:
        return None, 1.0
    if isinstance(weights, numbers.Number):
        s = float(weights)
        if reduction == Reduction.MEAN:
            s = 1.0 if s != 0.0 else 0.0
        return None, s
    return torch.as_tensor(weights), 1.0


def _finish(loss, loss_collection):
    if loss_collection is not None:
        _V.add_to_collection(loss_collection, loss)
    return loss


def sparse_softmax_cross_entropy(labels, logits, weights=1.0, scope=None, loss_collection=None,
                                 reduction=Reduction.SUM_BY_NONZERO_WEIGHTS, label_smoothing=0.0,
                                 denominator_epsilon=0.0):
    """Cross entropy of ``logits`` [..., K] against integer ``labels`` [...] (or [..., 1]).

    ``weights``: a Python scalar, or a tensor with one value per row ([N] or [N, 1]).  Returns a scalar, or the
    weighted per-row losses in the shape of ``labels`` for ``Reduction.NONE``."""
    Reduction.validate(reduction)
    k = logits.shape[-1]
    rows = logits.reshape(-1, k) if logits.dim() != 2 else logits
    w, s = _split_weights(weights, reduction)
    with _V.name_scope(scope or "sparse_softmax_cross_entropy_loss"):
        loss = _L.weighted_softmax_xent(rows, labels.reshape(-1), w, label_smoothing, _MODES[reduction],
                                        denominator_epsilon, s)
        if reduction == Reduction.NONE:
            loss = loss.reshape(logits.shape[:-1])
        return _finish(loss, loss_collection)


def softmax_cross_entropy(onehot_labels, logits, weights=1.0, label_smoothing=0, scope=None, loss_collection=None,
                          reduction=Reduction.SUM_BY_NONZERO_WEIGHTS):
    """Cross entropy against dense (soft) targets, smoothed as TF does: ``onehot * (1 - ls) + ls / K``.  The rows are
    the fp32 expression of ``nn.softmax_cross_entropy_with_logits``; weights and reduction run on the device."""
    Reduction.validate(reduction)
    k = logits.shape[-1]
    target = onehot_labels.float()
    if label_smoothing > 0:
        target = target * (1.0 - label_smoothing) + label_smoothing / k
    w, s = _split_weights(weights, reduction)
    with _V.name_scope(scope or "softmax_cross_entropy_loss"):
        rows = _nn.softmax_cross_entropy_with_logits(target.reshape(-1, k), logits.reshape(-1, k))
        loss = _L.reduce_rows(rows, w, _MODES[reduction], 0.0, s)
        if reduction == Reduction.NONE:
            loss = loss.reshape(logits.shape[:-1])
        return _finish(loss, loss_collection)
