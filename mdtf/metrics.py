"""``tf.metrics``: streaming evaluation metrics computed and accumulated on the device (TF 1.x names and argument
order; ``ops.metrics``, ``csrc/metrics.hip``).

Every function reduces one batch to ``{total, count}`` in fp64 on the inputs' device and returns a
:class:`MetricValue`; with ``accumulator=`` the same launch also adds the pair to an :class:`Accumulator`, the
streaming state.  Nothing is read by the host until ``MetricValue.value()`` / ``Accumulator.result()`` is called, so
the updates can sit inside a captured step.

Differences from TF 1.x:

* a :class:`MetricValue` is returned in place of TF's ``(value, update_op)`` pair: the batch's own pair is its
  ``.pair``, the streaming state is the ``Accumulator`` handed in;
* a row (element) whose weight is 0 is skipped instead of multiplied by 0: a NaN value there reaches neither the
  total nor the count, and :func:`top_k_accuracy` does not read the logits of such a row at all.

``weights`` is a tensor broadcastable to the values, or a Python scalar (a factor on total and count alike, which
the value cancels again unless it is 0).  :func:`top_k_accuracy` is an extension: the fused form of
``tf.metrics.mean(tf.nn.in_top_k(logits, labels, k), weights)``.  ``mdtf.estimator.metrics`` keeps its older
``(batch_value, weight)`` tuples; ``Estimator.evaluate`` accepts both.
"""
import numbers

import torch

from .ops import metrics as _M


def _ratio(pair):
    total, count = pair.tolist()                                 # the only host read
    return total / count if count != 0 else 0.0                  # div_no_nan


class MetricValue(object):
    """One batch of a metric: ``.pair`` is the fp64 ``[2]`` tensor ``{total, count}`` on the inputs' device."""

    def __init__(self, pair):
        self.pair = pair

    def value(self):
        """``total / count`` as a Python float, 0 when ``count == 0``.  Reads the device."""
        return _ratio(self.pair)


class Accumulator(object):
    """The state of a streaming metric: an fp64 ``[2]`` tensor ``{total, count}``.  Without ``device`` it is made
    on the device of the first update."""

    def __init__(self, device=None):
        self._t = None if device is None else torch.zeros(2, dtype=torch.float64, device=device)

    def on(self, device):
        """The state tensor, created on ``device`` when there is none yet."""
        if self._t is None:
            self._t = torch.zeros(2, dtype=torch.float64, device=device)
        return self._t

    @property
    def tensor(self):
        """The state (for collectives); zeros on the CPU before the first update."""
        return self.on("cpu")

    def update(self, value, *args, **kwargs):
        """Add a :class:`MetricValue` on the device; anything else is taken as the arguments of :func:`mean`."""
        if isinstance(value, MetricValue):
            if args or kwargs:
                raise TypeError("update(MetricValue) takes no further arguments")
            t = self.on(value.pair.device)
            t.add_(value.pair.to(t.device))
            return value
        return mean(value, *args, accumulator=self, **kwargs)

    def result(self):
        """``total / count`` over everything added, 0 when ``count == 0``.  Reads the device."""
        return _ratio(self.tensor)

    def reset(self):
        if self._t is not None:
            self._t.zero_()


def _split_weights(weights):
    if weights is None:
        return None, 1.0
    if isinstance(weights, numbers.Number):
        return None, float(weights)
    return torch.as_tensor(weights), 1.0


def _rows(values, weights):
    """(values [n], weights [n] or None, scalar factor): tensor weights broadcast to the values' shape."""
    w, s = _split_weights(weights)
    if w is not None and w.numel() != values.numel():
        w = w.to(values.device).expand(values.shape)
    return values.reshape(-1), (w.reshape(-1) if w is not None else None), s


def _reduce(values, w, s, accumulator):
    accum = accumulator.on(values.device) if accumulator is not None else None
    return MetricValue(_M.metric_reduce(values, w, s, accum))


def mean(values, weights=None, accumulator=None):
    """``tf.metrics.mean``: the weighted mean of ``values``."""
    return _reduce(*_rows(torch.as_tensor(values).detach().float(), weights), accumulator)


def accuracy(labels, predictions, weights=None, accumulator=None):
    """``tf.metrics.accuracy``: how often the class ids ``predictions`` equal ``labels``."""
    predictions = predictions.detach()
    labels = labels.detach().to(predictions.device).reshape(predictions.shape)
    return _reduce(*_rows((predictions == labels).float(), weights), accumulator)


def mean_squared_error(labels, predictions, weights=None, accumulator=None):
    """``tf.metrics.mean_squared_error``."""
    p = predictions.detach().float()
    d = p - labels.detach().float().to(p.device).reshape(p.shape)
    return _reduce(*_rows(d * d, weights), accumulator)


def top_k_accuracy(labels, logits, k=1, weights=None, accumulator=None):
    """How often ``labels`` [N] are among the top ``k`` classes of ``logits`` [N, K] (an extension; see the module
    docstring).  The weights reach the hits kernel, so the logits of a zero-weight row are not read.  As in
    ``tf.nn.in_top_k`` a class tied with the target counts as inside: ``k = 1`` counts an exact tie with the
    greatest logit as a hit, which an ``argmax`` comparison does not."""
    logits = logits.detach()
    rows = logits.reshape(-1, logits.shape[-1]) if logits.dim() != 2 else logits
    w, s = _split_weights(weights)
    if w is not None:
        w = _M.row_weights(w, rows.shape[0], rows.device)
    hits = _M.in_top_k_hits(rows, labels.reshape(-1), k, w)
    return _reduce(hits, w, s, accumulator)
