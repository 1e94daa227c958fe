"""``tf.nn.in_top_k`` rows and the ``tf.metrics`` reduction on the device (``csrc/metrics.hip``).

Definitions::

    t_r     = x[r, label_r],  c_r = #{j in [0, K): x[r, j] > t_r}
    hits_r  = 1 iff label_r in [0, K), t_r finite and c_r < k          (strict: ties with the target are inside)
    total   = wscale * sum_{r: w_r != 0} w_r * v_r,  count = wscale * sum_{r: w_r != 0} w_r       (fp64)

A row whose weight is 0 or whose label lies outside ``[0, K)`` is skipped, not multiplied: its logits are never read
and a NaN value under weight 0 reaches nothing.  On the GPU these are two launches with no host read, so they replay
inside a hipGraph.  CPU tensors, ``MDTF_KERNELS=torch`` and anything ``_native.use_native`` turns down run the
PyTorch expression of the same definitions: the comparison count in integers, the sums in fp64.
"""
import ctypes

import torch

from . import _native as N

N.register("mdtf_in_top_k", [N.P, N.I, N.P, N.P, N.I, N.I, N.L, N.I, N.P, N.P])
N.register("mdtf_metric_reduce", [N.P, N.P, N.I, ctypes.c_double, N.P, N.P, N.P])

_INT_MAX = 2 ** 31 - 1


def row_weights(weights, n, device):
    """fp32 [n] on ``device`` from a tensor broadcastable to the rows, or None."""
    if weights is None:
        return None
    return weights.detach().to(device=device, dtype=torch.float32).reshape(-1).expand(n).contiguous()


def _hits_reference(logits, labels, weights, k):
    n, kk = logits.shape
    valid = (labels >= 0) & (labels < kk)
    if weights is not None:
        valid = valid & (weights != 0)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    t = logits.gather(1, lab[:, None])
    count = (logits > t).sum(1)                                  # int64; NaN compares false
    return (valid & torch.isfinite(t.squeeze(1)) & (count < k)).float()


def in_top_k_hits(logits, labels, k, weights=None):
    """fp32 [N] of 0 / 1: whether ``labels`` [N] are among the top ``k`` of the rows of ``logits`` [N, K]."""
    if logits.dim() != 2 or labels.numel() != logits.shape[0]:
        raise ValueError("in_top_k expects [N, K] predictions and N targets, got %s and %s"
                         % (tuple(logits.shape), tuple(labels.shape)))
    k = int(k)
    if k < 1:
        raise ValueError("in_top_k needs k >= 1, got %d" % k)
    n, kk = logits.shape
    if kk < 1:
        raise ValueError("in_top_k needs at least one class")
    logits = logits.detach()
    if logits.dtype not in (torch.bfloat16, torch.float32):
        logits = logits.float()
    labels = labels.detach().reshape(-1).to(device=logits.device, dtype=torch.int64).contiguous()
    weights = row_weights(weights, n, logits.device)
    if not (N.use_native(logits) and n > 0):
        return _hits_reference(logits, labels, weights, k)
    if logits.stride(1) != 1 or logits.stride(0) < kk:
        logits = logits.contiguous()
    hits = torch.empty(n, dtype=torch.float32, device=logits.device)
    N.check(N.fn("mdtf_in_top_k")(N.ptr(logits), int(logits.dtype == torch.bfloat16), N.ptr(labels), N.ptr(weights),
                                  n, kk, logits.stride(0), min(k, _INT_MAX), N.ptr(hits), N.stream_ptr()),
            "in_top_k")
    return hits


def _reduce_reference(values, weights, wscale):
    v = values.double()
    if weights is None:
        total, count = v.sum(), torch.full((), float(v.numel()), dtype=torch.float64, device=v.device)
    else:
        w = weights.double()
        live = w != 0
        zero = torch.zeros_like(w)
        total, count = torch.where(live, w * v, zero).sum(), torch.where(live, w, zero).sum()
    if wscale == 0.0 or v.numel() == 0:
        return torch.zeros(2, dtype=torch.float64, device=v.device)
    return torch.stack([total, count]) * wscale


def metric_reduce(values, weights=None, wscale=1.0, accum=None):
    """fp64 [2] ``{total, count}`` of ``values`` [N] under ``weights`` (fp32 [N] or None) times ``wscale``; also
    added, on the device, to ``accum`` (fp64 [2]) when one is given."""
    values = values.detach().reshape(-1)
    n = values.numel()
    wscale = float(wscale)
    if accum is not None and (accum.dtype != torch.float64 or accum.numel() != 2 or not accum.is_contiguous()
                              or accum.device != values.device):
        raise ValueError("accum must be a contiguous fp64 [2] tensor on %s" % values.device)
    weights = row_weights(weights, n, values.device)
    if N.use_native(values) and n > 0:
        values = values.float().contiguous()
        pair = torch.empty(2, dtype=torch.float64, device=values.device)
        N.check(N.fn("mdtf_metric_reduce")(N.ptr(values), N.ptr(weights), n, wscale, N.ptr(pair), N.ptr(accum),
                                           N.stream_ptr()), "metric_reduce")
        return pair
    pair = _reduce_reference(values.float(), weights, wscale)
    if accum is not None:
        accum.add_(pair)
    return pair
