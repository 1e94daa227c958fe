"""Weighted, label-smoothed softmax cross entropy and the ``tf.losses`` reductions (``csrc/losses.hip``).

Definition (all fp32; ``eps`` = label smoothing, ``K`` classes)::

    loss_r = lse_r - (1 - eps) * x[r, label_r] - (eps / K) * sum_k x[r, k]
    effw_r = weight of row r, 0 when the row is ignored (label outside [0, K) or weight 0)
    num    = sum_r effw_r * loss_r
    den    = 1 | N | sum_r effw_r | #{r: effw_r != 0}   (+ den_add)
    out    = scale * num / den, 0 when den == 0

An ignored row is skipped, not multiplied by zero: its logits are never read, so NaN there reaches neither the loss
nor any gradient.  On the GPU three launches make the loss and one the gradient; the denominator and the upstream
gradient stay on the device (no host read: the step stays a replayable hipGraph).  CPU tensors, ``MDTF_KERNELS=torch``
and anything ``_native.use_native`` turns down run the PyTorch expression of the same definition.
"""
import torch

from . import _native as N

N.register("mdtf_xent_w_fwd", [N.P, N.I, N.P, N.P, N.F, N.I, N.I, N.L, N.F, N.I, N.P, N.P, N.P, N.P])
N.register("mdtf_loss_reduce", [N.P, N.P, N.I, N.I, N.F, N.F, N.P, N.P])
N.register("mdtf_xent_w_bwd", [N.P, N.I, N.P, N.P, N.P, N.P, N.P, N.P, N.I, N.I, N.L, N.L, N.F, N.P])

# reduction modes of mdtf_loss_reduce; NONE keeps the weighted rows
NONE, SUM, SUM_OVER_BATCH_SIZE, MEAN, SUM_BY_NONZERO_WEIGHTS = -1, 0, 1, 2, 3


def _reduce_native(rows, effw, mode, den_add, scale):
    """fp32 [2] = {scale * sum(effw * rows) / den, scale / den} from ``mdtf_loss_reduce``."""
    out = torch.empty(2, dtype=torch.float32, device=rows.device)
    N.check(N.fn("mdtf_loss_reduce")(N.ptr(rows), N.ptr(effw), rows.numel(), mode, den_add, scale, N.ptr(out),
                                     N.stream_ptr()), "loss_reduce")
    return out


def _reduce_reference(rows, effw, mode, den_add, scale):
    """The same reduction in PyTorch: fp64 sums, one rounding to fp32, ``div_no_nan``."""
    num = (effw.double() * rows.double()).sum()
    if mode == SUM:
        den = torch.ones((), dtype=torch.float64, device=rows.device)
    elif mode == SUM_OVER_BATCH_SIZE:
        den = torch.full((), float(rows.numel()), dtype=torch.float64, device=rows.device)
    elif mode == MEAN:
        den = effw.double().sum()
    else:
        den = (effw != 0).double().sum()
    den = den + den_add
    safe = torch.where(den == 0, torch.ones_like(den), den)
    return torch.where(den == 0, torch.zeros_like(num), scale * num / safe).float()


def _effective_weights(weights, n, device):
    if weights is None:
        return None
    return weights.detach().to(device=device, dtype=torch.float32).reshape(-1).expand(n).contiguous()


class _XentW(torch.autograd.Function):
    """Rows may be strided exactly as for ``kernels._Xent``; the gradient of a strided bf16 input comes back as the
    ``[:, :K]`` view of a zero-padded ``[N, ldo]`` buffer recorded in ``gemm._PADDED_GRADS``."""

    @staticmethod
    def forward(ctx, logits, labels, weights, eps, mode, den_add, scale):
        if logits.dtype not in (torch.bfloat16, torch.float32):
            logits = logits.float()
        if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
            logits = logits.contiguous()
        labels = labels.to(torch.int64).contiguous()
        n, k = logits.shape
        dev = logits.device
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        lse = torch.empty_like(loss)
        effw = torch.empty_like(loss)
        none = mode == NONE
        N.check(N.fn("mdtf_xent_w_fwd")(N.ptr(logits), int(logits.dtype == torch.bfloat16), N.ptr(labels),
                                        N.ptr(weights), scale if none else 1.0, n, k, logits.stride(0), eps,
                                        int(none), N.ptr(loss), N.ptr(lse), N.ptr(effw), N.stream_ptr()), "xent_w_fwd")
        ctx.eps = eps
        if none:
            ctx.save_for_backward(logits, labels, lse, effw)
            return loss
        out = _reduce_native(loss, effw, mode, den_add, scale)
        ctx.save_for_backward(logits, labels, lse, effw, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse, effw = ctx.saved_tensors[:4]
        coef = ctx.saved_tensors[4][1:] if len(ctx.saved_tensors) > 4 else None
        n, k = logits.shape
        ldi = logits.stride(0)
        ldo = ldi if (ldi != k and ldi % 8 == 0 and logits.dtype == torch.bfloat16) else k
        dl = torch.empty((n, ldo), dtype=logits.dtype, device=logits.device)
        g = g.float().contiguous()
        N.check(N.fn("mdtf_xent_w_bwd")(N.ptr(logits), int(logits.dtype == torch.bfloat16), N.ptr(labels), N.ptr(lse),
                                        N.ptr(effw), N.ptr(coef), N.ptr(g), N.ptr(dl), n, k, ldi, ldo, ctx.eps,
                                        N.stream_ptr()), "xent_w_bwd")
        none6 = (None,) * 6
        if ldo == k:
            return (dl,) + none6
        from . import gemm
        if len(gemm._PADDED_GRADS) > 16:
            gemm._PADDED_GRADS.clear()
        gemm._PADDED_GRADS[dl.data_ptr()] = ldo     # zero-padded by the kernel: the tied decoder reads whole rows
        return (dl[:, :k],) + none6


class _Reduce(torch.autograd.Function):
    """``mdtf_loss_reduce`` over rows some other expression made (the dense soft-target loss)."""

    @staticmethod
    def forward(ctx, rows, effw, mode, den_add, scale):
        rows = rows.float().contiguous()
        out = _reduce_native(rows, effw, mode, den_add, scale)
        ctx.save_for_backward(effw, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        effw, out = ctx.saved_tensors
        return (g.float() * out[1]) * effw, None, None, None, None


def _rows_reference(logits, labels, weights, eps, scale_rows):
    """(loss rows, effw) in fp32 without a dense one-hot tensor; ignored rows are exact zeros whatever they hold."""
    x = logits.float()
    n, k = x.shape
    labels = labels.long()
    valid = (labels >= 0) & (labels < k)
    w = torch.ones(n, dtype=torch.float32, device=x.device) if weights is None else weights
    w = w * scale_rows if scale_rows != 1.0 else w
    effw = torch.where(valid, w, torch.zeros_like(w))
    live = effw != 0
    x = torch.where(live[:, None], x, torch.zeros_like(x))
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    loss = torch.logsumexp(x, -1) - (1.0 - eps) * x.gather(1, lab[:, None]).squeeze(1)
    if eps > 0:
        loss = loss - (eps / k) * x.sum(-1)
    return torch.where(live, loss, torch.zeros_like(loss)), effw


def weighted_softmax_xent(logits, labels, weights=None, label_smoothing=0.0, mode=SUM_BY_NONZERO_WEIGHTS,
                          den_add=0.0, scale=1.0):
    """Sparse softmax cross entropy of ``logits`` [N, K] against ``labels`` [N] with per-row ``weights`` (fp32 [N] or
    None), reduced by ``mode``: a scalar, or the weighted rows ``scale * effw_r * loss_r`` for ``NONE``."""
    if logits.dim() != 2 or labels.numel() != logits.shape[0]:
        raise ValueError("weighted_softmax_xent expects [N, K] logits and N labels, got %s and %s"
                         % (tuple(logits.shape), tuple(labels.shape)))
    n, k = logits.shape
    if k < 2:
        raise ValueError("softmax cross entropy needs at least 2 classes, got %d" % k)
    eps, den_add, scale = float(label_smoothing), float(den_add), float(scale)
    if not 0.0 <= eps <= 1.0:
        raise ValueError("label_smoothing must lie in [0, 1], got %r" % eps)
    labels = labels.reshape(-1)
    weights = _effective_weights(weights, n, logits.device)
    if N.use_native(logits) and n > 0:
        return _XentW.apply(logits, labels, weights, eps, mode, den_add, scale)
    rows, effw = _rows_reference(logits, labels, weights, eps, scale if mode == NONE else 1.0)
    if mode == NONE:
        return rows * effw
    return _reduce_reference(rows, effw, mode, den_add, scale)


def reduce_rows(rows, weights=None, mode=SUM_BY_NONZERO_WEIGHTS, den_add=0.0, scale=1.0):
    """The same reductions over per-example losses ``rows`` [N] made elsewhere."""
    rows = rows.reshape(-1)
    n = rows.numel()
    effw = _effective_weights(weights, n, rows.device)
    if effw is None:
        effw = torch.ones(n, dtype=torch.float32, device=rows.device)
    if mode == NONE:
        return rows.float() * (effw * float(scale))
    if N.use_native(rows) and n > 0:
        return _Reduce.apply(rows, effw, mode, float(den_add), float(scale))
    return _reduce_reference(rows.float(), effw, mode, float(den_add), float(scale))
