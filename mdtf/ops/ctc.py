"""Connectionist temporal classification loss (``tf.nn.ctc_loss``) on the kernels of ``csrc/ctc.hip``.

Definition, all in the log domain, for time-major logits ``x`` [T, B, K] with the blank as class ``K - 1``, item ``b``
using the frames ``t < T_b`` and the labels ``l_1 .. l_L`` (``L = L_b``); ``l'`` is the extended label (blank, l_1,
blank, ..., l_L, blank) of ``S = 2L + 1`` states::

    lp[t, s]   = x[t, b, l'_s] - lse[t, b]
    alpha_0(0) = lp[0, 0], alpha_0(1) = lp[0, 1], every other state -inf
    alpha_t(s) = lp[t, s] + logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) if l'_s != blank, l'_{s-2})
    loss_b     = -logsumexp(alpha_{T_b-1}(S-1), alpha_{T_b-1}(S-2));   beta is the mirror image from T_b - 1 down
    dx[t,b,k]  = g_b (softmax(x[t, b])_k - sum_{s: l'_s = k} exp(alpha_t(s) + beta_t(s) - lp[t, s] + loss_b)),  t < T_b

An item with no alignment (``L_b + #{adjacent equal labels} > T_b``, or a label outside ``[0, K - 1)``) is infeasible:
its loss is ``+inf`` (0 with ``ignore_longer``), its gradient exactly 0.  Frames ``t >= T_b`` and infeasible items are
skipped, not multiplied by zero: NaN there reaches neither a loss nor a gradient.

On the GPU two launches make the loss and one the gradient whatever T is; the lengths are read on the device at every
launch (int32 device tensors are used as they are and may change in place between replays of a hipGraph), nothing is
read back by the host and there are no float atomics: everything is bitwise repeatable.  CPU tensors,
``MDTF_KERNELS=torch`` and ``Lmax > 511`` run :func:`ctc_reference`, the PyTorch expression of the same definition.
"""
import torch
import torch.nn.functional as F

from . import _native as N

BF16 = 0        # dtype codes of the entry points
FP32 = 1
MAX_LABELS = 511
_DIMS = [N.I] * 5 + [N.P]        # T, B, K, Lmax, dtype code, stream
N.register("mdtf_ctc_rows", [N.P] * 8 + _DIMS)
N.register("mdtf_ctc_alpha_beta", [N.P] * 8 + [N.I] + _DIMS)
N.register("mdtf_ctc_grad", [N.P] * 13 + _DIMS)


def native_ok(x, labels):
    """Whether the HIP kernels take this call (else the PyTorch expression runs)."""
    t, b, k = x.shape
    return (N.use_native(x) and x.dtype in (torch.bfloat16, torch.float32) and labels.shape[1] <= MAX_LABELS
            and t >= 1 and b >= 1 and t * b + b < (1 << 31))


def feasible(labels, seq_len, lab_len, t_n, k):
    """bool [B] without a host read: every label of the item inside [0, K - 1) and L_b + repeats <= T_b."""
    lmax = labels.shape[1]
    ln = lab_len.long().clamp(0, lmax)
    tb = seq_len.long().clamp(0, t_n)
    inside = torch.arange(lmax, device=labels.device)[None, :] < ln[:, None]
    bad = (inside & ((labels < 0) | (labels >= k - 1))).any(1)
    rep = (inside[:, 1:] & (labels[:, 1:] == labels[:, :-1])).sum(1)
    return ~bad & (ln + rep <= tb)


class _Reference(torch.autograd.Function):
    """``F.ctc_loss`` on an fp32 ``log_softmax`` with the gradient of the definition.  The gradient ``F.ctc_loss``
    hands to its log-probabilities is already ``g_b (exp(lp) - posterior)``, the gradient with respect to the logits
    (Graves et al., eq. 16).  ``log_softmax``'s backward would take ``p_k sum_j`` of it off, a sum that is zero but
    for the roundings of all K posteriors, and spread those over the row; here it is handed on as it is."""

    @staticmethod
    def forward(ctx, x, labels, seq_len, lab_len, ignore_longer):
        t_n, b_n, k = x.shape
        lmax = labels.shape[1]
        labels = labels.long()
        ok = feasible(labels, seq_len, lab_len, t_n, k)
        tb = seq_len.long().clamp(0, t_n)
        ln = lab_len.long().clamp(0, lmax)
        run = ok & (tb > 0)                                         # the items F.ctc_loss computes
        live = (torch.arange(t_n, device=x.device)[:, None] < tb[None, :]) & run[None, :]
        # dead frames and infeasible items are replaced before anything reads them
        xs = torch.where(live[:, :, None], x.float(), torch.zeros((), device=x.device))
        one, zero = torch.ones_like(tb), torch.zeros_like(tb)
        with torch.enable_grad():
            lp = torch.log_softmax(xs, -1).requires_grad_(True)
            rows = F.ctc_loss(lp, labels.clamp(0, k - 2), torch.where(run, tb, one), torch.where(run, ln, zero),
                              blank=k - 1, reduction="none")
        ctx.save_for_backward(lp, rows, live)
        ctx.dtype = x.dtype
        off = torch.full_like(rows, 0.0 if ignore_longer else float("inf"))
        return torch.where(run, rows, torch.where(ok, torch.zeros_like(rows), off)).detach()

    @staticmethod
    def backward(ctx, g):
        lp, rows, live = ctx.saved_tensors
        run = live.any(0)
        g = torch.where(run, g.float(), torch.zeros_like(rows))     # (an upstream NaN of a skipped item stays out)
        (dlp,) = torch.autograd.grad(rows, lp, g)
        return torch.where(live[:, :, None], dlp, torch.zeros_like(dlp)).to(ctx.dtype), None, None, None, None


def ctc_reference(x, labels, seq_len, lab_len, ignore_longer):
    """fp32 [B] by ``F.ctc_loss`` on an fp32 ``log_softmax``, the rules for dead frames and infeasible items around
    it; their gradient is an exact zero."""
    return _Reference.apply(x, labels, seq_len, lab_len, ignore_longer)


class _CTC(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, labels, seq_len, lab_len, ignore_longer):
        t_n, b_n, k = x.shape
        lmax = labels.shape[1]
        dev = x.device
        x = x.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        code = BF16 if x.dtype == torch.bfloat16 else FP32
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        lse, lpc = new((t_n, b_n)), new((t_n, b_n, lmax + 1))
        chain, flag = new((b_n, lmax), torch.int32), new((b_n,), torch.int32)
        alpha, beta = new((t_n, b_n, 2 * lmax + 1)), new((t_n, b_n, 2 * lmax + 1))
        loss = new((b_n,))
        dims = (t_n, b_n, k, lmax, code, N.stream_ptr())
        N.check(N.fn("mdtf_ctc_rows")(N.ptr(x), N.ptr(labels), N.ptr(seq_len), N.ptr(lab_len), N.ptr(lse), N.ptr(lpc),
                                      N.ptr(chain), N.ptr(flag), *dims), "ctc_rows")
        N.check(N.fn("mdtf_ctc_alpha_beta")(N.ptr(lpc), N.ptr(labels), N.ptr(seq_len), N.ptr(lab_len), N.ptr(flag),
                                            N.ptr(alpha), N.ptr(beta), N.ptr(loss), int(ignore_longer), *dims),
                "ctc_alpha_beta")
        ctx.save_for_backward(x, labels, seq_len, lab_len, flag, chain, lse, lpc, alpha, beta, loss)
        ctx.code = code
        return loss

    @staticmethod
    def backward(ctx, g):
        x, labels = ctx.saved_tensors[:2]
        t_n, b_n, k = x.shape
        g = g.float().contiguous()
        dx = torch.empty_like(x)
        N.check(N.fn("mdtf_ctc_grad")(*[N.ptr(t) for t in ctx.saved_tensors], N.ptr(g), N.ptr(dx), t_n, b_n, k,
                                      labels.shape[1], ctx.code, N.stream_ptr()), "ctc_grad")
        return dx, None, None, None, None


def _check_args(x, labels, seq_len, lab_len):
    if x.dim() != 3:
        raise ValueError("ctc_loss: inputs must be [T, B, K] (or [B, T, K] with time_major=False), got %s"
                         % (tuple(x.shape),))
    t_n, b_n, k = x.shape
    if k < 2:
        raise ValueError("ctc_loss: needs at least one class besides the blank, got K = %d" % k)
    if t_n < 1:
        raise ValueError("ctc_loss: needs at least one frame, got inputs %s" % (tuple(x.shape),))
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[0] != b_n:
        raise ValueError("ctc_loss: labels must be a dense integer [B, Lmax] tensor with B = %d, got %s"
                         % (b_n, tuple(labels.shape) if torch.is_tensor(labels) else type(labels).__name__))
    if labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError("ctc_loss: labels must be integers, got %s" % labels.dtype)
    if lab_len is None:
        raise ValueError("ctc_loss: dense labels need label_length [B] (there is no SparseTensor form)")
    for name, v in (("sequence_length", seq_len), ("label_length", lab_len)):
        if (torch.is_tensor(v) and v.dim() != 1) or not hasattr(v, "__len__") or len(v) != b_n:
            raise ValueError("ctc_loss: %s must have %d entries" % (name, b_n))


def ctc_loss(x, labels, seq_len, lab_len, ignore_longer=False):
    """fp32 [B] losses of time-major ``x`` [T, B, K] (bf16 or fp32) against dense ``labels`` [B, Lmax]."""
    from .rnn import _device_lengths
    _check_args(x, labels, seq_len, lab_len)
    dev = x.device
    seq_len, lab_len = _device_lengths(seq_len, dev), _device_lengths(lab_len, dev)
    labels = _device_lengths(labels, dev)                           # the same rule: int32 on the device as it is
    if native_ok(x, labels):
        return _CTC.apply(x, labels, seq_len, lab_len, bool(ignore_longer))
    return ctc_reference(x, labels, seq_len, lab_len, bool(ignore_longer))
