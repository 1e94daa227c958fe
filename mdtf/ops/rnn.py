"""LSTM over a time-major sequence (``tf.nn.dynamic_rnn`` over an ``LSTMCell``) on the kernels of ``csrc/lstm.hip``.

The cell is TF's ``LSTMCell`` / ``BasicLSTMCell`` with gate order ``i, j, f, o``, for ``x`` [T, B, I], ``kernel``
[I + H, 4H] and ``bias`` [4H]::

    [i j f o] = [x_t, h_{t-1}] @ kernel + bias
    c_t = c_{t-1} * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j)
    h_t = tanh(c_t) * sigmoid(o)

The HIP path runs for GPU tensors in bf16 with ``H % 32 == 0`` and no ``sequence_length``.  The input half
``xg = x @ kernel[:I] + bias`` over all ``T * B`` rows is one dense forward; the recurrence is one launch per step
(forward) and per step plus one (backward), all enqueued by one call of ``mdtf_lstm_fwd`` / ``mdtf_lstm_bwd``, with
the cell state in fp32 and ``hs`` / the post-activation gates saved in bf16.  The two halves of the kernel gradient
(``x^T @ dG`` and ``h_prev^T @ dG``) and the bias gradient are ``gemm.wgrad_into`` on the two row ranges of the
variable's fp32 gradient slot when there is one, and ``dx = dG @ kernel[:I]^T`` is the dense data gradient.

Every other case runs :func:`lstm_loop`, the definition as a PyTorch loop with fp32 gate math: CPU tensors,
``MDTF_KERNELS=torch`` (the comparator), fp32 activations, other ``H``, and any call with ``sequence_length`` (past
its length a row copies its state through and emits zeros, as TF does).  Not here: GRU and vanilla cells, peepholes,
projection, cell clipping, bidirectional and multi-cell wrappers.
"""
import torch

from . import _native as N
from ..train import variables as V

BF16 = 0        # dtype codes of the entry points (the kernels take only bf16)
FP32 = 1
N.register("mdtf_lstm_units", [N.I] * 4)
N.register("mdtf_lstm_fwd", [N.P] * 8 + [N.I] * 3 + [N.F, N.I, N.P])
N.register("mdtf_lstm_bwd", [N.P] * 9 + [N.I] * 4 + [N.P])


def native_ok(x, kernel, h0, sequence_length=None):
    """Whether the HIP kernels take this call (else the PyTorch loop runs)."""
    t, b, i = x.shape
    h = kernel.shape[1] // 4
    return (sequence_length is None and N.use_native(x) and x.dtype == torch.bfloat16 and h % 32 == 0 and h >= 32
            and t >= 1 and b >= 1 and i >= 1 and h0.is_cuda and b * 4 * h < (1 << 31) and b <= 16 * 65535)


def units_per_block(t, b, h):
    """Hidden units a block of the step kernels owns for this problem (16 or 32)."""
    return int(N.fn("mdtf_lstm_units")(t, b, h, BF16))


def lstm_loop(x, kernel, bias, h0, c0, forget_bias=1.0, sequence_length=None):
    """The definition as a loop over t: ``(hs [T, B, H], h_T, c_T)``.  Gate math and the cell state in fp32, ``h``
    in the dtype of ``x``.  ``sequence_length`` [B]: at ``t >= length`` a row emits zeros and keeps its state."""
    t_n, b_n, i_n = x.shape
    h_n = kernel.shape[1] // 4
    w = kernel.to(x.dtype)
    xg = torch.matmul(x.reshape(t_n * b_n, i_n), w[:i_n]) + bias.to(x.dtype)
    xg = xg.reshape(t_n, b_n, 4 * h_n)
    wh = w[i_n:].float()
    h, c = h0.to(x.dtype), c0.float()
    if sequence_length is not None:
        sequence_length = torch.as_tensor(sequence_length, device=x.device).reshape(b_n, 1)
    outs = []
    for t in range(t_n):
        pre = xg[t].float() + torch.matmul(h.float(), wh)
        gi, gj, gf, go = pre.split(h_n, 1)
        c_new = c * torch.sigmoid(gf + forget_bias) + torch.sigmoid(gi) * torch.tanh(gj)
        h_new = (torch.tanh(c_new) * torch.sigmoid(go)).to(x.dtype)
        if sequence_length is None:
            h, c = h_new, c_new
            outs.append(h)
        else:
            live = sequence_length > t
            h, c = torch.where(live, h_new, h), torch.where(live, c_new, c)
            outs.append(torch.where(live, h_new, torch.zeros_like(h_new)))
    return torch.stack(outs, 0), h, c.to(c0.dtype)


def _aligned(*ts):
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts)


class _LSTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, h0, c0, forget_bias):
        from . import gemm
        t_n, b_n, i_n = x.shape
        h_n = kernel.shape[1] // 4
        dev = x.device
        x, kernel = x.contiguous(), kernel.contiguous()
        h0b, c0f = h0.to(torch.bfloat16).contiguous(), c0.float().contiguous()
        wx, wh = kernel[:i_n], kernel[i_n:]
        x2 = x.view(t_n * b_n, i_n)
        xg = gemm.dense(x2, wx, bias.to(x.dtype)).contiguous()         # [T * B, 4H], the bias included
        wt = torch.empty(4 * h_n * h_n, dtype=torch.bfloat16, device=dev)
        hs = torch.empty((t_n, b_n, h_n), dtype=torch.bfloat16, device=dev)
        cs = torch.empty((t_n, b_n, h_n), dtype=torch.float32, device=dev)
        gates = torch.empty((t_n, b_n, 4 * h_n), dtype=torch.bfloat16, device=dev)
        if not _aligned(xg, wh, h0b, c0f):
            raise RuntimeError("mdtf lstm: operands must be 16-byte aligned")
        N.check(N.fn("mdtf_lstm_fwd")(N.ptr(xg), N.ptr(wh), N.ptr(wt), N.ptr(h0b), N.ptr(c0f), N.ptr(hs), N.ptr(cs),
                                      N.ptr(gates), t_n, b_n, h_n, float(forget_bias), BF16, N.stream_ptr()),
                "lstm_fwd")
        ctx.save_for_backward(x, kernel, h0b, c0f, hs, cs, gates)
        ctx.like = (kernel, bias, h0, c0)
        ctx.ksink, ctx.bsink = V.grad_sink(kernel), V.grad_sink(bias)
        return hs, hs[-1].clone(), cs[-1].clone()

    @staticmethod
    def backward(ctx, dhs, dh_t, dc_t):
        from . import gemm
        x, kernel, h0b, c0f, hs, cs, gates = ctx.saved_tensors
        kern_like, bias_like, h0_like, c0_like = ctx.like
        t_n, b_n, i_n = x.shape
        h_n = kernel.shape[1] // 4
        dev = x.device
        wx, wh = kernel[:i_n], kernel[i_n:]
        dhs = dhs.to(torch.bfloat16).contiguous()
        dh_t = dh_t.to(torch.bfloat16).contiguous()
        carry = dc_t.float().clone()                                    # dL/dc_T in, dL/dc_0 out
        dg = torch.empty((t_n, b_n, 4 * h_n), dtype=torch.bfloat16, device=dev)
        dh0 = torch.empty((b_n, h_n), dtype=torch.bfloat16, device=dev)
        N.check(N.fn("mdtf_lstm_bwd")(N.ptr(wh), N.ptr(gates), N.ptr(cs), N.ptr(c0f), N.ptr(dhs), N.ptr(dh_t),
                                      N.ptr(carry), N.ptr(dg), N.ptr(dh0), t_n, b_n, h_n, BF16, N.stream_ptr()),
                "lstm_bwd")
        dg2 = dg.view(t_n * b_n, 4 * h_n)
        dx = dkernel = dbias = None
        if ctx.needs_input_grad[0]:
            dx = gemm._hand_dgrad(dg2, wx)
            if dx is None:
                dx = torch.mm(dg2, wx.t())
            dx = dx.view(t_n, b_n, i_n)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            ksink, bsink = ctx.ksink, ctx.bsink
            gk = V.slot_or_zeros(ksink, kernel.shape, dev)
            gb = V.slot_or_zeros(bsink, (4 * h_n,), dev)
            h_prev = torch.cat([h0b[None], hs[:-1]], 0).view(t_n * b_n, h_n)
            if not gemm.wgrad_into(gk[:i_n], x.view(t_n * b_n, i_n), dg2, gb):
                gb.add_(torch.sum(dg2, 0, dtype=torch.float32))         # (a fixed-order sum: repeatable)
            gemm.wgrad_into(gk[i_n:], h_prev, dg2)
            dkernel = V.grad_marker(kern_like) if ksink is not None else gk.to(kern_like.dtype)
            dbias = V.grad_marker(bias_like) if bsink is not None else gb.to(bias_like.dtype)
        return dx, dkernel, dbias, dh0.to(h0_like.dtype), carry.to(c0_like.dtype), None


def lstm(x, kernel, bias, h0, c0, forget_bias=1.0, sequence_length=None):
    """``(hs, h_T, c_T)`` of the LSTM over time-major ``x`` [T, B, I] from the state ``(h0, c0)`` [B, H].  On the
    kernel path ``c_T`` is fp32 whatever ``c0`` is."""
    if x.dim() != 3:
        raise ValueError("lstm: x must be [T, B, I], got %s" % (tuple(x.shape),))
    t_n, b_n, i_n = x.shape
    if kernel.dim() != 2 or kernel.shape[1] % 4 or kernel.shape[0] != i_n + kernel.shape[1] // 4:
        raise ValueError("lstm: kernel must be [I + H, 4H] with I = %d, got %s" % (i_n, tuple(kernel.shape)))
    h_n = kernel.shape[1] // 4
    if tuple(bias.shape) != (4 * h_n,):
        raise ValueError("lstm: bias must be [%d], got %s" % (4 * h_n, tuple(bias.shape)))
    for name, s in (("h", h0), ("c", c0)):
        if tuple(s.shape) != (b_n, h_n):
            raise ValueError("lstm: initial %s must be [%d, %d], got %s" % (name, b_n, h_n, tuple(s.shape)))
    if sequence_length is not None and len(sequence_length) != b_n:
        raise ValueError("lstm: sequence_length must have %d entries" % b_n)
    if native_ok(x, kernel, h0, sequence_length):
        if kernel.dtype != x.dtype:
            kernel = kernel.to(x.dtype)
        return _LSTM.apply(x, kernel, bias, h0, c0, float(forget_bias))
    return lstm_loop(x, kernel, bias, h0, c0, forget_bias, sequence_length)
