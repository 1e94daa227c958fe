"""LSTM over a time-major sequence (``tf.nn.dynamic_rnn`` / ``tf.nn.bidirectional_dynamic_rnn`` over ``LSTMCell``s) on
the kernels of ``csrc/lstm.hip``.

The cell is TF's ``LSTMCell`` / ``BasicLSTMCell`` with gate order ``i, j, f, o``, for ``x`` [T, B, I], ``kernel``
[I + H, 4H] and ``bias`` [4H]::

    [i j f o] = [x_t, h_{t-1}] @ kernel + bias
    c_t = c_{t-1} * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j)
    h_t = tanh(c_t) * sigmoid(o)

``sequence_length`` [B]: row b is live at step t iff ``t < sequence_length[b]``; a dead row emits zeros and keeps its
state, as TF does.  ``reverse``: the same recurrence visits ``t = T - 1 .. 0`` under the same rule, which is TF's
``reverse_sequence`` -> LSTM -> ``reverse_sequence`` with no tensor reversed.

The HIP path runs for GPU tensors in bf16 with ``H % 32 == 0``, with or without lengths, in either direction, and
for two directions at once (:func:`bilstm`).  The input half ``xg = x @ kernel[:I] + bias`` over all ``T * B`` rows is
one dense forward (one product over ``[I, 8H]`` for two directions); the recurrence is one launch per step (forward)
and per step plus one (backward), both directions in the same launches, all enqueued by one call of
``mdtf_lstm_fwd_seq`` / ``mdtf_lstm_bwd_seq``, with the cell state in fp32 and ``hs`` / the post-activation gates saved
in bf16.  The lengths are an int32 device tensor that only the kernels read: nothing here reads them on the host, so
they may change between replays of a captured step.  The two halves of the kernel gradient (``x^T @ dG`` and
``h_prev^T @ dG``) and the bias gradient are ``gemm.wgrad_into`` on the two row ranges of the variable's fp32 gradient
slot when there is one, and ``dx = dG @ kernel[:I]^T`` is the dense data gradient.

Every other case runs :func:`lstm_loop`, the definition as a PyTorch loop with fp32 gate math: CPU tensors,
``MDTF_KERNELS=torch`` (the comparator), fp32 activations and other ``H``.  Not here: vanilla cells, peepholes,
projection, cell clipping and multi-cell wrappers (the GRU is ``ops/gru.py``).
"""
import ctypes

import torch

from . import _native as N
from ..train import variables as V

BF16 = 0        # dtype codes of the entry points (the kernels take only bf16)
FP32 = 1
N.register("mdtf_lstm_units", [N.I] * 4)
N.register("mdtf_lstm_fwd", [N.P] * 8 + [N.I] * 3 + [N.F, N.I, N.P])
N.register("mdtf_lstm_bwd", [N.P] * 9 + [N.I] * 4 + [N.P])
N.register("mdtf_lstm_fwd_seq", [N.P, N.I, N.I, N.P] + [N.I] * 4 + [N.F, N.I, N.P])
N.register("mdtf_lstm_bwd_seq", [N.P, N.I, N.I, N.P] + [N.I] * 4 + [N.P])


def native_ok(x, kernel, h0, sequence_length=None):
    """Whether the HIP kernels take this call (else the PyTorch loop runs); lengths do not matter."""
    t, b, i = x.shape
    h = kernel.shape[1] // 4
    return (N.use_native(x) and x.dtype == torch.bfloat16 and h % 32 == 0 and h >= 32
            and t >= 1 and b >= 1 and i >= 1 and h0.is_cuda and b * 4 * h < (1 << 31) and b <= 16 * 65535)


def units_per_block(t, b, h):
    """Hidden units a block of the step kernels owns for this problem (16 or 32)."""
    return int(N.fn("mdtf_lstm_units")(t, b, h, BF16))


def lstm_loop(x, kernel, bias, h0, c0, forget_bias=1.0, sequence_length=None, reverse=False):
    """The definition as a loop over t: ``(hs [T, B, H], h_T, c_T)``.  Gate math and the cell state in fp32, ``h``
    in the dtype of ``x``.  ``sequence_length`` [B]: at ``t >= length`` a row emits zeros and keeps its state.
    ``reverse``: t runs from ``T - 1`` down to 0 (the padding steps first, leaving the initial state in place)."""
    t_n, b_n, i_n = x.shape
    h_n = kernel.shape[1] // 4
    w = kernel.to(x.dtype)
    xg = torch.matmul(x.reshape(t_n * b_n, i_n), w[:i_n]) + bias.to(x.dtype)
    xg = xg.reshape(t_n, b_n, 4 * h_n)
    wh = w[i_n:].float()
    h, c = h0.to(x.dtype), c0.float()
    if sequence_length is not None:
        sequence_length = torch.as_tensor(sequence_length, device=x.device).reshape(b_n, 1)
    outs = [None] * t_n
    for t in (range(t_n - 1, -1, -1) if reverse else range(t_n)):
        pre = xg[t].float() + torch.matmul(h.float(), wh)
        gi, gj, gf, go = pre.split(h_n, 1)
        c_new = c * torch.sigmoid(gf + forget_bias) + torch.sigmoid(gi) * torch.tanh(gj)
        h_new = (torch.tanh(c_new) * torch.sigmoid(go)).to(x.dtype)
        if sequence_length is None:
            h, c = h_new, c_new
            outs[t] = h
        else:
            live = sequence_length > t
            h, c = torch.where(live, h_new, h), torch.where(live, c_new, c)
            outs[t] = torch.where(live, h_new, torch.zeros_like(h_new))
    return torch.stack(outs, 0), h, c.to(c0.dtype)


def _aligned(*ts):
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts)


def _table(rows):
    """The entry points' pointer table: one row of tensors (or None) per direction."""
    flat = [t.data_ptr() if t is not None else 0 for row in rows for t in row]
    return (ctypes.c_void_p * len(flat))(*flat)


def _h_prev(h0b, hs, lens, reverse):
    """[T * B, H]: the ``h`` every live (t, b) started from, for the recurrent half of the kernel gradient.  Dead
    (t, b) hold something finite (their dG is zero).  Device ops only."""
    t_n, b_n, h_n = hs.shape
    if not reverse:
        hp = torch.cat([h0b[None], hs[:-1]], 0)                         # dead rows of hs are zero
    else:
        hp = torch.cat([hs[1:], h0b[None]], 0)
        if lens is not None:                                            # a row's first visited live step is len - 1
            first = torch.arange(t_n, device=hs.device)[:, None] == lens.clamp(0, t_n)[None] - 1
            hp = torch.where(first[:, :, None], h0b[None], hp)
    return hp.view(t_n * b_n, h_n)


class _LSTM(torch.autograd.Function):
    """``ndir`` (1 or 2) LSTMs over the same ``x`` and lengths, direction d reversed where bit d of ``reverse`` is
    set; ``params``: ``kernel, bias, h0, c0`` per direction; returns ``hs, h_T, c_T`` per direction."""

    @staticmethod
    def forward(ctx, x, lens, forget_bias, reverse, *params):
        from . import gemm
        ndir = len(params) // 4
        t_n, b_n, i_n = x.shape
        h_n = params[0].shape[1] // 4
        dev = x.device
        x = x.contiguous()
        x2 = x.view(t_n * b_n, i_n)
        kernels = [params[4 * d].contiguous() for d in range(ndir)]
        biases = [params[4 * d + 1].to(x.dtype) for d in range(ndir)]
        h0s = [params[4 * d + 2].to(torch.bfloat16).contiguous() for d in range(ndir)]
        c0s = [params[4 * d + 3].float().contiguous() for d in range(ndir)]
        # the input halves of all directions, bias included: one product, [T * B, ndir * 4H]
        xg = gemm.dense_multi(x2, [k[:i_n] for k in kernels], biases).contiguous()
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        rows, saved, outs = [], [], []
        for d in range(ndir):
            hs, cs = new((t_n, b_n, h_n), torch.bfloat16), new((t_n, b_n, h_n), torch.float32)
            gates = new((t_n, b_n, 4 * h_n), torch.bfloat16)
            h_fin, c_fin = new((b_n, h_n), torch.bfloat16), new((b_n, h_n), torch.float32)
            wh, wt = kernels[d][i_n:], new(4 * h_n * h_n, torch.bfloat16)
            if not _aligned(wh, h0s[d], c0s[d]) or xg.data_ptr() % 16:
                raise RuntimeError("mdtf lstm: operands must be 16-byte aligned")
            rows.append((xg[:, 4 * h_n * d:], wh, wt, h0s[d], c0s[d], hs, cs, gates, h_fin, c_fin))
            saved += [kernels[d], h0s[d], c0s[d], hs, cs, gates]
            outs += [hs, h_fin, c_fin]
        N.check(N.fn("mdtf_lstm_fwd_seq")(_table(rows), ndir, reverse, N.ptr(lens), t_n, b_n, h_n, xg.shape[1],
                                          float(forget_bias), BF16, N.stream_ptr()), "lstm_fwd_seq")
        ctx.save_for_backward(x, lens, *saved)
        ctx.reverse, ctx.like = reverse, params
        ctx.sinks = [(V.grad_sink(params[4 * d]), V.grad_sink(params[4 * d + 1])) for d in range(ndir)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        from . import gemm
        x, lens = ctx.saved_tensors[:2]
        saved = ctx.saved_tensors[2:]
        ndir = len(saved) // 6
        t_n, b_n, i_n = x.shape
        h_n = saved[0].shape[1] // 4
        dev = x.device
        x2 = x.view(t_n * b_n, i_n)
        rows, keep = [], []
        for d in range(ndir):
            kernel, h0b, c0f, hs, cs, gates = saved[6 * d:6 * d + 6]
            dhs, dh_t, dc_t = grads[3 * d:3 * d + 3]
            dhs, dh_t = dhs.to(torch.bfloat16).contiguous(), dh_t.to(torch.bfloat16).contiguous()
            carry = dc_t.float().clone()                                # dL/dc_T in, dL/dc_0 out
            dg = torch.empty((t_n, b_n, 4 * h_n), dtype=torch.bfloat16, device=dev)
            dh0 = torch.empty((b_n, h_n), dtype=torch.bfloat16, device=dev)
            rows.append((kernel[i_n:], gates, cs, c0f, dhs, dh_t, carry, dg, dh0))
            keep.append((dg.view(t_n * b_n, 4 * h_n), dh0, carry))
        N.check(N.fn("mdtf_lstm_bwd_seq")(_table(rows), ndir, ctx.reverse, N.ptr(lens), t_n, b_n, h_n, BF16,
                                          N.stream_ptr()), "lstm_bwd_seq")
        dx, out = None, []
        for d in range(ndir):
            kernel, h0b, _, hs = saved[6 * d:6 * d + 4]
            kern_like, bias_like, h0_like, c0_like = ctx.like[4 * d:4 * d + 4]
            dg2, dh0, carry = keep[d]
            wx = kernel[:i_n]
            if ctx.needs_input_grad[0] and dx is None:
                dx = gemm._hand_dgrad(dg2, wx)
                if dx is None:
                    dx = torch.mm(dg2, wx.t())
            elif ctx.needs_input_grad[0]:
                dx.addmm_(dg2, wx.t())                                  # the second direction adds into the first's
            dkernel = dbias = None
            if ctx.needs_input_grad[4 + 4 * d] or ctx.needs_input_grad[5 + 4 * d]:
                ksink, bsink = ctx.sinks[d]
                gk = V.slot_or_zeros(ksink, kernel.shape, dev)
                gb = V.slot_or_zeros(bsink, (4 * h_n,), dev)
                if not gemm.wgrad_into(gk[:i_n], x2, dg2, gb):
                    gb.add_(torch.sum(dg2, 0, dtype=torch.float32))     # (a fixed-order sum: repeatable)
                gemm.wgrad_into(gk[i_n:], _h_prev(h0b, hs, lens, (ctx.reverse >> d) & 1), dg2)
                dkernel = V.grad_marker(kern_like) if ksink is not None else gk.to(kern_like.dtype)
                dbias = V.grad_marker(bias_like) if bsink is not None else gb.to(bias_like.dtype)
            out += [dkernel, dbias, dh0.to(h0_like.dtype), carry.to(c0_like.dtype)]
        if dx is not None:
            dx = dx.view(t_n, b_n, i_n)
        return (dx, None, None, None) + tuple(out)


def _check_args(x, kernel, bias, h0, c0, sequence_length):
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


def _device_lengths(sequence_length, device):
    """The kernels' int32 [B] tensor: a device int32 tensor as it is, anything else copied once."""
    if sequence_length is None:
        return None
    if (torch.is_tensor(sequence_length) and sequence_length.device == device and sequence_length.dtype == torch.int32
            and sequence_length.is_contiguous()):
        return sequence_length
    return torch.as_tensor(sequence_length, dtype=torch.int32).to(device).contiguous()


def lstm(x, kernel, bias, h0, c0, forget_bias=1.0, sequence_length=None, reverse=False):
    """``(hs, h_T, c_T)`` of the LSTM over time-major ``x`` [T, B, I] from the state ``(h0, c0)`` [B, H], in the
    ``reverse`` direction if asked.  On the kernel path ``c_T`` is fp32 whatever ``c0`` is."""
    _check_args(x, kernel, bias, h0, c0, sequence_length)
    if native_ok(x, kernel, h0, sequence_length):
        if kernel.dtype != x.dtype:
            kernel = kernel.to(x.dtype)
        return _LSTM.apply(x, _device_lengths(sequence_length, x.device), float(forget_bias), int(bool(reverse)),
                           kernel, bias, h0, c0)
    return lstm_loop(x, kernel, bias, h0, c0, forget_bias, sequence_length, reverse)


def bilstm(x, fw, bw, forget_bias=1.0, sequence_length=None):
    """A forward-in-time and a reverse LSTM over the same ``x`` [T, B, I] and lengths: ``((hs, h_T, c_T) of fw, the
    same of bw)`` for ``fw`` / ``bw`` = ``(kernel, bias, h0, c0)`` with the same ``H``.  On the kernel path every step
    launch runs step s of ``fw`` and step ``T - 1 - s`` of ``bw``; directions that differ in ``H`` or in
    ``forget_bias`` (a pair) run as two calls of :func:`lstm`."""
    fb_fw, fb_bw = forget_bias if isinstance(forget_bias, (tuple, list)) else (forget_bias, forget_bias)
    for p in (fw, bw):
        _check_args(x, *p, sequence_length)
    if (fw[0].shape == bw[0].shape and fb_fw == fb_bw and native_ok(x, fw[0], fw[2], sequence_length)
            and bw[2].is_cuda):
        flat = [t.to(x.dtype) if j == 0 and t.dtype != x.dtype else t for p in (fw, bw) for j, t in enumerate(p)]
        out = _LSTM.apply(x, _device_lengths(sequence_length, x.device), float(fb_fw), 0b10, *flat)
        return out[:3], out[3:]
    if sequence_length is not None and x.is_cuda:
        sequence_length = _device_lengths(sequence_length, x.device)    # copied once for both calls
    return lstm(x, *fw, fb_fw, sequence_length), lstm(x, *bw, fb_bw, sequence_length, True)
