"""GRU over a time-major sequence (``tf.nn.dynamic_rnn`` over a ``GRUCell``) on the kernels of ``csrc/gru.hip``.

The cell is TF's ``GRUCell``, which applies the reset gate before the candidate product, for ``x`` [T, B, I],
``gates_kernel`` [I + H, 2H], ``gates_bias`` [2H], ``cand_kernel`` [I + H, H] and ``cand_bias`` [H]::

    [r u] = sigmoid([x_t, h_{t-1}] @ gates_kernel + gates_bias)
    c     = tanh([x_t, r * h_{t-1}] @ cand_kernel + cand_bias)
    h_t   = u * h_{t-1} + (1 - u) * c

``sequence_length`` [B]: row b is live at step t iff ``t < sequence_length[b]``; a dead row emits zeros and keeps its
state, as TF does.  ``reverse``: the same recurrence visits ``t = T - 1 .. 0`` under the same rule, which is TF's
``reverse_sequence`` -> GRU -> ``reverse_sequence`` with no tensor reversed.

The HIP path runs for GPU tensors in bf16 with ``H % 32 == 0``, with or without lengths, in either direction, and for
two directions at once (:func:`bigru`).  The input half ``xg = x @ [gates_kernel[:I] | cand_kernel[:I]] + [gates_bias |
cand_bias]`` over all ``T * B`` rows is one dense forward (one product over ``[I, 6H]`` for two directions); the
recurrence is two launches per step (``r``, ``u`` and ``r * h``; then the candidate and the update), both directions
in the same launches, all enqueued by one call of ``mdtf_gru_fwd_seq``, and ``2T + 1`` launches of
``mdtf_gru_bwd_seq`` backwards.  The lengths are an int32 device tensor that only the kernels read: nothing here reads
them on the host, so they may change between replays of a captured step.  The state is carried in fp32 inside the
call (``h`` is a leaky integrator: a bf16 carry loses the update where ``u`` is near 1); ``hs``, and with it the
returned state, are its bf16 rounding, so ``h_T`` has the bits of ``hs`` at each row's last visited live step
(``hs[-1]`` on a full-length forward call, ``h0`` for length 0).  Dead ``(t, b)`` of every saved buffer and of ``dG``
are zeros, so the whole ``[T * B, .]`` buffers go into the products: both kernel gradients and both bias gradients are
``gemm.wgrad_into`` on the row ranges of the variables' fp32 gradient slots when there are any (the recurrent rows of
the gates kernel against ``rnn._h_prev``, those of the candidate kernel against ``r * h_prev``), and ``dx`` is the
dense data gradient over ``[gates_kernel[:I] | cand_kernel[:I]]``, the second direction's added into the first's.

Every other case runs :func:`gru_loop`, the definition as a PyTorch loop with fp32 gate math and an fp32 carry: CPU
tensors, ``MDTF_KERNELS=torch`` (the comparator), fp32 activations and other ``H``.  A single forward-in-time call
without lengths runs ``mdtf_gru_fwd`` / ``mdtf_gru_bwd``, the same recurrence without the length and direction logic:
the same bits, a little faster per step.  Not here: the reset-after (Keras / cuDNN)
cell, vanilla cells and multi-cell wrappers.
"""
import torch

from . import _native as N
from . import rnn
from ..train import variables as V

BF16 = 0        # dtype codes of the entry points (the kernels take only bf16)
FP32 = 1
N.register("mdtf_gru_units", [N.I] * 4)
N.register("mdtf_gru_force_units", [N.I] * 2)
N.register("mdtf_gru_fwd", [N.P] * 10 + [N.I] * 4 + [N.P])
N.register("mdtf_gru_bwd", [N.P] * 8 + [N.I] * 4 + [N.P])
N.register("mdtf_gru_fwd_seq", [N.P, N.I, N.I, N.P] + [N.I] * 5 + [N.P])
N.register("mdtf_gru_bwd_seq", [N.P, N.I, N.I, N.P] + [N.I] * 4 + [N.P])


def native_ok(x, cand_kernel, h0, sequence_length=None):
    """Whether the HIP kernels take this call (else the PyTorch loop runs); lengths do not matter."""
    t, b, i = x.shape
    h = cand_kernel.shape[1]
    return (N.use_native(x) and x.dtype == torch.bfloat16 and h % 32 == 0 and h >= 32
            and t >= 1 and b >= 1 and i >= 1 and h0.is_cuda and b * 3 * h < (1 << 31) and b <= 16 * 65535)


def units_per_block(t, b, h):
    """Hidden units a block owns for this problem, ``(gate launch, the other launches)``, each 16 or 32."""
    code = int(N.fn("mdtf_gru_units")(t, b, h, BF16))
    return code & 0xFF, code >> 8


def gru_loop(x, gates_kernel, gates_bias, cand_kernel, cand_bias, h0, sequence_length=None, reverse=False):
    """The definition as a loop over t: ``(hs [T, B, H], h_T)``.  Gate math and the carried state in fp32, ``hs`` and
    ``h_T`` in the dtype of ``x``.  ``sequence_length`` [B]: at ``t >= length`` a row emits zeros and keeps its state.
    ``reverse``: t runs from ``T - 1`` down to 0 (the padding steps first, leaving the initial state in place)."""
    t_n, b_n, i_n = x.shape
    h_n = cand_kernel.shape[1]
    wg, wc = gates_kernel.to(x.dtype), cand_kernel.to(x.dtype)
    xg = torch.matmul(x.reshape(t_n * b_n, i_n), torch.cat([wg[:i_n], wc[:i_n]], 1))
    xg = (xg + torch.cat([gates_bias, cand_bias]).to(x.dtype)).reshape(t_n, b_n, 3 * h_n).float()
    wgh, wch = wg[i_n:].float(), wc[i_n:].float()
    h = h0.float()
    if sequence_length is not None:
        sequence_length = torch.as_tensor(sequence_length, device=x.device).reshape(b_n, 1)
    outs = [None] * t_n
    for t in (range(t_n - 1, -1, -1) if reverse else range(t_n)):
        hb = h.to(x.dtype).float()                                      # the products see h in the dtype of x
        r, u = torch.sigmoid(xg[t, :, :2 * h_n] + torch.matmul(hb, wgh)).split(h_n, 1)
        c = torch.tanh(xg[t, :, 2 * h_n:] + torch.matmul((r * h).to(x.dtype).float(), wch))
        h_new = u * h + (1.0 - u) * c
        if sequence_length is None:
            h = h_new
            outs[t] = h.to(x.dtype)
        else:
            live = sequence_length > t
            h = torch.where(live, h_new, h)
            outs[t] = torch.where(live, h_new, torch.zeros_like(h_new)).to(x.dtype)
    return torch.stack(outs, 0), h.to(x.dtype)


def _aligned(*ts):
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts)


class _GRU(torch.autograd.Function):
    """``ndir`` (1 or 2) GRUs over the same ``x`` and lengths, direction d reversed where bit d of ``reverse`` is set;
    ``params``: ``gates_kernel, gates_bias, cand_kernel, cand_bias, h0`` per direction; returns ``hs, h_T`` per
    direction."""

    @staticmethod
    def forward(ctx, x, lens, reverse, *params):
        from . import gemm
        ndir = len(params) // 5
        t_n, b_n, i_n = x.shape
        h_n = params[2].shape[1]
        dev = x.device
        x = x.contiguous()
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        ws, bs = [], []
        for d in range(ndir):
            gk, gb, ck, cb = params[5 * d:5 * d + 4]
            ws += [gk[:i_n], ck[:i_n]]
            bs += [gb.to(x.dtype), cb.to(x.dtype)]
        # the input halves of r | u | c of all directions, biases included: one product, [T * B, ndir * 3H]
        xg = gemm.dense_multi(x.view(t_n * b_n, i_n), ws, bs).contiguous()
        rows, saved, outs = [], [], []
        for d in range(ndir):
            gk, ck = params[5 * d].contiguous(), params[5 * d + 2].contiguous()
            h0 = params[5 * d + 4]
            h0b, h0f = h0.to(torch.bfloat16).contiguous(), h0.float().contiguous()
            hs, rh = new((t_n, b_n, h_n), torch.bfloat16), new((t_n, b_n, h_n), torch.bfloat16)
            hf, gates = new((t_n, b_n, h_n), torch.float32), new((t_n, b_n, 3 * h_n), torch.bfloat16)
            wt, h_fin = new(3 * h_n * h_n, torch.bfloat16), new((b_n, h_n), torch.bfloat16)
            if not _aligned(gk[i_n:], ck[i_n:], h0b, h0f) or xg.data_ptr() % 16:
                raise RuntimeError("mdtf gru: operands must be 16-byte aligned")
            rows.append((xg[:, 3 * h_n * d:], gk[i_n:], ck[i_n:], wt, h0b, h0f, hs, hf, rh, gates, h_fin))
            saved += [gk, ck, h0b, h0f, hs, hf, rh, gates]
            outs += [hs, h_fin]
        # full length, forward in time, one direction: the kernels without the length and direction logic, which are
        # 1.2 to 1.8 us a step faster (profiles/gru.md) and give the same bits
        ctx.plain = lens is None and ndir == 1 and not reverse
        if ctx.plain:
            N.check(N.fn("mdtf_gru_fwd")(*[N.ptr(z) for z in rows[0][:10]], t_n, b_n, h_n, BF16, N.stream_ptr()),
                    "gru_fwd")
            outs[1].copy_(outs[0][-1])
        else:
            N.check(N.fn("mdtf_gru_fwd_seq")(rnn._table(rows), ndir, reverse, N.ptr(lens), t_n, b_n, h_n, xg.shape[1],
                                             BF16, N.stream_ptr()), "gru_fwd_seq")
        ctx.save_for_backward(x, lens, *saved)
        ctx.reverse, ctx.like = reverse, params
        ctx.sinks = [[V.grad_sink(p) for p in params[5 * d:5 * d + 4]] for d in range(ndir)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        from . import gemm
        x, lens = ctx.saved_tensors[:2]
        saved = ctx.saved_tensors[2:]
        ndir = len(saved) // 8
        t_n, b_n, i_n = x.shape
        h_n = saved[1].shape[1]
        dev = x.device
        x2 = x.view(t_n * b_n, i_n)
        rows, keep = [], []
        for d in range(ndir):
            gk, ck, h0b, h0f, hs, hf, rh, gates = saved[8 * d:8 * d + 8]
            dhs = grads[2 * d].to(torch.bfloat16).contiguous()
            carry = grads[2 * d + 1].float().clone()                    # dL/dh_T in, dL/dh_0 out
            dg = torch.empty((t_n, b_n, 3 * h_n), dtype=torch.bfloat16, device=dev)
            rows.append((gk[i_n:], ck[i_n:], gates, hf, h0f, dhs, carry, dg))
            keep.append((dg.view(t_n * b_n, 3 * h_n), carry))
        if ctx.plain:
            N.check(N.fn("mdtf_gru_bwd")(*[N.ptr(z) for z in rows[0]], t_n, b_n, h_n, BF16, N.stream_ptr()), "gru_bwd")
        else:
            N.check(N.fn("mdtf_gru_bwd_seq")(rnn._table(rows), ndir, ctx.reverse, N.ptr(lens), t_n, b_n, h_n, BF16,
                                             N.stream_ptr()), "gru_bwd_seq")
        dx, out = None, []
        for d in range(ndir):
            gk, ck, h0b, _, hs, _, rh, _ = saved[8 * d:8 * d + 8]
            like = ctx.like[5 * d:5 * d + 5]
            dg2, carry = keep[d]
            dgate, dpc = dg2[:, :2 * h_n], dg2[:, 2 * h_n:]
            if ctx.needs_input_grad[0]:
                wx = torch.cat([gk[:i_n], ck[:i_n]], 1)
                if dx is None:
                    dx = gemm._hand_dgrad(dg2, wx)
                    if dx is None:
                        dx = torch.mm(dg2, wx.t())
                else:
                    dx.addmm_(dg2, wx.t())                              # the second direction adds into the first's
            grads_d = [None] * 4
            if any(ctx.needs_input_grad[3 + 5 * d:7 + 5 * d]):
                slots = [V.slot_or_zeros(s, p.shape, dev) for s, p in zip(ctx.sinks[d], like[:4])]
                sgk, sgb, sck, scb = slots
                if not gemm.wgrad_into(sgk[:i_n], x2, dgate, sgb):
                    sgb.add_(torch.sum(dgate, 0, dtype=torch.float32))  # (a fixed-order sum: repeatable)
                gemm.wgrad_into(sgk[i_n:], rnn._h_prev(h0b, hs, lens, (ctx.reverse >> d) & 1), dgate)
                if not gemm.wgrad_into(sck[:i_n], x2, dpc, scb):
                    scb.add_(torch.sum(dpc, 0, dtype=torch.float32))
                gemm.wgrad_into(sck[i_n:], rh.view(t_n * b_n, h_n), dpc)
                grads_d = [V.grad_marker(p) if s is not None else g.to(p.dtype)
                           for s, g, p in zip(ctx.sinks[d], slots, like[:4])]
            out += grads_d + [carry.to(like[4].dtype)]
        if dx is not None:
            dx = dx.view(t_n, b_n, i_n)
        return (dx, None, None) + tuple(out)


def _check_args(x, gk, gb, ck, cb, h0, sequence_length):
    if x.dim() != 3:
        raise ValueError("gru: x must be [T, B, I], got %s" % (tuple(x.shape),))
    t_n, b_n, i_n = x.shape
    if ck.dim() != 2 or ck.shape[0] != i_n + ck.shape[1]:
        raise ValueError("gru: candidate kernel must be [I + H, H] with I = %d, got %s" % (i_n, tuple(ck.shape)))
    h_n = ck.shape[1]
    for name, t, shape in (("gates kernel", gk, (i_n + h_n, 2 * h_n)), ("gates bias", gb, (2 * h_n,)),
                           ("candidate bias", cb, (h_n,)), ("initial state", h0, (b_n, h_n))):
        if tuple(t.shape) != shape:
            raise ValueError("gru: %s must be %s, got %s" % (name, list(shape), tuple(t.shape)))
    if sequence_length is not None and len(sequence_length) != b_n:
        raise ValueError("gru: sequence_length must have %d entries" % b_n)


def _cast(p, dtype):
    """A direction's ``(gates_kernel, gates_bias, cand_kernel, cand_bias, h0)`` with both kernels in ``dtype``."""
    return tuple(t.to(dtype) if j in (0, 2) and t.dtype != dtype else t for j, t in enumerate(p))


def gru(x, gates_kernel, gates_bias, cand_kernel, cand_bias, h0, sequence_length=None, reverse=False):
    """``(hs, h_T)`` of the GRU over time-major ``x`` [T, B, I] from the state ``h0`` [B, H] (any dtype; its gradient
    comes back in that dtype), in the ``reverse`` direction if asked.  ``h_T`` is in the dtype of ``x`` and has the
    bits of ``hs`` at each row's last visited live step (``hs[-1]`` on a full-length forward call)."""
    p = (gates_kernel, gates_bias, cand_kernel, cand_bias, h0)
    _check_args(x, *p, sequence_length)
    if native_ok(x, cand_kernel, h0, sequence_length):
        return _GRU.apply(x, rnn._device_lengths(sequence_length, x.device), int(bool(reverse)), *_cast(p, x.dtype))
    return gru_loop(x, *p, sequence_length, reverse)


def bigru(x, fw, bw, sequence_length=None):
    """A forward-in-time and a reverse GRU over the same ``x`` [T, B, I] and lengths: ``((hs, h_T) of fw, the same of
    bw)`` for ``fw`` / ``bw`` = ``(gates_kernel, gates_bias, cand_kernel, cand_bias, h0)``.  With the same ``H`` on the
    kernel path every pair of step launches runs step s of ``fw`` and step ``T - 1 - s`` of ``bw``; otherwise the
    directions run as two calls of :func:`gru`."""
    for p in (fw, bw):
        _check_args(x, *p, sequence_length)
    if fw[2].shape == bw[2].shape and native_ok(x, fw[2], fw[4], sequence_length) and bw[4].is_cuda:
        out = _GRU.apply(x, rnn._device_lengths(sequence_length, x.device), 0b10, *_cast(fw, x.dtype),
                         *_cast(bw, x.dtype))
        return out[:2], out[2:]
    if sequence_length is not None and x.is_cuda:
        sequence_length = rnn._device_lengths(sequence_length, x.device)    # copied once for both calls
    return gru(x, *fw, sequence_length), gru(x, *bw, sequence_length, True)
