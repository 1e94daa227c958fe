"""GRU over a time-major sequence (``tf.nn.dynamic_rnn`` over a ``GRUCell``) on the kernels of ``csrc/gru.hip``.

The cell is TF's ``GRUCell``, which applies the reset gate before the candidate product, for ``x`` [T, B, I],
``gates_kernel`` [I + H, 2H], ``gates_bias`` [2H], ``cand_kernel`` [I + H, H] and ``cand_bias`` [H]::

    [r u] = sigmoid([x_t, h_{t-1}] @ gates_kernel + gates_bias)
    c     = tanh([x_t, r * h_{t-1}] @ cand_kernel + cand_bias)
    h_t   = u * h_{t-1} + (1 - u) * c

The HIP path runs for GPU tensors in bf16 with ``H % 32 == 0``, full length, forward in time.  The input half
``xg = x @ [gates_kernel[:I] | cand_kernel[:I]] + [gates_bias | cand_bias]`` over all ``T * B`` rows is one dense
forward; the recurrence is two launches per step (``r``, ``u`` and ``r * h``; then the candidate and the update), all
enqueued by one call of ``mdtf_gru_fwd``, and ``2T + 1`` launches of ``mdtf_gru_bwd`` backwards.  The state is carried
in fp32 inside the call (``h`` is a leaky integrator: a bf16 carry loses the update where ``u`` is near 1); ``hs``, and
with it the returned state, are its bf16 rounding, so ``h_T`` is bit for bit ``hs[-1]``.  Both kernel gradients and
both bias gradients are ``gemm.wgrad_into`` on the row ranges of the variables' fp32 gradient slots when there are
any, and ``dx`` is the dense data gradient over ``[gates_kernel[:I] | cand_kernel[:I]]``.

Every other case runs :func:`gru_loop`, the definition as a PyTorch loop with fp32 gate math and an fp32 carry: CPU
tensors, ``MDTF_KERNELS=torch`` (the comparator), fp32 activations, other ``H``, and any call with
``sequence_length``.  Not here: the reset-after (Keras / cuDNN) cell, vanilla cells and multi-cell wrappers.
"""
import torch

from . import _native as N
from ..train import variables as V

BF16 = 0        # dtype codes of the entry points (the kernels take only bf16)
FP32 = 1
N.register("mdtf_gru_units", [N.I] * 4)
N.register("mdtf_gru_force_units", [N.I] * 2)
N.register("mdtf_gru_fwd", [N.P] * 10 + [N.I] * 4 + [N.P])
N.register("mdtf_gru_bwd", [N.P] * 8 + [N.I] * 4 + [N.P])


def native_ok(x, cand_kernel, h0, sequence_length=None):
    """Whether the HIP kernels take this call (else the PyTorch loop runs)."""
    t, b, i = x.shape
    h = cand_kernel.shape[1]
    return (sequence_length is None and N.use_native(x) and x.dtype == torch.bfloat16 and h % 32 == 0 and h >= 32
            and t >= 1 and b >= 1 and i >= 1 and h0.is_cuda and b * 3 * h < (1 << 31) and b <= 16 * 65535)


def units_per_block(t, b, h):
    """Hidden units a block owns for this problem, ``(gate launch, the other launches)``, each 16 or 32."""
    code = int(N.fn("mdtf_gru_units")(t, b, h, BF16))
    return code & 0xFF, code >> 8


def gru_loop(x, gates_kernel, gates_bias, cand_kernel, cand_bias, h0, sequence_length=None):
    """The definition as a loop over t: ``(hs [T, B, H], h_T)``.  Gate math and the carried state in fp32, ``hs`` and
    ``h_T`` in the dtype of ``x``.  ``sequence_length`` [B]: at ``t >= length`` a row emits zeros and keeps its state."""
    t_n, b_n, i_n = x.shape
    h_n = cand_kernel.shape[1]
    wg, wc = gates_kernel.to(x.dtype), cand_kernel.to(x.dtype)
    xg = torch.matmul(x.reshape(t_n * b_n, i_n), torch.cat([wg[:i_n], wc[:i_n]], 1))
    xg = (xg + torch.cat([gates_bias, cand_bias]).to(x.dtype)).reshape(t_n, b_n, 3 * h_n).float()
    wgh, wch = wg[i_n:].float(), wc[i_n:].float()
    h = h0.float()
    if sequence_length is not None:
        sequence_length = torch.as_tensor(sequence_length, device=x.device).reshape(b_n, 1)
    outs = []
    for t in range(t_n):
        hb = h.to(x.dtype).float()                                      # the products see h in the dtype of x
        r, u = torch.sigmoid(xg[t, :, :2 * h_n] + torch.matmul(hb, wgh)).split(h_n, 1)
        c = torch.tanh(xg[t, :, 2 * h_n:] + torch.matmul((r * h).to(x.dtype).float(), wch))
        h_new = u * h + (1.0 - u) * c
        if sequence_length is None:
            h = h_new
            outs.append(h.to(x.dtype))
        else:
            live = sequence_length > t
            h = torch.where(live, h_new, h)
            outs.append(torch.where(live, h_new, torch.zeros_like(h_new)).to(x.dtype))
    return torch.stack(outs, 0), h.to(x.dtype)


def _aligned(*ts):
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts)


class _GRU(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, gk, gb, ck, cb, h0):
        from . import gemm
        t_n, b_n, i_n = x.shape
        h_n = ck.shape[1]
        dev = x.device
        ctx.like = (gk, gb, ck, cb, h0)
        ctx.sinks = [V.grad_sink(p) for p in (gk, gb, ck, cb)]
        x = x.contiguous()
        gk, ck = gk.contiguous(), ck.contiguous()
        h0b, h0f = h0.to(torch.bfloat16).contiguous(), h0.float().contiguous()
        # the input halves of r | u | c, biases included: one product, [T * B, 3H]
        xg = gemm.dense_multi(x.view(t_n * b_n, i_n), [gk[:i_n], ck[:i_n]], [gb.to(x.dtype), cb.to(x.dtype)]).contiguous()
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        hs, rh = new((t_n, b_n, h_n), torch.bfloat16), new((t_n, b_n, h_n), torch.bfloat16)
        hf, gates = new((t_n, b_n, h_n), torch.float32), new((t_n, b_n, 3 * h_n), torch.bfloat16)
        wt = new(3 * h_n * h_n, torch.bfloat16)
        if not _aligned(xg, gk[i_n:], ck[i_n:], h0b, h0f):
            raise RuntimeError("mdtf gru: operands must be 16-byte aligned")
        N.check(N.fn("mdtf_gru_fwd")(N.ptr(xg), N.ptr(gk[i_n:]), N.ptr(ck[i_n:]), N.ptr(wt), N.ptr(h0b), N.ptr(h0f),
                                     N.ptr(hs), N.ptr(hf), N.ptr(rh), N.ptr(gates), t_n, b_n, h_n, BF16,
                                     N.stream_ptr()), "gru_fwd")
        ctx.save_for_backward(x, gk, ck, h0b, h0f, hs, hf, rh, gates)
        return hs, hs[-1].clone()

    @staticmethod
    def backward(ctx, dhs, dh_t):
        from . import gemm
        x, gk, ck, h0b, h0f, hs, hf, rh, gates = ctx.saved_tensors
        t_n, b_n, i_n = x.shape
        h_n = ck.shape[1]
        dev = x.device
        dhs = dhs.to(torch.bfloat16).contiguous()
        carry = dh_t.float().clone()                                    # dL/dh_T in, dL/dh_0 out
        dg = torch.empty((t_n, b_n, 3 * h_n), dtype=torch.bfloat16, device=dev)
        N.check(N.fn("mdtf_gru_bwd")(N.ptr(gk[i_n:]), N.ptr(ck[i_n:]), N.ptr(gates), N.ptr(hf), N.ptr(h0f), N.ptr(dhs),
                                     N.ptr(carry), N.ptr(dg), t_n, b_n, h_n, BF16, N.stream_ptr()), "gru_bwd")
        x2, dg2 = x.view(t_n * b_n, i_n), dg.view(t_n * b_n, 3 * h_n)
        dgate, dpc = dg2[:, :2 * h_n], dg2[:, 2 * h_n:]
        dx = None
        if ctx.needs_input_grad[0]:
            wx = torch.cat([gk[:i_n], ck[:i_n]], 1)
            dx = gemm._hand_dgrad(dg2, wx)
            if dx is None:
                dx = torch.mm(dg2, wx.t())
            dx = dx.view(t_n, b_n, i_n)
        grads = [None] * 4
        if any(ctx.needs_input_grad[1:5]):
            gk_like, gb_like, ck_like, cb_like = ctx.like[:4]
            slots = [V.slot_or_zeros(s, p.shape, dev) for s, p in zip(ctx.sinks, ctx.like[:4])]
            sgk, sgb, sck, scb = slots
            h_prev = torch.cat([h0b[None], hs[:-1]], 0).view(t_n * b_n, h_n)
            if not gemm.wgrad_into(sgk[:i_n], x2, dgate, sgb):
                sgb.add_(torch.sum(dgate, 0, dtype=torch.float32))      # (a fixed-order sum: repeatable)
            gemm.wgrad_into(sgk[i_n:], h_prev, dgate)
            if not gemm.wgrad_into(sck[:i_n], x2, dpc, scb):
                scb.add_(torch.sum(dpc, 0, dtype=torch.float32))
            gemm.wgrad_into(sck[i_n:], rh.view(t_n * b_n, h_n), dpc)
            grads = [V.grad_marker(p) if s is not None else g.to(p.dtype)
                     for s, g, p in zip(ctx.sinks, slots, ctx.like[:4])]
        return (dx,) + tuple(grads) + (carry.to(ctx.like[4].dtype),)


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


def gru(x, gates_kernel, gates_bias, cand_kernel, cand_bias, h0, sequence_length=None):
    """``(hs, h_T)`` of the GRU over time-major ``x`` [T, B, I] from the state ``h0`` [B, H] (any dtype; its gradient
    comes back in that dtype).  ``h_T`` is in the dtype of ``x`` and equals ``hs[-1]`` bit for bit on a full-length
    call."""
    _check_args(x, gates_kernel, gates_bias, cand_kernel, cand_bias, h0, sequence_length)
    if native_ok(x, cand_kernel, h0, sequence_length):
        gk = gates_kernel if gates_kernel.dtype == x.dtype else gates_kernel.to(x.dtype)
        ck = cand_kernel if cand_kernel.dtype == x.dtype else cand_kernel.to(x.dtype)
        return _GRU.apply(x, gk, gates_bias, ck, cand_bias, h0)
    return gru_loop(x, gates_kernel, gates_bias, cand_kernel, cand_bias, h0, sequence_length)
