"""Per-row lengths, the reverse direction and ``bidirectional_dynamic_rnn`` on the kernels of ``csrc/lstm.hip``
(``cuda``) and on the PyTorch loop (``cpu``) against the fp64 oracle of ``lstm_helpers``.  The reverse direction's
oracle is the same oracle on inputs and output gradients put through ``reverse_sequence``, its ``outputs`` and ``dx``
put back.

Limits.  ``cpu``: ``gamma(I + H + 8)``.  ``cuda``: twice the error of the fp32 expression with the kernels' bf16
rounding points (never the kernels), worst over the three cases, both directions and the two-direction form, from

    python -m bench.lstm_tolerance --lengths

    case b fw outputs=2.624e-03 h_T=1.249e-03 c_T=1.526e-03 dx=3.600e-03 dkernel=3.432e-03 dbias=3.023e-03 dh0=1.593e-03 dc0=1.952e-03
    case b bw outputs=1.991e-03 h_T=8.260e-04 c_T=1.795e-03 dx=2.911e-03 dkernel=2.812e-03 dbias=3.596e-03 dh0=1.593e-03 dc0=2.528e-03
    case b bidirectional bw outputs=2.425e-03 h_T=9.668e-04 c_T=6.935e-04 dx=2.992e-03 dkernel=2.754e-03 dbias=2.590e-03 dh0=8.105e-04 dc0=2.251e-03
    case d fw outputs=3.146e-03 h_T=2.940e-03 c_T=1.240e-03 dx=3.348e-03 dkernel=4.357e-03 dbias=2.485e-03 dh0=3.603e-03 dc0=4.093e-03
    case d bw outputs=3.261e-03 h_T=2.940e-03 c_T=1.238e-03 dx=3.024e-03 dkernel=3.422e-03 dbias=2.669e-03 dh0=3.450e-03 dc0=4.093e-03
    case d bidirectional bw outputs=3.675e-03 h_T=2.338e-03 c_T=1.159e-03 dx=3.748e-03 dkernel=3.571e-03 dbias=2.460e-03 dh0=3.462e-03 dc0=2.519e-03
    case u32 fw outputs=3.147e-03 h_T=1.124e-03 c_T=8.868e-04 dx=4.357e-03 dkernel=2.203e-03 dbias=2.657e-03 dh0=2.163e-03 dc0=3.407e-03
    case u32 bw outputs=2.763e-03 h_T=1.124e-03 c_T=9.253e-04 dx=3.694e-03 dkernel=2.488e-03 dbias=2.067e-03 dh0=2.163e-03 dc0=3.675e-03

("bidirectional bw": the second direction of the pair, with the parameters of ``other``; its dx is the pair's.)
"""
import functools
import os
import sys
import types

import pytest
import torch

import mdtf
from mdtf.ops import _native, rnn
from mdtf.train import variables as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_helpers as LH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
State = mdtf.nn.rnn_cell.LSTMStateTuple
# u32 (2, 256, 8, 512): the U = 32 kernels; rows 16-31 die after step 0 (a whole dead tile), rows 32-47 never live
LENGTHS = {"b": (3, 0, 2, 3, 1), "d": (4, 3, 2, 1) * 4 + (2,),
           "u32": (2,) * 16 + (1,) * 16 + (0,) * 16 + (2,) * 208}
U32 = (2, 256, 8, 512)
PAIRS = ("b", "d")               # the cases of the bidirectional test
MEASURED_LENGTHS = {"outputs": 3.68e-03, "h_T": 2.94e-03, "c_T": 1.80e-03, "dx": 4.36e-03, "dkernel": 4.36e-03,
                    "dbias": 3.60e-03, "dh0": 3.60e-03, "dc0": 4.09e-03}
LIMIT = {k: 2.0 * v for k, v in MEASURED_LENGTHS.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    if name != "u32":
        return LH.case(name, LENGTHS[name])
    (t, b, i, h), s = U32, 2000
    c = types.SimpleNamespace(
        shape=U32, lengths=LENGTHS[name], x=NH.randn((t, b, i), s), kernel=NH.randn((i + h, 4 * h), s + 1, (i + h) ** -0.5),
        bias=NH.randn((4 * h,), s + 2, 0.25), h0=NH.randn((b, h), s + 3, 0.5), c0=NH.randn((b, h), s + 4, 0.5),
        dhs=NH.randn((t, b, h), s + 5), dh_t=NH.randn((b, h), s + 6), dc_t=NH.randn((b, h), s + 7))
    c.ref = LH.oracle(c.x, c.kernel, c.bias, c.h0, c.c0, c.dhs, c.dh_t, c.dc_t, c.lengths)
    return c


def other(c):
    """Different parameters, state and gradients of the same shapes (for the second direction of a pair)."""
    return types.SimpleNamespace(shape=c.shape, lengths=c.lengths, x=c.x, kernel=c.kernel.flip(1) * 0.5, bias=-c.bias,
                                 h0=c.c0, c0=c.h0, dhs=-c.dhs, dh_t=c.dc_t, dc_t=c.dh_t)


def reverse_sequence(x, lengths):
    t = torch.arange(x.shape[0])[:, None]
    n = torch.tensor(lengths)[None]
    return x[torch.where(t < n, n - 1 - t, t), torch.arange(x.shape[1])[None]]


@functools.lru_cache(maxsize=None)
def reference(name, direction, alt=False):
    c = other(case(name)) if alt else case(name)
    if direction == "fw":
        return c.ref if not alt else LH.oracle(c.x, c.kernel, c.bias, c.h0, c.c0, c.dhs, c.dh_t, c.dc_t, c.lengths)
    rev = functools.partial(reverse_sequence, lengths=c.lengths)
    ref = LH.oracle(rev(c.x), c.kernel, c.bias, c.h0, c.c0, rev(c.dhs), c.dh_t, c.dc_t, c.lengths)
    return dict(ref, outputs=rev(ref["outputs"]), dx=rev(ref["dx"]))


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _run(device, cs, directions, lengths, slot0=None):
    """Forward + backward of one direction (``dynamic_rnn`` for fw, ``rnn.lstm(reverse=True)`` for bw) or of an
    fw / bw pair (``bidirectional_dynamic_rnn``) on variables holding the parameters of ``cs``: a dict over
    ``LH.NAMES`` per direction.  cuda: bf16 tensors, fp32 gradient slots (the first kernel's holding ``slot0``)."""
    put = (lambda t: NH.put(t, device)) if device == "cuda" else (lambda t: t.clone())
    V.reset_default_graph()
    store = V.get_store()
    store.device, store.compute_dtype = torch.device(device), torch.bfloat16 if device == "cuda" else None
    pair = len(cs) == 2
    scopes = ["bidirectional_rnn/%s/lstm_cell" % d for d in directions] if pair else ["rnn/lstm_cell"]
    vs, leaves = [], []
    for c, scope in zip(cs, scopes):
        with mdtf.variable_scope(scope):
            mdtf.get_variable("kernel", c.kernel.shape, initializer=lambda *a, c=c, **k: c.kernel.clone())
            mdtf.get_variable("bias", c.bias.shape, initializer=lambda *a, c=c, **k: c.bias.clone())
        vs.append((store.variable(scope + "/kernel"), store.variable(scope + "/bias")))
        if device == "cuda":
            fill = slot0 if slot0 is not None and not leaves else torch.zeros(c.kernel.shape)
            vs[-1][0].grad, vs[-1][1].grad = fill.to(device).contiguous(), torch.zeros(c.bias.shape, device=device)
        leaves.append((put(c.h0).requires_grad_(True), c.c0.clone().to(device).requires_grad_(True)))
    x = put(cs[0].x).requires_grad_(True)
    cells = [mdtf.nn.rnn_cell.LSTMCell(c.shape[3], forget_bias=LH.FORGET_BIAS) for c in cs]
    states = [State(c0, h0) for h0, c0 in leaves]
    with mdtf.variable_scope("", reuse=True):
        if pair:
            outs, fin = mdtf.nn.bidirectional_dynamic_rnn(cells[0], cells[1], x, lengths, states[0], states[1],
                                                          time_major=True)
        elif directions[0] == "fw":
            out, st = mdtf.nn.dynamic_rnn(cells[0], x, sequence_length=lengths, initial_state=states[0], time_major=True)
            outs, fin = [out], [st]
        else:
            with mdtf.variable_scope("rnn"):
                kernel, bias = cells[0].variables(x.shape[2])
            out, h_t, c_t = rnn.lstm(x, kernel, bias, leaves[0][0], leaves[0][1], LH.FORGET_BIAS, lengths, reverse=True)
            outs, fin = [out], [State(c_t, h_t)]
    ys = [y for out, st in zip(outs, fin) for y in (out, st.h, st.c)]
    gs = [g for c in cs for g in (c.dhs, c.dh_t, c.dc_t)]
    torch.autograd.backward(ys, [g.to(device).to(y.dtype) for g, y in zip(gs, ys)])
    return [dict(zip(LH.NAMES, (out, st.h, st.c, x.grad, kv.grad, bv.grad, h0.grad, c0.grad)))
            for out, st, (kv, bv), (h0, c0) in zip(outs, fin, vs, leaves)]


def _check(what, got, ref, shape, device, lengths, direction, slot0=None):
    if slot0 is not None:
        got = dict(got, dkernel=got["dkernel"].detach().cpu().double() - slot0.double())
    for k, e in LH.errors(got, ref).items():
        limit = LIMIT[k] if device == "cuda" else LH.gamma(shape[2] + shape[3] + 8)
        print("LSTM_LEN_ERR %-24s %-8s %.3e (limit %.3e)" % (what, k, e, limit))
        assert e <= limit, "%s %s: error %.3e of max |ref| above %.3e" % (what, k, e, limit)
    out = got["outputs"].detach()
    for b, n in enumerate(lengths):
        assert n == shape[0] or float(out[n:, b].abs().max()) == 0.0, (what, b)      # dead outputs are exactly zero
        if n:                                     # h_T is the output of the row's last visited live step, bit for bit
            assert NH.bits_equal(got["h_T"][b], out[n - 1 if direction == "fw" else 0, b]), (what, b)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("direction", ["fw", "bw"])
@pytest.mark.parametrize("name", list(LENGTHS))
def test_lengths_one_direction(name, direction, device):
    device = _device(device)
    c = case(name)
    if device == "cuda":
        assert rnn.native_ok(NH.put(c.x, device), NH.put(c.kernel, device), NH.put(c.h0, device), c.lengths)
        assert name != "u32" or rnn.units_per_block(2, 256, 512) == 32
    got, = _run(device, [c], [direction], c.lengths)
    _check("%s %s %s" % (name, direction, device), got, reference(name, direction), c.shape, device, c.lengths, direction)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", PAIRS)
def test_bidirectional_dynamic_rnn(name, device):
    device = _device(device)
    cs = [case(name), other(case(name))]
    refs = [reference(name, "fw"), reference(name, "bw", True)]
    refs = [dict(r, dx=refs[0]["dx"] + refs[1]["dx"]) for r in refs]          # x feeds both directions
    slot0 = NH.randn(cs[0].kernel.shape, 7) if device == "cuda" else None     # a filled slot: dkernel adds into it
    got = _run(device, cs, ["fw", "bw"], cs[0].lengths, slot0)
    names = {v.name for v in V.get_store().trainable_variables()}
    assert names == {"bidirectional_rnn/%s/lstm_cell/%s" % (d, p) for d in ("fw", "bw") for p in ("kernel", "bias")}
    for g, r, d in zip(got, refs, ("fw", "bw")):
        _check("bi %s %s %s" % (name, d, device), g, r, cs[0].shape, device, cs[0].lengths, d, slot0 if d == "fw" else None)
    if device == "cuda":
        again = _run(device, cs, ["fw", "bw"], cs[0].lengths, slot0)
        for g, a in zip(got, again):
            for k in LH.NAMES:
                assert NH.bits_equal(g[k], a[k]), k


@pytest.mark.parametrize("device", GPU_ONLY)
def test_the_kernels_read_the_lengths(device):
    device = _device(device)
    c = case("b")
    lens = torch.full((5,), 3, dtype=torch.int32, device=device)
    _run(device, [c], ["fw"], lens)
    lens.copy_(torch.tensor(c.lengths, dtype=torch.int32))                   # in place: the same device buffer
    for direction in ("fw", "bw"):
        got, = _run(device, [c], [direction], lens)
        _check("device lengths " + direction, got, reference("b", direction), c.shape, device, c.lengths, direction)


@pytest.mark.parametrize("device", GPU_ONLY)
def test_no_lengths_forward_matches_the_plain_entry_points_bit_for_bit(device):
    device = _device(device)
    c = LH.case("c")
    (t, b, i, h), P, st = c.shape, _native.ptr, _native.stream_ptr()
    new = lambda *shape, dtype=torch.bfloat16: torch.full(shape, 7.0, dtype=dtype, device=device)
    xg = NH.put(c.x.reshape(t * b, i) @ c.kernel[:i] + c.bias, device).contiguous()
    wh, h0, c0 = NH.put(c.kernel[i:], device).contiguous(), NH.put(c.h0, device), c.c0.to(device)
    dhs, dh_t = NH.put(c.dhs, device), NH.put(c.dh_t, device)
    res = []
    for seq in (False, True):
        wt, hs, cs, gates = new(4 * h * h), new(t, b, h), new(t, b, h, dtype=torch.float32), new(t, b, 4 * h)
        h_fin, c_fin, carry = new(b, h), new(b, h, dtype=torch.float32), c.dc_t.to(device)
        dg, dh0 = new(t, b, 4 * h), new(b, h)
        if seq:
            fwd = rnn._table([(xg, wh, wt, h0, c0, hs, cs, gates, h_fin, c_fin)])
            bwd = rnn._table([(wh, gates, cs, c0, dhs, dh_t, carry, dg, dh0)])
            assert _native.fn("mdtf_lstm_fwd_seq")(fwd, 1, 0, None, t, b, h, 4 * h, 1.0, 0, st) == 0
            assert _native.fn("mdtf_lstm_bwd_seq")(bwd, 1, 0, None, t, b, h, 0, st) == 0
            assert NH.bits_equal(h_fin, hs[-1]) and NH.bits_equal(c_fin, cs[-1])
        else:
            assert _native.fn("mdtf_lstm_fwd")(P(xg), P(wh), P(wt), P(h0), P(c0), P(hs), P(cs), P(gates), t, b, h, 1.0,
                                               0, st) == 0
            assert _native.fn("mdtf_lstm_bwd")(P(wh), P(gates), P(cs), P(c0), P(dhs), P(dh_t), P(carry), P(dg), P(dh0),
                                               t, b, h, 0, st) == 0
        res.append((hs, cs, gates, dg, dh0, carry))
    for old, seq in zip(*res):
        assert NH.bits_equal(old, seq)
