"""``mdtf.nn.dynamic_rnn`` over an ``LSTMCell``, the kernels of ``csrc/lstm.hip`` and the PyTorch loop against the fp64
oracle of ``lstm_helpers``.  ``cpu`` runs the loop on fp32 tensors of bf16-representable values; ``cuda`` runs the HIP
kernels on bf16 tensors, the kernel gradient landing in an fp32 slot.  The limits are explained in ``lstm_helpers``.
"""
import os
import sys

import pytest
import torch

import mdtf
from mdtf.ops import _native
from mdtf.train import variables as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_helpers as LH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
UNSUPPORTED = -2
State = mdtf.nn.rnn_cell.LSTMStateTuple


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _run(device, c, slot0=None, fp32=False):
    """Forward + backward through ``mdtf.nn.dynamic_rnn`` on variables holding the case's kernel and bias; a dict
    over ``LH.NAMES``.  cuda: bf16 tensors (``fp32``: fp32 ones), fp32 state ``c``, fp32 gradient slots."""
    bf16 = device == "cuda" and not fp32
    put = (lambda t: NH.put(t, device)) if bf16 else (lambda t: t.clone().to(device))
    V.reset_default_graph()
    store = V.get_store()
    store.device, store.compute_dtype = torch.device(device), torch.bfloat16 if bf16 else None
    with mdtf.variable_scope("rnn/lstm_cell"):
        mdtf.get_variable("kernel", c.kernel.shape, initializer=lambda *a, **k: c.kernel.clone())
        mdtf.get_variable("bias", c.bias.shape, initializer=lambda *a, **k: c.bias.clone())
    kv, bv = store.variable("rnn/lstm_cell/kernel"), store.variable("rnn/lstm_cell/bias")
    if device == "cuda":
        kv.grad = (slot0 if slot0 is not None else torch.zeros(c.kernel.shape)).to(device).contiguous()
        bv.grad = torch.zeros(c.bias.shape, device=device)
    x, h0 = put(c.x).requires_grad_(True), put(c.h0).requires_grad_(True)
    c0 = c.c0.clone().to(device).requires_grad_(True)
    cell = mdtf.nn.rnn_cell.LSTMCell(c.shape[3], forget_bias=LH.FORGET_BIAS)
    with mdtf.variable_scope("", reuse=True):
        out, (c_t, h_t) = mdtf.nn.dynamic_rnn(cell, x, sequence_length=c.lengths, initial_state=State(c0, h0),
                                              time_major=True)
    assert out.dtype == x.dtype and h_t.dtype == x.dtype and c_t.dtype == torch.float32
    torch.autograd.backward([out, h_t, c_t], [g.to(device).to(t.dtype)
                                              for g, t in ((c.dhs, out), (c.dh_t, h_t), (c.dc_t, c_t))])
    assert kv.grad.dtype == torch.float32 and bv.grad.dtype == torch.float32
    return dict(zip(LH.NAMES, (out, h_t, c_t, x.grad, kv.grad, bv.grad, h0.grad, c0.grad)))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", list("abcde"))
def test_geometry_case(name, device):
    device = _device(device)
    c = LH.case(name)
    if device == "cuda":
        from mdtf.ops import rnn
        assert rnn.units_per_block(*c.shape[:2], c.shape[3]) in (16, 32)
    LH.check("%s %s" % (name, device), _run(device, c), c, device == "cuda")


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("name", ["c", "d"])
def test_kernel_gradient_adds_into_a_filled_slot_and_repeats(name, device):
    device = _device(device)
    c = LH.case(name)
    slot0 = NH.randn(c.kernel.shape, 7)
    got = _run(device, c, slot0=slot0)
    LH.check("slot " + name, got, c, True, slot0=slot0)
    again = _run(device, c, slot0=slot0)
    for k in LH.NAMES:
        assert NH.bits_equal(got[k], again[k]), k


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("name,code", [("h48", 0), ("b", 1)], ids=["H48", "fp32"])
def test_entry_points_refuse(name, code, device):
    device = _device(device)
    from mdtf.ops import rnn  # noqa: F401  (registers the signatures)
    t, b, i, h = LH.CASES[name]
    buf = [torch.zeros(t * b * 4 * h + 4 * h * h, dtype=torch.float32, device=device) for _ in range(9)]
    p = [_native.ptr(z) for z in buf]
    assert _native.fn("mdtf_lstm_fwd")(*p[:8], t, b, h, 1.0, code, _native.stream_ptr()) == UNSUPPORTED
    assert _native.fn("mdtf_lstm_bwd")(*p, t, b, h, code, _native.stream_ptr()) == UNSUPPORTED


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name,fp32", [("h48", False), ("b", True)], ids=["H48", "fp32"])
def test_fallback_meets_the_oracle(name, fp32, device):
    device = _device(device)
    c = LH.case(name)
    LH.check("fallback %s %s" % (name, device), _run(device, c, fp32=fp32), c, device == "cuda" and not fp32)


@pytest.mark.parametrize("device", DEVICES)
def test_sequence_length_zeroes_outputs_and_freezes_state(device):
    device = _device(device)
    c = LH.case("b", lengths=(3, 1, 2, 3, 1))
    got = _run(device, c)
    out = got["outputs"].detach()
    assert float(out[1:, 1].abs().max()) == 0.0 and float(out[2, 2].abs().max()) == 0.0
    assert float(c.ref["outputs"][1:, 1].abs().max()) == 0.0
    assert NH.bits_equal(got["h_T"][1], got["outputs"][0, 1])
    LH.check("lengths " + device, got, c, device == "cuda")


def test_variable_names_time_major_and_options():
    V.reset_default_graph()
    x = NH.randn((3, 4, 6), 5)                                   # [B, T, I]
    cell = mdtf.nn.rnn_cell.BasicLSTMCell(8)
    with mdtf.variable_scope("model"):
        out, state = mdtf.nn.dynamic_rnn(cell, x, dtype=torch.float32, scope="enc")
    shapes = {v.name: tuple(v.shape) for v in V.get_store().trainable_variables()}
    assert shapes == {"model/enc/lstm_cell/kernel": (14, 32), "model/enc/lstm_cell/bias": (32,)}
    assert tuple(out.shape) == (3, 4, 8) and isinstance(state, State) and tuple(state.c.shape) == (3, 8)
    with mdtf.variable_scope("model", reuse=True):
        out_t, state_t = mdtf.nn.dynamic_rnn(cell, x.transpose(0, 1), time_major=True, scope="enc")
    assert torch.equal(out_t.transpose(0, 1), out) and torch.equal(state_t.h, state.h)
    assert torch.equal(state.h, out[:, -1]) and tuple(cell.zero_state(5, torch.float32).h.shape) == (5, 8)
    for opt in (dict(use_peepholes=True), dict(num_proj=4), dict(cell_clip=1.0)):
        with pytest.raises(NotImplementedError):
            mdtf.nn.rnn_cell.LSTMCell(8, **opt)
    with mdtf.variable_scope("model", reuse=True), pytest.raises(ValueError):
        mdtf.nn.dynamic_rnn(cell, NH.randn((3, 4, 7), 6), scope="enc")          # kernel rows do not match I + H
    with mdtf.variable_scope("other"), pytest.raises(ValueError):
        mdtf.nn.dynamic_rnn(cell, x, initial_state=State(torch.zeros(3, 8), torch.zeros(2, 8)))


def test_two_stacked_layers_train_one_step_on_cpu():
    from mdtf.layers import tools
    from mdtf.models import SoftmaxCrossEntropyLoss
    from mdtf.runtime import Model, Net, Tower
    from mdtf.train import step as S

    class M(Model):
        def inference(self, x):
            y, _ = tools.lstm("lstm1", x, 16)
            y, state = tools.lstm("lstm2", y, 8)
            return tools.dense("logits", state.h, 4)

    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device, store.compute_dtype = torch.device("cpu"), None
    xp, yp = mdtf.placeholder(torch.float32, [None, 5, 6]), mdtf.placeholder(torch.int64, [None])
    opt, tg = mdtf.train.GradientDescentOptimizer(0.1), []
    _, loss, _ = Tower(Net(M()), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), opt, batch_size=2).process()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    _, lv = sess.run([op, loss], feed_dict={xp: NH.randn((2, 5, 6), 9), yp: torch.tensor([1, 3])})
    assert torch.isfinite(torch.as_tensor(lv)).all()
    for name, shape in (("lstm1/lstm_cell/kernel", (22, 64)), ("lstm2/lstm_cell/kernel", (24, 32))):
        v = store.variable(name)
        assert v.shape == shape and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0.0
