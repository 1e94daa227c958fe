"""``mdtf.nn.dynamic_rnn`` over a ``GRUCell``, the kernels of ``csrc/gru.hip`` and the PyTorch loop against the fp64
oracle of ``gru_helpers``.  ``cpu`` runs the loop on fp32 tensors of bf16-representable values; ``cuda`` runs the HIP
kernels on bf16 tensors, the kernel and bias gradients landing in fp32 slots.  The limits are explained in
``gru_helpers``.
"""
import os
import sys

import pytest
import torch

import mdtf
from mdtf.ops import _native
from mdtf.train import variables as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_helpers as GH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
UNSUPPORTED = -2
VARS = ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")
SLOTS = ("dgates_kernel", "dgates_bias", "dcand_kernel", "dcand_bias")


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _run(device, c, slots0=None, fp32=False):
    """Forward + backward through ``mdtf.nn.dynamic_rnn`` on variables holding the case's weights; a dict over
    ``GH.NAMES``.  cuda: bf16 tensors (``fp32``: fp32 ones) and fp32 gradient slots, pre-filled with ``slots0``."""
    bf16 = device == "cuda" and not fp32
    put = (lambda t: NH.put(t, device)) if bf16 else (lambda t: t.clone().to(device))
    V.reset_default_graph()
    store = V.get_store()
    store.device, store.compute_dtype = torch.device(device), torch.bfloat16 if bf16 else None
    values = dict(zip(VARS, (c.gk, c.gb, c.ck, c.cb)))
    for name, value in values.items():
        scope, leaf = name.split("/")
        with mdtf.variable_scope("rnn/gru_cell/" + scope):
            mdtf.get_variable(leaf, value.shape, initializer=lambda *a, value=value, **k: value.clone())
    variables = [store.variable("rnn/gru_cell/" + name) for name in VARS]
    if device == "cuda":
        for v, key in zip(variables, SLOTS):
            v.grad = (slots0[key] if slots0 else torch.zeros(v.shape)).to(device).contiguous()
    x, h0 = put(c.x).requires_grad_(True), put(c.h0).requires_grad_(True)
    with mdtf.variable_scope("", reuse=True):
        out, state = mdtf.nn.dynamic_rnn(mdtf.nn.rnn_cell.GRUCell(c.shape[3]), x, sequence_length=c.lengths,
                                         initial_state=h0, time_major=True)
    assert out.dtype == x.dtype and state.dtype == x.dtype and tuple(state.shape) == (c.shape[1], c.shape[3])
    if c.lengths is None:
        assert NH.bits_equal(state, out[-1])
    torch.autograd.backward([out, state], [c.dhs.to(device).to(out.dtype), c.dh_t.to(device).to(out.dtype)])
    assert all(v.grad.dtype == torch.float32 for v in variables) and h0.grad.dtype == h0.dtype
    return dict(zip(GH.NAMES, (out, state, x.grad) + tuple(v.grad for v in variables) + (h0.grad,)))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", list(GH.SHORT) + ["carry"])
def test_geometry_case(name, device):
    device = _device(device)
    c = GH.case(name)
    GH.check("%s %s" % (name, device), _run(device, c), c, device == "cuda")


@pytest.mark.parametrize("device", GPU_ONLY)
def test_both_block_widths_occur(device):
    _device(device)
    from mdtf.ops import gru
    units = [gru.units_per_block(*GH.CASES[n][:2], GH.CASES[n][3]) for n in GH.SHORT]
    assert {u for pair in units for u in pair} == {16, 32}, units


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("name", ["c", "d"])
def test_gradients_add_into_filled_slots_and_repeat(name, device):
    device = _device(device)
    c = GH.case(name)
    slots0 = {k: NH.randn(c.ref[k].shape, 7 + i) for i, k in enumerate(SLOTS)}
    got = _run(device, c, slots0=slots0)
    GH.check("slot " + name, got, c, True, slots0=slots0)
    again = _run(device, c, slots0=slots0)
    for k in GH.NAMES:
        assert NH.bits_equal(got[k], again[k]), k


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("name,code", [("h48", 0), ("b", 1)], ids=["H48", "fp32"])
def test_entry_points_refuse(name, code, device):
    device = _device(device)
    from mdtf.ops import gru  # noqa: F401  (registers the signatures)
    t, b, i, h = GH.CASES[name]
    buf = [torch.zeros(t * b * 3 * h + 3 * h * h, dtype=torch.float32, device=device) for _ in range(10)]
    p = [_native.ptr(z) for z in buf]
    assert _native.fn("mdtf_gru_units")(t, b, h, code) == 0
    assert _native.fn("mdtf_gru_fwd")(*p, t, b, h, code, _native.stream_ptr()) == UNSUPPORTED
    assert _native.fn("mdtf_gru_bwd")(*p[:8], t, b, h, code, _native.stream_ptr()) == UNSUPPORTED


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name,fp32", [("h48", False), ("b", True)], ids=["H48", "fp32"])
def test_fallback_meets_the_oracle(name, fp32, device):
    device = _device(device)
    c = GH.case(name)
    GH.check("fallback %s %s" % (name, device), _run(device, c, fp32=fp32), c, device == "cuda" and not fp32)


@pytest.mark.parametrize("device", DEVICES)
def test_sequence_length_zeroes_outputs_and_freezes_state(device):
    device = _device(device)
    c = GH.case("b", lengths=(3, 1, 2, 3, 1))
    got = _run(device, c)
    out = got["outputs"].detach()
    assert float(out[1:, 1].abs().max()) == 0.0 and float(out[2, 2].abs().max()) == 0.0
    assert float(c.ref["outputs"][1:, 1].abs().max()) == 0.0
    assert NH.bits_equal(got["h_T"][1], got["outputs"][0, 1]) and NH.bits_equal(got["h_T"][2], got["outputs"][1, 2])
    GH.check("lengths " + device, got, c, device == "cuda")


def test_variable_names_time_major_and_options():
    V.reset_default_graph()
    x = NH.randn((3, 4, 6), 5)                                   # [B, T, I]
    cell = mdtf.nn.rnn_cell.GRUCell(8)
    with mdtf.variable_scope("model"):
        out, state = mdtf.nn.dynamic_rnn(cell, x, dtype=torch.float32, scope="enc")
    store = V.get_store()
    shapes = {v.name: tuple(v.shape) for v in store.trainable_variables()}
    assert shapes == {"model/enc/gru_cell/gates/kernel": (14, 16), "model/enc/gru_cell/gates/bias": (16,),
                      "model/enc/gru_cell/candidate/kernel": (14, 8), "model/enc/gru_cell/candidate/bias": (8,)}
    assert bool((store.variable("model/enc/gru_cell/gates/bias").master == 1.0).all())
    assert bool((store.variable("model/enc/gru_cell/candidate/bias").master == 0.0).all())
    assert tuple(out.shape) == (3, 4, 8) and torch.is_tensor(state) and tuple(state.shape) == (3, 8)
    assert cell.state_size == 8 and cell.output_size == 8 and tuple(cell.zero_state(5, torch.float32).shape) == (5, 8)
    with mdtf.variable_scope("model", reuse=True):
        out_t, state_t = mdtf.nn.dynamic_rnn(cell, x.transpose(0, 1), time_major=True, scope="enc")
    assert torch.equal(out_t.transpose(0, 1), out) and torch.equal(state_t, state) and torch.equal(state, out[:, -1])
    with pytest.raises(NotImplementedError):
        mdtf.nn.rnn_cell.GRUCell(8, activation=torch.relu)
    with mdtf.variable_scope("bi"), pytest.raises(TypeError):
        mdtf.nn.bidirectional_dynamic_rnn(cell, mdtf.nn.rnn_cell.GRUCell(8), x, dtype=torch.float32)


def test_two_stacked_layers_train_one_step_on_cpu():
    from mdtf.layers import tools
    from mdtf.models import SoftmaxCrossEntropyLoss
    from mdtf.runtime import Model, Net, Tower
    from mdtf.train import step as S

    class M(Model):
        def inference(self, x):
            y, _ = tools.gru("gru1", x, 16)
            y, state = tools.gru("gru2", y, 8)
            return tools.dense("logits", state, 4)

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
    for name, shape in (("gru1/gru_cell/gates/kernel", (22, 32)), ("gru2/gru_cell/candidate/kernel", (24, 8))):
        v = store.variable(name)
        assert v.shape == shape and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0.0


@pytest.mark.parametrize("device", GPU_ONLY)
def test_entry_points_replay_in_a_graph(device):
    device = _device(device)
    from mdtf.ops import gru
    c = GH.case("d")
    t, b, i, h = c.shape
    bf = lambda z: z.to(device).bfloat16().contiguous()
    new = lambda *shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype, device=device)
    xg = bf(NH.randn((t, b, 3 * h), 3))
    wg, wc, h0b, h0f, dhs = bf(c.gk[i:]), bf(c.ck[i:]), bf(c.h0), c.h0.to(device), bf(c.dhs)
    dh_t = c.dh_t.to(device)

    def buffers():
        return dict(wt=new(3 * h * h), hs=new(t, b, h), hf=new(t, b, h, dtype=torch.float32), rh=new(t, b, h),
                    gates=new(t, b, 3 * h), carry=new(b, h, dtype=torch.float32), dg=new(t, b, 3 * h))

    def call(z):
        P, st = _native.ptr, _native.stream_ptr()
        z["carry"].copy_(dh_t)
        _native.check(_native.fn("mdtf_gru_fwd")(P(xg), P(wg), P(wc), P(z["wt"]), P(h0b), P(h0f), P(z["hs"]), P(z["hf"]),
                                                 P(z["rh"]), P(z["gates"]), t, b, h, gru.BF16, st), "gru_fwd")
        _native.check(_native.fn("mdtf_gru_bwd")(P(wg), P(wc), P(z["gates"]), P(z["hf"]), P(h0f), P(dhs), P(z["carry"]),
                                                 P(z["dg"]), t, b, h, gru.BF16, st), "gru_bwd")

    eager, graphed = buffers(), buffers()
    call(eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(graphed)                                            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(graphed)
    for _ in range(2):
        for k in ("hs", "hf", "rh", "gates", "dg", "carry"):
            graphed[k].fill_(1.0)
        g.replay()
        torch.cuda.synchronize()
        for k in ("hs", "hf", "rh", "gates", "dg", "carry"):
            assert NH.bits_equal(graphed[k], eager[k]), k
