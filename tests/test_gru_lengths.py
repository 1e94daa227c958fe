"""Per-row lengths, the reverse direction and a forward plus a reverse GRU: the kernels of ``csrc/gru.hip`` (``cuda``,
bf16, gradients landing in fp32 slots) and the PyTorch loop (``cpu``) against the fp64 oracle of ``gru_seq_helpers``.
``fw`` runs ``mdtf.nn.dynamic_rnn``, ``bw`` ``ops.gru.gru(reverse=True)``, ``both`` ``ops.gru.bigru``.
"""
import os
import sys

import pytest
import torch

import mdtf
from mdtf.layers import tools
from mdtf.ops import _native, gru, rnn
from mdtf.train import variables as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_helpers as GH  # noqa: E402
import gru_seq_helpers as GS  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
LEAVES = ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _run(device, jobs, lengths="case"):
    """Forward + backward of the job(s) of a ``GS.plan`` (two: the pair): a dict over ``GH.NAMES`` per direction."""
    mode = "both" if len(jobs) == 2 else jobs[0][1]
    lengths = jobs[0][0].lengths if isinstance(lengths, str) else lengths
    put = (lambda t: NH.put(t, device)) if device == "cuda" else (lambda t: t.clone())
    V.reset_default_graph()
    store = V.get_store()
    store.device, store.compute_dtype = torch.device(device), torch.bfloat16 if device == "cuda" else None
    scopes = ["bi/%s/gru_cell/" % d for _, d, _ in jobs] if mode == "both" else ["rnn/gru_cell/"]
    vs, params = [], []
    for (c, _, _), scope in zip(jobs, scopes):
        for leaf, value in zip(LEAVES, (c.gk, c.gb, c.ck, c.cb)):
            with mdtf.variable_scope(scope + leaf.split("/")[0]):
                mdtf.get_variable(leaf.split("/")[1], value.shape, initializer=lambda *a, value=value, **k: value.clone())
        vs.append([store.variable(scope + leaf) for leaf in LEAVES])
        if device == "cuda":
            for v in vs[-1]:
                v.grad = torch.zeros(v.shape, device=device)
    x = put(jobs[0][0].x).requires_grad_(True)
    h0s = [put(c.h0).requires_grad_(True) for c, _, _ in jobs]
    cell = mdtf.nn.rnn_cell.GRUCell(jobs[0][0].shape[3])
    with mdtf.variable_scope("", reuse=True):
        for scope in scopes:
            with mdtf.variable_scope(scope[:-len("/gru_cell/")]):
                params.append(cell.variables(x.shape[2]))
        if mode == "fw":
            res = [mdtf.nn.dynamic_rnn(cell, x, sequence_length=lengths, initial_state=h0s[0], time_major=True)]
        elif mode == "bw":
            res = [gru.gru(x, *params[0], h0s[0], lengths, reverse=True)]
        else:
            res = gru.bigru(x, params[0] + (h0s[0],), params[1] + (h0s[1],), lengths)
    ys = [y for pair in res for y in pair]
    gs = [g for c, _, _ in jobs for g in (c.dhs, c.dh_t)]
    torch.autograd.backward(ys, [g.to(device).to(y.dtype) for g, y in zip(gs, ys)])
    return [dict(zip(GH.NAMES, (out, h_t, x.grad) + tuple(v.grad for v in v4) + (h0.grad,)))
            for (out, h_t), v4, h0 in zip(res, vs, h0s)]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode", GS.MODES)
@pytest.mark.parametrize("name", list(GS.CASES))
def test_lengths_and_directions(name, mode, device):
    device = _device(device)
    c = GS.case(name)
    if device == "cuda":
        assert gru.native_ok(NH.put(c.x, device), NH.put(c.ck, device), NH.put(c.h0, device), c.lengths)
        assert name != "u32" or gru.units_per_block(c.shape[0], c.shape[1], c.shape[3]) == (16, 32)
    jobs = GS.plan(name, mode)
    for got, (c, direction, ref) in zip(_run(device, jobs), jobs):
        GS.check("%s %s %s %s" % (name, mode, direction, device), got, ref, c, direction, device == "cuda")


def test_layer_functions_name_their_variables_as_tf_does():
    V.reset_default_graph()
    x = NH.randn((3, 4, 6), 5)                                   # [B, T, I]
    out, (h_fw, h_bw) = tools.bigru("enc", x, 8, sequence_length=(4, 2, 0))
    names = {v.name for v in V.get_store().trainable_variables()}
    assert names == {"enc/%s/gru_cell/%s" % (d, leaf) for d in ("fw", "bw") for leaf in LEAVES}
    assert tuple(out.shape) == (3, 4, 16) and tuple(h_fw.shape) == tuple(h_bw.shape) == (3, 8)
    with mdtf.variable_scope("", reuse=True):
        fw, _ = tools.gru("enc/fw", x, 8, sequence_length=(4, 2, 0))
        bw, s_bw = tools.gru("enc/bw", x, 8, sequence_length=(4, 2, 0), reverse=True)
    assert torch.equal(out, torch.cat([fw, bw], -1)) and torch.equal(s_bw, h_bw)
    assert torch.equal(h_bw[1], out[1, 0, 8:]) and float(out[1, 2:].detach().abs().max()) == 0.0 and not bool(h_bw[2].any())


@pytest.mark.parametrize("device", GPU_ONLY)
def test_full_lengths_and_the_pair_match_the_single_calls_bit_for_bit(device):
    device = _device(device)
    t, b = GS.case("tile").shape[:2]
    fw, jobs = GS.plan("tile", "fw"), GS.plan("tile", "both")
    plain, = _run(device, fw, lengths=None)
    full, = _run(device, fw, lengths=(t,) * b)
    for k in GH.NAMES:
        assert NH.bits_equal(plain[k], full[k]), k
    pair, again = _run(device, jobs), _run(device, jobs)
    alone = _run(device, jobs[:1]) + _run(device, jobs[1:])
    for d in range(2):
        for k in GH.NAMES:
            assert NH.bits_equal(pair[d][k], again[d][k]), k
            # dx: the pair rounds the sum of both products once, the single calls round each
            assert k == "dx" or NH.bits_equal(pair[d][k], alone[d][k]), (d, k)


@pytest.mark.parametrize("device", GPU_ONLY)
def test_entry_points_zero_dead_rows_and_replay_with_new_lengths(device):
    device = _device(device)
    c, o = GS.case("tile"), GS.other("tile")
    (t, b, i, h), P = c.shape, _native.ptr
    nan = lambda *shape, dtype=torch.bfloat16: torch.full(shape, float("nan"), dtype=dtype, device=device)
    xg = NH.put(NH.randn((t, b, 6 * h), 3), device)
    w = [tuple(NH.put(v, device) for v in (z.gk[i:], z.ck[i:], z.h0)) + (z.h0.to(device), NH.put(z.dhs, device),
                                                                          z.dh_t.to(device)) for z in (c, o)]
    lens = torch.tensor(c.lengths, dtype=torch.int32, device=device)
    work = ("hs", "hf", "rh", "gates", "dg")

    def buffers():
        return [dict(wt=nan(3 * h * h), hs=nan(t, b, h), hf=nan(t, b, h, dtype=torch.float32), rh=nan(t, b, h),
                     gates=nan(t, b, 3 * h), h_fin=nan(b, h), carry=nan(b, h, dtype=torch.float32), dg=nan(t, b, 3 * h))
                for _ in range(2)]

    def call(zs):
        fwd, bwd = [], []
        for d, (z, (wg, wc, h0b, h0f, dhs, dh_t)) in enumerate(zip(zs, w)):
            z["carry"].copy_(dh_t)
            fwd.append((xg[:, :, 3 * h * d:], wg, wc, z["wt"], h0b, h0f, z["hs"], z["hf"], z["rh"], z["gates"], z["h_fin"]))
            bwd.append((wg, wc, z["gates"], z["hf"], h0f, dhs, z["carry"], z["dg"]))
        st = _native.stream_ptr()
        _native.check(_native.fn("mdtf_gru_fwd_seq")(rnn._table(fwd), 2, 0b10, P(lens), t, b, h, 6 * h, gru.BF16, st),
                      "gru_fwd_seq")
        _native.check(_native.fn("mdtf_gru_bwd_seq")(rnn._table(bwd), 2, 0b10, P(lens), t, b, h, gru.BF16, st),
                      "gru_bwd_seq")

    eager, graphed = buffers(), buffers()
    call(eager)
    torch.cuda.synchronize()
    dead = (torch.arange(t)[:, None] >= torch.tensor(c.lengths)[None]).to(device)
    for z in eager:
        assert all(bool(torch.isfinite(v).all()) for v in z.values())   # so 0 * NaN cannot reach a weight gradient
        assert all(float(z[k][dead].abs().max()) == 0.0 for k in work)
    lens.fill_(2)                                                # captured with other lengths in the same buffer
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(graphed)                                            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(graphed)
    lens.copy_(torch.tensor(c.lengths, dtype=torch.int32))
    for _ in range(2):
        for z in graphed:
            for k in work + ("h_fin",):
                z[k].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for z, e in zip(graphed, eager):
            for k in work + ("h_fin", "carry"):
                assert NH.bits_equal(z[k], e[k]), k
