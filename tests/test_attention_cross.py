"""Encoder-decoder attention with per-item source lengths: ``cross_attention`` / ``tools.attention_layer`` and the
kernels of ``csrc/attention_cross.hip`` against an fp64 reference (-inf on the columns >= length, the kernels' dropout
bits, autograd gradients) at the smallest shapes at which each branch of the tiling can go wrong.

``cpu`` runs the PyTorch expression on fp32 tensors holding bf16-representable values; ``cuda`` runs the HIP kernels.
Bounds: the aggregate relative errors of ``test_kernels_gpu.py::test_fused_attention_fwd_bwd``.
"""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from mdtf.ops import _native
from mdtf.ops import transformer as T

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]

#        B  Sq   Sk   nh dh   lengths        random 15 % mask
CASES = [(2, 64, 128, 2, 64, (128, 70), False),        # Sq < Sk; the crossing tile is not aligned
         (2, 192, 64, 3, 64, (64, 1), False),          # Sq > Sk; three query blocks; a single visible key
         (3, 128, 320, 2, 128, (320, 129, 0), False),  # head dim 128; skipped tiles; one key into a tile; an empty item
         (2, 128, 192, 2, 64, None, True),             # no lengths; the mask alone
         (2, 192, 128, 2, 128, (128, 70), False)]      # head dim 128 runs 128-query blocks: the last one is half full
RAGGED = CASES[:3]
FALLBACK = (2, 64, 96, 2, 64, (96, 50), False)         # Sk is no multiple of 64
# the CPU parametrisation runs the PyTorch path without dropout only
VALUE_CASES = [pytest.param("cpu", c, 0.0) for c in CASES] + \
              [pytest.param("cuda", c, p, marks=pytest.mark.gpu) for c in CASES for p in (0.0, 0.1)]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _keep_mask(seed, B, nh, Sq, Sk, p):
    """The kernels' dropout keep bits: the counter hash of element (bh * Sq + q) * Sk + k and the seed."""
    idx = np.arange(B * nh * Sq * Sk, dtype=np.uint64).astype(np.uint32)
    x = (idx * np.uint32(0x9E3779B1)) ^ np.uint32(seed)
    x ^= x >> np.uint32(16)
    x = x * np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x = x * np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    thr = np.uint32(min(int(p * 4294967296.0), 4294967295))
    return torch.from_numpy((x >= thr).reshape(B, nh, Sq, Sk))


def _reference(q, kv, mask, lengths, dout, B, Sq, Sk, nh, dh, keep=None, p_drop=0.0):
    """fp64 attention of bf16-rounded ``q`` over ``kv`` with -inf on the columns >= length: (out, dq, dkv).  An item
    of length 0 has no softmax: its probabilities are zero."""
    x, y = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = x.reshape(B, Sq, nh, dh).transpose(1, 2)
    k, v = (t.transpose(1, 2) for t in y.reshape(B, Sk, 2, nh, dh).unbind(2))
    s = qh @ k.transpose(-1, -2) / dh ** 0.5
    if mask is not None:
        s = s + mask.double()[:, None, None, :]
    n = torch.tensor(lengths if lengths is not None else [Sk] * B)
    hidden = (torch.arange(Sk)[None, :] >= n[:, None]) & (n > 0)[:, None]
    pr = torch.softmax(s.masked_fill(hidden[:, None, None, :], float("-inf")), -1)
    pr = pr * (n > 0).double()[:, None, None, None]
    if keep is not None:
        pr = pr * keep / (1 - p_drop)
    out = (pr @ v).transpose(1, 2).reshape(B * Sq, nh * dh)
    out.backward(dout.double())
    return out.detach(), x.grad, y.grad


@functools.lru_cache(maxsize=None)
def _inputs(B, Sq, Sk, nh, dh, with_mask):
    """bf16-representable fp32 q, kv, dout and the key mask (or None); computed once and left unchanged."""
    g = torch.Generator().manual_seed(33 + Sq + 2 * Sk + dh)
    H = nh * dh
    q = (torch.randn(B * Sq, H, generator=g) * 0.5).bfloat16().float()
    kv = (torch.randn(B * Sk, 2 * H, generator=g) * 0.5).bfloat16().float()
    dout = torch.randn(B * Sq, H, generator=g).bfloat16().float()
    mask = (torch.rand(B, Sk, generator=g) < 0.15).float() * -10000.0 if with_mask else None
    return q, kv, dout, mask


def _run(device, case, p_drop=0.0, kv=None, seed=1234567):
    """``cross_attention`` forward and backward on ``device`` (bf16 on the GPU): (out, dq, dkv)."""
    B, Sq, Sk, nh, dh, case_lengths, with_mask = case
    q, kv0, dout, mask = _inputs(B, Sq, Sk, nh, dh, with_mask)
    dt = torch.bfloat16 if device == "cuda" else torch.float32
    x = q.clone().to(device, dt).requires_grad_(True)
    y = (kv0 if kv is None else kv).clone().to(device, dt).requires_grad_(True)
    lengths = list(case_lengths) if case_lengths is not None else None
    # cross_attention draws its dropout seed with torch.randint: hand it a known one
    with mock.patch.object(torch, "randint", lambda *a, **k: torch.tensor([seed])):
        out = T.cross_attention(x, y, B, Sq, Sk, nh, mask.to(device) if with_mask else None, lengths, p_drop)
    out.backward(dout.to(device, dt))
    return out.detach(), x.grad, y.grad


def _check(case, got, p_drop=0.0, seed=1234567, device="cpu"):
    B, Sq, Sk, nh, dh, lengths, with_mask = case
    H = nh * dh
    q, kv, dout, mask = _inputs(B, Sq, Sk, nh, dh, with_mask)
    keep = _keep_mask(T.effective_seed(seed, torch.device(device)), B, nh, Sq, Sk, p_drop) if p_drop else None
    ref, dq, dkv = _reference(q, kv, mask, lengths, dout, B, Sq, Sk, nh, dh, keep, p_drop)
    errs = [_rel(got[0], ref), _rel(got[1], dq), _rel(got[2][:, :H], dkv[:, :H]), _rel(got[2][:, H:], dkv[:, H:])]
    print("rel err out, dq, dk, dv:", errs)
    assert errs[0] < 1.5e-2 and max(errs[1:]) < 3e-2, errs
    for b in [i for i, n in enumerate(lengths or ()) if n == 0]:       # the empty item: exact zeros
        assert all(bool((t.view(B, -1, t.shape[-1])[b] == 0).all()) for t in got)


@pytest.mark.parametrize("device,case,p_drop", VALUE_CASES)
def test_values(device, case, p_drop):
    """out, dq, dk, dv against fp64 with the same dropout bits; the empty item's rows exactly zero."""
    device = _device(device)
    _check(case, _run(device, case, p_drop), p_drop, device=device)


@pytest.mark.parametrize("case", RAGGED)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_hidden_keys_are_invisible(device, case):
    """Other finite K / V rows at k >= len leave out and dq bitwise unchanged; their dK / dV rows are exactly zero."""
    _device(device)
    B, Sq, Sk, nh, dh, lengths, with_mask = case
    kv = _inputs(B, Sq, Sk, nh, dh, with_mask)[1]
    other = kv.clone().view(B, Sk, -1)
    noise = torch.randn(other.shape, generator=torch.Generator().manual_seed(1)).bfloat16().float() * 3
    for b, n in enumerate(lengths):
        other[b, n:] = noise[b, n:]
    a = _run(device, case, 0.1)
    c = _run(device, case, 0.1, kv=other.view(B * Sk, -1))
    assert torch.equal(a[0].view(torch.int16), c[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int16), c[1].view(torch.int16))
    for dkv in (a[2].view(B, Sk, -1), c[2].view(B, Sk, -1)):
        for b, n in enumerate(lengths):
            assert bool((dkv[b, n:] == 0).all())
            assert n == 0 or bool((dkv[b, :n] != 0).any())


@pytest.mark.parametrize("device", GPU_ONLY)
def test_lengths_are_read_on_the_device(device):
    """Forward and backward with dropout captured once: replays are bitwise the eager result for the same step
    counter, and after ``kv_lengths.copy_(other)`` the eager result for ``other`` (no host read, no allocation)."""
    _device(device)
    case = B, Sq, Sk, nh, dh, first, _ = CASES[2]
    second = (65, 0, 320)
    q, kv, dout, _ = _inputs(B, Sq, Sk, nh, dh, False)
    x = q.cuda().bfloat16().requires_grad_(True)
    y = kv.cuda().bfloat16().requires_grad_(True)
    d = dout.cuda().bfloat16()
    lens = torch.tensor(first, dtype=torch.int32, device="cuda")
    other = torch.tensor(second, dtype=torch.int32, device="cuda")

    def step():
        x.grad = y.grad = None
        with mock.patch.object(torch, "randint", lambda *a, **k: torch.tensor([1234567])):
            out = T.cross_attention(x, y, B, Sq, Sk, nh, None, lens, 0.1)
        out.backward(d)
        return out.detach(), x.grad, y.grad

    eager = {}
    for name, n in (("second", other), ("first", torch.tensor(first, dtype=torch.int32, device="cuda"))):
        lens.copy_(n)
        eager[name] = [t.clone() for t in step()]
    assert not torch.equal(eager["first"][0], eager["second"][0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = step()
    for name in ("first", "first", "second"):
        if name == "second":
            lens.copy_(other)
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(e, t) for e, t in zip(eager[name], out)), name
    del graph


@pytest.mark.parametrize("device", DEVICES)
def test_unsupported_length_takes_the_pytorch_path(device):
    """Sk = 96 is no multiple of 64: the PyTorch expression runs, lengths included."""
    device = _device(device)
    _check(FALLBACK, _run(device, FALLBACK), device=device)


def test_shape_errors():
    q, kv = torch.zeros(128, 128), torch.zeros(256, 256)
    for args in ((q, kv, 2, 64, 64, 2), (q, kv, 2, 64, 128, 3), (q, kv[:, :128], 2, 64, 128, 2)):
        with pytest.raises(ValueError):
            T.cross_attention(*args)
    with pytest.raises(ValueError):
        T.cross_attention(q, kv, 2, 64, 128, 2, kv_lengths=[128, 70, 3])


def test_attention_layer_on_cpu():
    """``tools.attention_layer``: BERT's variable names, created value, key, query; the self case is
    ``fused_attention`` on the same weights; the cross case with ``to_lengths`` matches fp64; causal cross raises."""
    from mdtf.layers import tools
    from mdtf.ops import nn as ops
    from mdtf.train import step as St
    from mdtf.train import variables as V
    V.reset_default_graph()
    St.reset()
    store = V.get_store()
    store.device = torch.device("cpu")
    store.generator.manual_seed(7)
    B, Sq, Sk, nh, dh, lengths, _ = case = CASES[0]
    H = nh * dh
    q, kv, _, _ = _inputs(B, Sq, Sk, nh, dh, False)
    frm, to = q.view(B, Sq, H), kv.view(B, Sk, 2 * H)           # the "to" sequence is 2H wide
    out = tools.attention_layer("att", frm, to, nh, dh, to_lengths=lengths)
    names = ["att/%s/%s" % (n, p) for n in ("value", "key", "query") for p in ("kernel", "bias")]
    assert list(store.vars) == names
    assert [store.vars[n].shape for n in names] == [(2 * H, H), (H,), (2 * H, H), (H,), (H, H), (H,)]
    for n in names[1::2]:
        store.vars[n].assign(torch.randn(H, generator=store.generator).bfloat16().float() * 0.1)
    w = {n: store.vars[n].master.detach() for n in names}
    with V.variable_scope(V.get_variable_scope(), reuse=True), torch.no_grad():
        out = tools.attention_layer("att", frm, to, nh, dh, to_lengths=lengths)
        with pytest.raises(ValueError):
            tools.attention_layer("att", frm, to, nh, dh, causal=True)
    assert out.shape == (B, Sq, H)
    qp = frm.reshape(B * Sq, H).double() @ w["att/query/kernel"].double() + w["att/query/bias"].double()
    kvp = torch.cat([to.reshape(B * Sk, 2 * H).double() @ w["att/%s/kernel" % n].double() + w["att/%s/bias" % n].double()
                     for n in ("key", "value")], 1)
    ref = _reference(qp, kvp, None, lengths, torch.zeros(B * Sq, H), B, Sq, Sk, nh, dh)[0]
    assert _rel(out.reshape(B * Sq, H), ref) < 1.5e-2
    with torch.no_grad():
        got = tools.attention_layer("self", frm, frm, nh, dh, causal=True)
        ws, bs = zip(*[(store.vars["self/%s/kernel" % n].master, store.vars["self/%s/bias" % n].master)
                       for n in ("query", "key", "value")])
        qkv = ops.dense_multi(frm.reshape(B * Sq, H), list(ws), list(bs))
        assert torch.equal(got.reshape(B * Sq, H), T.fused_attention(qkv, B, Sq, nh, None, 0.0, causal=True))
    V.reset_default_graph()
