"""Causal self-attention: ``fused_attention(..., causal=True)`` / ``attention(..., causal=True)`` and the kernels of
``csrc/attention_causal.hip`` against an fp64 reference (key mask plus a -inf upper triangle, the kernels' dropout
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

#          B  S    nh dh
SHAPES = [(2, 64, 2, 64),      # one tile, diagonal only
          (2, 128, 2, 64),     # one query block, waves 0-1 skip the second key tile; leaves the S = 128 kernel
          (2, 192, 3, 64),     # ends on a half query block; three blocks in the heaviest-first mapping
          (1, 320, 2, 128)]    # head dim 128; unmasked, diagonal and skipped tiles in one block
EXACT_SHAPES = SHAPES[2:]
T_CUT = 75                     # not tile-aligned
# the CPU parametrisation runs the PyTorch path without dropout only
VALUE_CASES = [pytest.param("cpu", s, 0.0) for s in SHAPES] + \
              [pytest.param("cuda", s, p, marks=pytest.mark.gpu) for s in SHAPES for p in (0.0, 0.1)]


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


def _keep_mask(seed, B, nh, S, p):
    """The kernels' dropout keep bits: the counter hash of element (bh, q, k) and the seed."""
    idx = np.arange(B * nh * S * S, dtype=np.uint64).astype(np.uint32)
    x = (idx * np.uint32(0x9E3779B1)) ^ np.uint32(seed)
    x ^= x >> np.uint32(16)
    x = x * np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x = x * np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    thr = np.uint32(min(int(p * 4294967296.0), 4294967295))
    return torch.from_numpy((x >= thr).reshape(B, nh, S, S))


def _reference(qkv, mask, dout, B, S, nh, dh, keep=None, p_drop=0.0):
    """fp64 causal attention of bf16-rounded ``qkv``: (out [B*S, H], dqkv [B*S, 3H], lse [B, nh, S])."""
    x = qkv.double().detach().requires_grad_(True)
    q, k, v = (t.transpose(1, 2) for t in x.reshape(B, S, 3, nh, dh).unbind(2))
    tri = torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    s = q @ k.transpose(-1, -2) / dh ** 0.5 + mask.double()[:, None, None, :] + tri
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep / (1 - p_drop)
    out = (pr @ v).transpose(1, 2).reshape(B * S, nh * dh)
    out.backward(dout.double())
    return out.detach(), x.grad, torch.logsumexp(s, -1).detach()


@functools.lru_cache(maxsize=None)
def _inputs(B, S, nh, dh):
    """bf16-representable fp32 qkv, a random 15 % key mask and dout; computed once and left unchanged."""
    g = torch.Generator().manual_seed(21 + S + dh)
    H = nh * dh
    qkv = (torch.randn(B * S, 3 * H, generator=g) * 0.5).bfloat16().float()
    mask = (torch.rand(B, S, generator=g) < 0.15).float() * -10000.0
    dout = torch.randn(B * S, H, generator=g).bfloat16().float()
    return qkv, mask, dout


def _run(device, qkv, mask, dout, B, S, nh, p_drop=0.0, causal=True, seed=1234567):
    """``fused_attention`` forward and backward on ``device`` (bf16 on the GPU); (out, dqkv, kernel seed)."""
    dt = torch.bfloat16 if device == "cuda" else torch.float32
    x = qkv.clone().to(device, dt).requires_grad_(True)
    # fused_attention draws its dropout seed with torch.randint: hand it a known one (any other draw would show as a
    # mismatch with the reference's keep bits)
    with mock.patch.object(torch, "randint", lambda *a, **k: torch.tensor([seed])):
        out = T.fused_attention(x, B, S, nh, mask.to(device), p_drop, causal=causal)
    out.backward(dout.to(device, dt))
    return out.detach(), x.grad, seed


def _check(out, grad, ref, gref, H):
    assert _rel(out, ref) < 1.5e-2
    for part in range(3):      # dq, dk, dv
        sl = slice(part * H, (part + 1) * H)
        assert _rel(grad[:, sl], gref[:, sl]) < 3e-2, part


@pytest.mark.parametrize("device,shape,p_drop", VALUE_CASES)
def test_values(device, shape, p_drop):
    """out, dq, dk, dv against fp64 with the same dropout bits."""
    device = _device(device)
    B, S, nh, dh = shape
    qkv, mask, dout = _inputs(*shape)
    out, grad, seed = _run(device, qkv, mask, dout, B, S, nh, p_drop)
    keep = _keep_mask(T.effective_seed(seed, torch.device(device)), B, nh, S, p_drop) if p_drop else None
    ref, gref, _ = _reference(qkv, mask, dout, B, S, nh, dh, keep, p_drop)
    _check(out, grad, ref, gref, nh * dh)


@pytest.mark.parametrize("shape", EXACT_SHAPES)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_future_keys_do_not_reach_the_past(device, shape):
    """New K and V rows at positions >= t leave the output rows of queries < t bitwise unchanged."""
    _device(device)
    B, S, nh, dh = shape
    H = nh * dh
    qkv, mask, dout = _inputs(*shape)
    other = qkv.clone().view(B, S, 3 * H)
    other[:, T_CUT:, H:] = torch.randn(B, S - T_CUT, 2 * H, generator=torch.Generator().manual_seed(1)).bfloat16()
    a = _run(device, qkv, mask, dout, B, S, nh, 0.1)[0].view(B, S, H)
    b = _run(device, other.view(B * S, 3 * H), mask, dout, B, S, nh, 0.1)[0].view(B, S, H)
    assert torch.equal(a[:, :T_CUT].view(torch.int16), b[:, :T_CUT].view(torch.int16))
    assert not torch.equal(a[:, T_CUT:], b[:, T_CUT:])


@pytest.mark.parametrize("shape", EXACT_SHAPES)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_past_dout_gives_no_future_gradient(device, shape):
    """With dout zero for queries >= t, rows >= t of dq, dk and dv are exactly zero."""
    _device(device)
    B, S, nh, dh = shape
    qkv, mask, dout = _inputs(*shape)
    dout = dout.clone().view(B, S, -1)
    dout[:, T_CUT:] = 0
    grad = _run(device, qkv, mask, dout.view(B * S, -1), B, S, nh, 0.1)[1].view(B, S, -1)
    assert bool((grad[:, T_CUT:] == 0).all())
    assert bool((grad[:, :T_CUT] != 0).any())


@pytest.mark.parametrize("shape", EXACT_SHAPES)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_lse_of_first_query_is_its_own_score(device, shape):
    """lse runs over the visible keys: query 0 sees key 0 alone, so lse[0] = scale * q0.k0 + mask[0]."""
    _device(device)
    B, S, nh, dh = shape
    qkv, mask, _ = _inputs(*shape)
    out = T.fused_attention(qkv.cuda().bfloat16().requires_grad_(True), B, S, nh, mask.cuda(), causal=True)
    lse = out.grad_fn.saved_tensors[2].view(B, nh, S)[:, :, 0].cpu()
    q, k, _ = qkv.view(B, S, 3, nh, dh)[:, 0].unbind(1)
    want = (q * k).sum(-1) / dh ** 0.5 + mask[:, :1]
    assert ((lse - want).abs() <= 1e-3 * want.abs()).all()


@pytest.mark.parametrize("shape", [(2, 128, 2, 64), (2, 192, 3, 64)])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_non_causal_route_is_untouched(device, shape):
    """``causal=False`` is bitwise ``_FusedAttention.apply`` with the same seed."""
    _device(device)
    B, S, nh, dh = shape
    qkv, mask, dout = _inputs(*shape)
    out, grad, seed = _run(device, qkv, mask, dout, B, S, nh, 0.1, causal=False)
    x = qkv.cuda().bfloat16().requires_grad_(True)
    old = T._FusedAttention.apply(x, mask.cuda(), B, S, nh, 0.1, seed)
    old.backward(dout.cuda().bfloat16())
    assert torch.equal(out, old.detach()) and torch.equal(grad, x.grad)


@pytest.mark.parametrize("device", DEVICES)
def test_unsupported_length_takes_the_pytorch_path(device):
    """S = 96 is no multiple of 64: the PyTorch expression runs (the kernels would refuse the shape)."""
    device = _device(device)
    B, S, nh, dh = 2, 96, 2, 64
    qkv, mask, dout = _inputs(B, S, nh, dh)
    out, grad, _ = _run(device, qkv, mask, dout, B, S, nh)
    ref, gref, _ = _reference(qkv, mask, dout, B, S, nh, dh)
    _check(out, grad, ref, gref, nh * dh)


def test_bert_causal_on_cpu():
    """``Bert("tiny", seq_len=64, causal=True)``, one forward / backward on the CPU: the sequence output at the
    predicted positions (all < 63) ignores the token at position 63, and position 63's embedding gets no gradient."""
    from mdtf.models import Bert, SyntheticBertLoader
    from mdtf.train import step as St
    from mdtf.train import variables as V
    V.reset_default_graph()
    St.reset()
    store = V.get_store()
    store.device = torch.device("cpu")
    store.generator.manual_seed(7)
    ld = SyntheticBertLoader(seq_len=64, max_predictions=5, vocab=512, seed=4)
    ld.batch_size = 2
    raw = ld._make()[0]
    raw[:, -5:] = torch.tensor([0, 7, 31, 32, 62])              # masked_lm_positions
    other = raw.clone()
    other[:, 63] = (raw[:, 63] + 1) % 512
    def logits(causal, r, reuse):
        model = Bert("tiny", vocab_size=512, seq_len=64, max_predictions=5, dropout=0.0, causal=causal)
        with V.variable_scope("net", reuse=reuse):
            return model.inference(r)[0]

    mlm = logits(True, raw, False)
    with torch.no_grad():
        assert torch.equal(mlm, logits(True, other, True))
        assert not torch.equal(logits(False, raw, True), logits(False, other, True))
    mlm.float().sum().backward()
    grad = store.vars["net/bert/embeddings/position_embeddings"].grad
    assert bool((grad[63] == 0).all()) and bool((grad[62] != 0).any())


@pytest.mark.parametrize("device", GPU_ONLY)
def test_hip_graph_replay_equals_eager(device):
    """Forward and backward with dropout captured once and replayed twice: each replay is bitwise the eager result for
    the same step counter (the entries allocate nothing and read nothing on the host)."""
    _device(device)
    shape = B, S, nh, dh = SHAPES[2]
    qkv, mask, dout = _inputs(*shape)
    x = qkv.cuda().bfloat16().requires_grad_(True)
    m, d = mask.cuda(), dout.cuda().bfloat16()

    def step():
        x.grad = None
        with mock.patch.object(torch, "randint", lambda *a, **k: torch.tensor([1234567])):
            out = T.fused_attention(x, B, S, nh, m, 0.1, causal=True)
        out.backward(d)
        return out.detach(), x.grad

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = step()
    for _ in range(2):
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager[0], out[0]) and torch.equal(eager[1], out[1])
    del graph
