"""``mdtf.nn.ctc_loss`` (``ops/ctc.py``, ``csrc/ctc.hip``) against ``torch.nn.functional.ctc_loss`` on CPU in fp64 over
an fp64 ``log_softmax`` of the bf16-representable inputs (blank = K - 1, ``reduction='none'``, the gradient by
autograd with a non-uniform upstream ``g``).  ``cpu`` runs the PyTorch expression on fp32 tensors, ``cuda`` the HIP
kernels on bf16 (or fp32) tensors.

Limits (``U = 2^-24``; ``ctc_helpers.oracle``), derived from the code as written, ``check_bound`` on every element:

* one guarded log-add ``m + log(sum_i exp(a_i - m))`` of three terms, the sum ``s`` in [1, 3]: the two differences
  that are not 0 round once and so does the intrinsic's scaling of its argument, each ``|d| e^d U <= U / e`` (1.5 U
  together); ``__expf`` and ``__logf`` are taken at 2 ulp = 4 U relative (the ISA's v_exp_f32 / v_log_f32 are 1 ulp;
  no device-library accuracy table ships with the toolchain here, so this is twice the hardware figure, not a
  documented one): 4 U relative to ``s``, two additions 2 U, and ``(4 + 1) U log 3 = 5.5 U`` for the logarithm and its
  scaling.  ``C_LOGADD = 13``.
* loss: ``E_b = sum_{t < T_b} [e_lse(t) + U (A_t + P_t + C_LOGADD)]`` with ``A_t = max_s |alpha_t(s)|`` over the
  finite states, taken from the fp64 oracle's own alpha (``torch._ctc_loss``), and ``P_t = max_s |lp[t, s]|``.
  ``e_lse`` is ``nhwc_helpers.lse_bound``; it enters through ``lp = x - lse``, which rounds once at ``P_t``;
  ``lp + (m + log s)`` rounds once at ``A_t``.  Errors pass through a log-sum-exp with weight at most 1, so they add
  up over t and never grow.  (The form has one rounding at each magnitude: the rounding of ``m + log s`` itself, at
  ``A_t - P_t``, and the final two-term log-add have no term of their own.)
* gradient: ``|g_b| (e_p + occ_k (2 E_b + C_GRAD U))`` plus ``out_bound``'s rounding to the output dtype.  ``e_p`` is
  the fp32 softmax bound of ``test_losses.py``; ``occ_k`` counts the states that hold symbol k; ``E_b`` bounds the
  error of an exponent ``z = alpha + beta - lp + loss <= 0``, of which ``exp`` makes an absolute error of at most
  the same size.  ``C_GRAD = 9``: per term the intrinsic at 2 ulp (4 U) and its argument scaling with the last
  rounding of ``z`` (``2 |z| e^z U <= U``), the term's addition into the ordered sum (1 U, the sum is at most 1), and
  the subtraction from ``p``, the product with ``g_b`` and the second ``__expf`` (3 U, shared by the terms).

Both devices are held to the same limits: ``cpu`` runs PyTorch's own fp32 ``F.ctc_loss``.  Measured ratios:
``profiles/ctc.md``, "Limits".
"""
import os
import sys

import pytest
import torch

import mdtf
from mdtf.ops import _native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_helpers as CH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
UNSUPPORTED = -2
# (T, B, K, Lmax).  small: a repeated label, an empty one, an item with exactly one alignment, an item shorter than T
# (wave variant) | S = 63 and 65: either side of the wave / block switch | S = 261: two states per thread and the LDS
# apron | K = 2050: the row kernels' block-per-row form, K no multiple of 8
CASES = {"small": CH.Case(6, 4, 5, 2, 11, labels=[[1, 1], [0, 0], [2, 3], [0, 2]], seq=[6, 5, 2, 4],
                          lab_len=[2, 0, 2, 2]),
         "S63": CH.Case(70, 2, 40, 31, 12), "S65": CH.Case(70, 2, 40, 32, 13), "S261": CH.Case(270, 2, 7, 130, 14),
         "K2050": CH.Case(4, 2, 2050, 1, 15)}
RUNS = [pytest.param(n, d, torch.float32 if d == "cpu" else torch.bfloat16, True, id="%s-%s" % (n, d),
                     marks=[pytest.mark.gpu] * (d == "cuda")) for n in CASES for d in ("cpu", "cuda")]
RUNS += [pytest.param(n, "cuda", torch.float32, True, id=n + "-cuda-fp32", marks=pytest.mark.gpu)
         for n in ("small", "K2050")]
RUNS += [pytest.param("small", d, torch.float32 if d == "cpu" else torch.bfloat16, False, id="small-batch-major-" + d,
                      marks=[pytest.mark.gpu] * (d == "cuda")) for d in ("cpu", "cuda")]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _run(device, c, dtype=None, time_major=True, ignore=False, x=None, items=None, seq=None):
    """(loss [B], d inputs [T, B, K]) of ``mdtf.nn.ctc_loss`` on the case, its lengths as int32 device tensors."""
    dtype = dtype or (torch.float32 if device == "cpu" else torch.bfloat16)
    items = list(range(c.shape[1])) if items is None else items
    x = (c.x if x is None else x)[:, items].to(device).to(dtype)
    x = (x if time_major else x.transpose(0, 1).contiguous()).requires_grad_(True)
    seq = c.seq if seq is None else seq
    loss = mdtf.nn.ctc_loss(c.labels[items].to(device), x, seq[items].to(device), time_major=time_major,
                            ignore_longer_outputs_than_inputs=ignore, label_length=c.lab_len[items].to(device))
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (len(items),)
    loss.backward(c.g[items].to(device))
    assert x.grad.dtype == dtype
    return loss.detach(), (x.grad if time_major else x.grad.transpose(0, 1))


@pytest.mark.parametrize("name,device,dtype,time_major", RUNS)
def test_matches_the_fp64_oracle(name, device, dtype, time_major):
    device = _device(device)
    c = CASES[name]
    loss, dx = _run(device, c, dtype, time_major)
    what = "ctc %s %s %s" % (name, device, dtype)
    NH.check_bound(loss, c.ref["loss"], c.ref["e_loss"], what + " loss")
    dead = torch.arange(c.shape[0])[:, None] >= c.seq[None, :]
    assert not bool(dx.cpu()[dead].any()), what + ": gradient at frames past the length"
    NH.check_bound(dx, c.ref["dx"], NH.out_bound(c.ref["dx"], c.ref["acc"], dtype == torch.bfloat16), what + " dx")


@pytest.mark.parametrize("kind", ["too-long", "label-out-of-range"])
@pytest.mark.parametrize("device", DEVICES)
def test_infeasible_item(device, kind):
    """Item 1 has no alignment ([1, 1, 1] needs 5 frames and has 4; or a label K - 1): loss exactly +inf, or 0 with
    ignore_longer_outputs_than_inputs, gradient exactly 0, the neighbours bit-identical to a batch without it."""
    device = _device(device)
    labels = [[0, 1, 2], [1, 1, 1], [2, 2, 0]] if kind == "too-long" else [[0, 1, 2], [1, 3, 0], [2, 2, 0]]
    c = CH.Case(5, 3, 4, 3, 21, labels=labels, seq=[5, 4, 5], lab_len=[3, 3, 2])
    alone = _run(device, c, items=[0, 2])
    for ignore, want in ((True, 0.0), (False, float("inf"))):
        loss, dx = _run(device, c, ignore=ignore)
        assert float(loss[1]) == want and not bool(dx[:, 1].any())
        assert NH.bits_equal(loss[[0, 2]], alone[0]) and NH.bits_equal(dx[:, [0, 2]], alone[1])
        assert bool(torch.isfinite(loss[[0, 2]]).all()) and bool(dx[:, 0].any())


@pytest.mark.parametrize("device", DEVICES)
def test_nan_in_dead_frames_and_infeasible_items(device):
    device = _device(device)
    c = CH.Case(6, 3, 5, 2, 22, labels=[[1, 1], [0, 0], [2, 3]], seq=[4, 1, 6], lab_len=[2, 2, 2])  # item 1: infeasible
    x = c.x.clone()
    x[4:, 0] = float("nan")
    x[:, 1] = float("nan")
    clean, poisoned = _run(device, c, ignore=True), _run(device, c, ignore=True, x=x)
    assert NH.bits_equal(clean[0], poisoned[0]) and NH.bits_equal(clean[1], poisoned[1])
    assert bool(torch.isfinite(poisoned[0]).all()) and bool(torch.isfinite(poisoned[1]).all())
    assert not bool(poisoned[1][4:, 0].any()) and not bool(poisoned[1][:, 1].any()) and bool(poisoned[1][:4, 0].any())


def _entry_points(c, device, seq):
    """Buffers for the three entry points and a function that enqueues them on the current stream."""
    t, b, k, lmax = c.shape
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
    z = dict(lse=new(t, b), lpc=new(t, b, lmax + 1), chain=new(b, lmax, dtype=torch.int32),
             flag=new(b, dtype=torch.int32), alpha=new(t, b, 2 * lmax + 1), beta=new(t, b, 2 * lmax + 1), loss=new(b),
             dx=new(t, b, k, dtype=torch.bfloat16))
    x, lab, ln, g = c.x.to(device).bfloat16(), c.labels.int().to(device), c.lab_len.to(device), c.g.to(device)
    P = _native.ptr

    def call():
        dims = (t, b, k, lmax, 0, _native.stream_ptr())
        lens = (P(lab), P(seq), P(ln))
        _native.check(_native.fn("mdtf_ctc_rows")(P(x), *lens, P(z["lse"]), P(z["lpc"]), P(z["chain"]), P(z["flag"]),
                                                  *dims), "ctc_rows")
        _native.check(_native.fn("mdtf_ctc_alpha_beta")(P(z["lpc"]), *lens, P(z["flag"]), P(z["alpha"]), P(z["beta"]),
                                                        P(z["loss"]), 0, *dims), "ctc_alpha_beta")
        _native.check(_native.fn("mdtf_ctc_grad")(P(x), *lens, P(z["flag"]), P(z["chain"]), P(z["lse"]), P(z["lpc"]),
                                                  P(z["alpha"]), P(z["beta"]), P(z["loss"]), P(g), P(z["dx"]), *dims),
                      "ctc_grad")
    return z, call


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("name", ["small", "S65"])
def test_repeatable_and_replays_in_a_graph_with_new_lengths(name, device):
    """Two runs are bit-identical; the three entry points, captured once, are replayed after the lengths tensor
    changed in place and equal an eager run with the new lengths bit for bit."""
    device = _device(device)
    c = CASES[name]
    from mdtf.ops import ctc  # noqa: F401  (registers the signatures)
    first, again = _run(device, c), _run(device, c)
    assert NH.bits_equal(first[0], again[0]) and NH.bits_equal(first[1], again[1])
    seq = c.seq.to(device)
    z, call = _entry_points(c, device, seq)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for new_seq in (c.seq - 1, c.seq):
        seq.copy_(new_seq)                                       # in place: the graph holds the tensor's address
        want_loss, want_dx = _run(device, c, seq=new_seq)
        for _ in range(2):
            z["loss"].fill_(1.0), z["dx"].fill_(1.0)
            g.replay()
            torch.cuda.synchronize()
            assert NH.bits_equal(z["loss"], want_loss) and NH.bits_equal(z["dx"], want_dx), new_seq


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("lmax,code", [(512, 0), (8, 2)], ids=["Lmax512", "fp16"])
def test_entry_points_refuse(lmax, code, device):
    device = _device(device)
    from mdtf.ops import ctc  # noqa: F401
    p = [_native.ptr(torch.zeros(4096, dtype=torch.int32, device=device)) for _ in range(13)]
    dims = (2, 2, 8, lmax, code, _native.stream_ptr())
    assert _native.fn("mdtf_ctc_rows")(*p[:8], *dims) == UNSUPPORTED
    assert _native.fn("mdtf_ctc_alpha_beta")(*p[:8], 0, *dims) == UNSUPPORTED
    assert _native.fn("mdtf_ctc_grad")(*p, *dims) == UNSUPPORTED


def test_argument_checks():
    x, labels, seq, ln = torch.zeros(4, 2, 5), torch.zeros(2, 3, dtype=torch.long), [4, 4], [1, 1]
    for kw in (dict(preprocess_collapse_repeated=True), dict(ctc_merge_repeated=False)):
        with pytest.raises(NotImplementedError):
            mdtf.nn.ctc_loss(labels, x, seq, label_length=ln, **kw)
    bad = [dict(), dict(label_length=[1]), dict(label_length=ln, sequence_length=[4]),
           dict(label_length=ln, sequence_length=torch.tensor(4)),
           dict(label_length=ln, inputs=x[0]), dict(label_length=ln, labels=labels[:1]),
           dict(label_length=ln, labels=labels.float()), dict(label_length=ln, inputs=x[:, :, :1])]
    for kw in bad:
        args = dict(labels=labels, inputs=x, sequence_length=seq)
        args.update(kw)
        with pytest.raises(ValueError):
            mdtf.nn.ctc_loss(**args)
    from mdtf.ops import losses as OL
    assert tuple(OL.reduce_rows(mdtf.nn.ctc_loss(labels, x, seq, label_length=ln)).shape) == ()
