"""``mdtf.nn.group_norm`` / ``tools.group_norm`` and the kernels of ``csrc/groupnorm.hip`` against the fp64 oracle of
``group_norm_helpers``, element by element, at the smallest shapes at which the group folding, the strip and chunk
index arithmetic and the variance can still be wrong.

``cpu`` runs the PyTorch expression on fp32 tensors holding bf16 values; ``cuda`` runs the HIP kernels, parameters
with fp32 gradient slots, once per design (``path`` 1 resident, 2 streaming).  Bounds: ``group_norm_helpers``.
"""
import functools
import os
import sys
import types

import pytest
import torch

import mdtf
from mdtf.ops import _native
from mdtf.ops import nn as ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_norm_helpers as GH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
EINVAL, EPS = -1, 1e-6

CASES = [(2, 3, 3, 8, 1, 0.0),         # (N, H, W, C, G, shift); one group of everything
         (2, 5, 7, 16, 2, 0.0),        # Cg = 8: vector-aligned groups
         (1, 4, 4, 24, 8, 0.0),        # Cg = 3: groups straddling vectors
         (2, 3, 5, 32, 32, 0.0),       # Cg = 1: instance norm
         (3, 7, 7, 64, 32, 0.0),       # Cg = 2, odd H * W, three images in the parameter-gradient order
         (1, 1, 1, 16, 2, 0.0),        # m = 8
         (2, 13, 13, 40, 5, 0.0),      # five vectors per pixel
         (2, 5, 7, 16, 2, 30.0)]       # mean >> std: no variance as E[x^2] - mean^2
CASE_IDS = ["%dx%dx%dx%d_g%d%s" % (c[:5] + ("_shift" if c[5] else "",)) for c in CASES]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


class _Case(object):
    def __init__(self, n, h, w, c, g, shift, seed):
        self.G = g
        self.x = NH.bf16_exact(NH.randn((n, h, w, c), seed) + shift)
        self.g = NH.bf16_exact(NH.randn((c,), seed + 1, 0.5) + 1.0)
        self.b = NH.randn((c,), seed + 2, 0.5)
        self.dy = NH.randn((n, h, w, c), seed + 3)

    @functools.lru_cache(maxsize=None)
    def ref(self, K=1):
        return GH.Ref(self.x, self.g, self.b, self.dy, self.G, EPS, K)

    def chunks(self, device, path):
        if device == "cpu" or path != 2:
            return 1
        from mdtf.ops import groupnorm
        c = self.x.shape[3]
        return -(-self.x.shape[1] * self.x.shape[2] // (groupnorm.chunk_vectors(c) // (c // 8)))


@functools.lru_cache(maxsize=None)
def _case(i):
    return _Case(*CASES[i], seed=100 + 10 * i)


def _run(device, case, act, path=None, slot0=None):
    """forward + backward through ``mdtf.nn.group_norm``.  cuda: bf16 x, fp32 parameters whose gradients land in fp32
    slots (pre-filled with ``slot0`` or zeros); cpu: fp32, the gradients in ``.grad`` (plus ``slot0``)."""
    xd = NH.put(case.x, device).requires_grad_(True)
    gd, bd = case.g.clone().to(device).requires_grad_(True), case.b.clone().to(device).requires_grad_(True)
    s0 = slot0 if slot0 is not None else (torch.zeros_like(case.g), torch.zeros_like(case.b))
    if device == "cuda":
        slots = [s.to(device).contiguous() for s in s0]
        gd._mdtf_var, bd._mdtf_var = types.SimpleNamespace(grad=slots[0]), types.SimpleNamespace(grad=slots[1])
    y = ops.group_norm(xd, gd, bd, case.G, EPS, act, path=path)
    y.backward(NH.put(case.dy, device))
    if device == "cpu":
        slots = [gd.grad + s0[0], bd.grad + s0[1]]
    return y.detach(), xd.grad, slots[0], slots[1]


def _check(what, device, case, act, got, K=1, slot0=None):
    y, dx, dg, db = got
    bf = device == "cuda"
    assert y.dtype == (torch.bfloat16 if bf else torch.float32) and dx.dtype == y.dtype
    assert dg.dtype == torch.float32 and db.dtype == torch.float32
    s0 = slot0 or (None, None)
    out = case.ref(K).outputs(act == "relu", y.cpu() > 0, bf, what, s0[0], s0[1])
    for name, t in zip(("y", "dx", "dgamma", "dbeta"), got):
        NH.check_bound(t, out[name], out[name + "_bound"], "%s %s" % (what, name))


def _paths(device, shape, G):
    if device == "cpu":
        return [None]
    from mdtf.ops import groupnorm
    fits = groupnorm.resident_fits(shape[1], shape[2], shape[3], G, True)
    return ([1] if fits else []) + [2]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case(i, act, device):
    device = _device(device)
    case = _case(i)
    paths = _paths(device, case.x.shape, case.G)
    assert device == "cpu" or paths == [1, 2], "every listed case fits the resident kernels"
    for path in paths:
        what = "%s %s %s path %s" % (CASE_IDS[i], act, device, path)
        K = case.chunks(device, path)
        got = _run(device, case, act, path)
        _check(what, device, case, act, got, K)
        if device == "cuda":
            from mdtf.ops import groupnorm
            y2, mean, rstd = groupnorm.forward_nhwc(NH.put(case.x, device), case.g.to(device), case.b.to(device),
                                                    case.G, EPS, act == "relu", path)
            assert NH.bits_equal(y2, got[0]), "the entry point and the autograd wrapper disagree"
            rm, em, rr, er = case.ref(K).stats()
            NH.check_bound(mean, rm, em, what + " mean")
            NH.check_bound(rstd, rr, er, what + " rstd")
            for a, b in zip(got, _run(device, case, act, path)):
                assert NH.bits_equal(a, b), "two runs differ"


@pytest.mark.parametrize("device", DEVICES)
def test_two_streaming_chunks(device):
    """One image of more pixels than a streaming chunk holds, the boundary inside an image row."""
    device = _device(device)
    c, side = 16, 40
    if device == "cuda":
        from mdtf.ops import groupnorm
        pixels = groupnorm.chunk_vectors(c) // (c // 8)
        side = next(s for s in range(3, 4096) if s * s > pixels and pixels % s)
    case = _Case(1, side, side, c, 4, 0.0, 700)
    for path in _paths(device, case.x.shape, case.G):
        K = case.chunks(device, path)
        assert device == "cpu" or path == 1 or K == 2
        _check("chunks %d path %s" % (side, path), device, case, "relu", _run(device, case, "relu", path), K)


@pytest.mark.parametrize("device", DEVICES)
def test_parameter_gradients_add_into_filled_slots(device):
    device = _device(device)
    case = _case(4)
    slot0 = (NH.randn((64,), 7, 4.0), NH.randn((64,), 8, 4.0))
    for path in _paths(device, case.x.shape, case.G):
        got = _run(device, case, "relu", path, slot0)
        _check("slot %s path %s" % (device, path), device, case, "relu", got, slot0=slot0)


_p = lambda g: _native.ptr(g.t if isinstance(g, NH.Guarded) else g)  # noqa: E731


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("path", [1, 2])
def test_entry_points_on_guarded_buffers(path, device):
    """Guards intact, inputs unchanged, every output element stored and finite; refusals before any launch."""
    device = _device(device)
    from mdtf.ops import groupnorm  # noqa: F401  (registers the signatures)
    case = _case(6)
    n, h, w, c = case.x.shape
    G = case.G
    gx, gdy = NH.Guarded(case.x.bfloat16(), device), NH.Guarded(case.dy.bfloat16(), device)
    gg, gb = NH.Guarded(case.g, device), NH.Guarded(case.b, device)
    gy, gdx = (NH.Guarded(None, device, torch.bfloat16, case.x.shape) for _ in range(2))
    gmean, grstd = (NH.Guarded(None, device, torch.float32, (n, G)) for _ in range(2))
    gdg, gdb = (NH.Guarded(None, device, torch.float32, (c,)) for _ in range(2))
    wf = int(_native.fn("mdtf_gn_fwd_ws")(n, h, w, c, G, path))
    wb = int(_native.fn("mdtf_gn_bwd_ws")(n, h, w, c, G, path))
    assert (wf > 0) == (path == 2) and wb >= 2 * n * c
    gwf, gwb = NH.Guarded(None, device, torch.float32, (max(wf, 4),)), NH.Guarded(None, device, torch.float32, (wb,))

    def fwd(x, y, c_=c, g_=G, p=path):
        rc = _native.fn("mdtf_gn_fwd")(_p(x), _p(gg), _p(gb), _p(y), _p(gmean), _p(grstd), _p(gwf), n, h, w, c_, g_,
                                       EPS, 1, p, _native.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def bwd(c_=c, g_=G, p=path):
        rc = _native.fn("mdtf_gn_bwd")(_p(gx), _p(gdy), _p(gg), _p(gb), _p(gmean), _p(grstd), _p(gdx), _p(gdg),
                                       _p(gdb), _p(gwb), n, h, w, c_, g_, 1, 0, p, _native.stream_ptr())
        torch.cuda.synchronize()
        return rc
    assert fwd(gx, gy, c_=c - 4) == EINVAL and fwd(gx, gy, g_=3) == EINVAL          # C % 8, C % G
    assert bwd(c_=c - 4) == EINVAL and bwd(g_=3) == EINVAL
    for g in (gx, gdy, gg, gb, gy, gdx, gmean, grstd, gdg, gdb, gwf, gwb):
        assert g.unchanged()
    assert fwd(gx, gy) == 0
    NH.assert_contained("gn_fwd", [gx, gg, gb], [gy, gmean, grstd] + ([gwf] if path == 2 and wf >= 4 else []))
    for g in (gmean, grstd):
        g.before = g.buf.clone()                       # now inputs
    assert bwd() == 0
    NH.assert_contained("gn_bwd", [gx, gdy, gg, gb, gmean, grstd], [gdx, gdg, gdb, gwb])
    for g in (gy, gdx, gmean, grstd, gdg, gdb):
        assert bool(torch.isfinite(g.t.float()).all())
    _check("raw path %d" % path, device, case, "relu", (gy.t, gdx.t, gdg.t, gdb.t), case.chunks(device, path))
    # a strip that does not fit the resident kernels
    big = (64, 64, 64, 2)
    assert not _native.fn("mdtf_gn_resident_fits")(*big, 0)
    xb = torch.zeros((1,) + big[:3], dtype=torch.bfloat16, device=device)
    gbig = NH.Guarded(torch.ones(64), device)
    st = NH.Guarded(None, device, torch.float32, (1, 2))
    rc = _native.fn("mdtf_gn_fwd")(_p(xb), _p(gbig), _p(gbig), _p(torch.empty_like(xb)), _p(st), _p(st), _p(gwf), 1,
                                   *big, EPS, 0, 1, _native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == EINVAL and st.unchanged()


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("path", [1, 2])
def test_replays_in_a_graph(path, device):
    """forward + backward captured once and replayed twice after x changed in place give the eager bits."""
    device = _device(device)
    case, other = _case(4), _Case(*CASES[4], seed=900)
    xd = NH.put(other.x, device).requires_grad_(True)
    gd, bd = case.g.clone().to(device).requires_grad_(True), case.b.clone().to(device).requires_grad_(True)
    slots = [torch.zeros(64, device=device), torch.zeros(64, device=device)]
    gd._mdtf_var, bd._mdtf_var = types.SimpleNamespace(grad=slots[0]), types.SimpleNamespace(grad=slots[1])
    dyd = NH.put(case.dy, device)

    def step():
        xd.grad = None
        y = ops.group_norm(xd, gd, bd, case.G, EPS, "relu", path=path)
        y.backward(dyd)
        return y.detach(), xd.grad
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = step()
    eager = _run(device, case, "relu", path)
    with torch.no_grad():
        xd.copy_(NH.put(case.x, device))
    for _ in range(2):
        for t in slots:
            t.zero_()
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, (out[0], out[1], slots[0], slots[1])):
            assert NH.bits_equal(a, b), "a replay differs from the eager run"
    del graph


def test_api_errors():
    x, g = torch.zeros(1, 4, 4, 16), torch.ones(16)
    for bad in (lambda: mdtf.nn.group_norm(x[0], g, g, 4), lambda: mdtf.nn.group_norm(x, g, g, 5),
                lambda: mdtf.nn.group_norm(x, g[:8], g, 4), lambda: mdtf.nn.group_norm(x, g, g[:8], 4),
                lambda: mdtf.nn.group_norm(x, g, g, 4, act="gelu")):
        with pytest.raises(ValueError):
            bad()
    assert mdtf.nn.group_norm(x, g, g, 4, act="relu").shape == x.shape


def test_tools_group_norm_trains_its_two_variables():
    """``GroupNorm/gamma`` (ones) and ``GroupNorm/beta`` (zeros), nothing else, and one CPU step moves both."""
    from mdtf.layers import tools
    from mdtf.models import SoftmaxCrossEntropyLoss
    from mdtf.runtime import Model, Net, Tower
    from mdtf.train import variables as V

    class M(Model):
        def inference(self, x):
            return tools.dense("logits", ops.global_avg_pool(tools.group_norm(x, groups=4, relu=True)), 16)
    store = V.get_store()
    store.device, store.compute_dtype = torch.device("cpu"), None
    store.generator.manual_seed(11)
    xp, yp = mdtf.placeholder(torch.float32, [None, 6, 6, 16]), mdtf.placeholder(torch.int64, [None])
    opt = mdtf.train.GradientDescentOptimizer(0.5)
    tg = []
    _, loss, _ = Tower(Net(M()), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), opt, batch_size=2).process()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    names = sorted(v.name for v in store.trainable_variables() if v.name.startswith("GroupNorm"))
    assert names == ["GroupNorm/beta", "GroupNorm/gamma"]
    gam, bet = store.vars["GroupNorm/gamma"], store.vars["GroupNorm/beta"]
    assert gam.keep_fp32 and bet.keep_fp32 and gam.shape == (16,) and bet.shape == (16,)
    assert bool((gam.value() == 1).all()) and bool((bet.value() == 0).all())
    sess.run([op, loss], feed_dict={xp: NH.randn((2, 6, 6, 16), 500), yp: torch.tensor([3, 6])})
    assert bool((gam.value() != 1).any()) and bool((bet.value() != 0).any())
