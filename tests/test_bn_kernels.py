"""The BatchNorm kernels of ``csrc/bn.hip`` (training forward / backward, the partial-statistics and early-finalize
entry points, inference, the dual form ``relu(BN(x) + BN2(r))`` and the stem form ``maxpool(relu(BN(x)))``) against
the fp64 oracles of ``bn_helpers``, element by element, at the smallest shapes that reach each code path.

Every test takes a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.nn.batch_norm`` on fp32 tensors holding
bf16-representable values (this validates the oracles, the bounds and the exclusion caps without a GPU); ``cuda``
runs the HIP kernels on bf16 tensors, through the autograd wrappers and once more through the registered entry points
with every buffer inside sentinel guard bands (guards intact, inputs bitwise unchanged except the buffers the API
says it rewrites, every output element stored).

The bounds are derived in ``bn_helpers``; the operation count k of every ``gamma(k)`` stands next to its use there.
Every training case carries the planted channels of ``bn_helpers.bn_case``: constant 0, constant 77/256 (variance 0,
invstd = eps^-1/2), mean 64 with unit spread, gamma < 0 and gamma = 0.  eps and decay are the defaults of
``ops.batch_norm`` (1e-3, 0.9): with eps = 1e-5 the bound of the constant channel's invstd is unbounded on ``cpu`` at
M = 523, where k = M, and the whole channel would count as undetermined; ``test_train_eps_1e5`` repeats the training
cases at 1e-5 on ``cuda``, where k is the kernels' own.

On the MI355X the 42 ``cuda`` cases of the file take 7 s, the slowest (the first, which loads the library) 1.2 s; the
observed shares of the bounds are recorded in ``bn_helpers``.
"""
import os
import sys

import pytest
import torch

from mdtf.ops import _native
from mdtf.ops import nn as ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_helpers as BH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import TINY, U, gamma  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
EPS, DECAY = 1e-3, 0.9             # the defaults of ops.batch_norm
# M x C.  C: 8 (tpr 1, rg 256) | 24 (two channel blocks, the second half empty; 2048 % C != 0) | 64 | 192 (not fixed,
# half-empty second block) | 2048 (rg 1: no tree) | 2056 (one vector in the second channel block).  M: 1 | 5 (fewer
# rows than row groups) | 37 | 523 (unrolled and tail loops, uneven rows per group, several row blocks at C >= 64, a
# partly filled last elementwise block at C = 24) | 129 x 64: 1032 vectors, just past one 1024-vector block | 45 x 2048:
# three row blocks of 15 rows, 4 j + 3 rows per thread: an unrolled trip that ran one row too far would count a row of
# the next block twice (at the other shapes it could only read past the last row).
SHAPES = [(1, 8), (5, 8), (37, 24), (523, 24), (5, 64), (129, 64), (523, 64), (37, 192), (523, 192), (1, 2048),
          (37, 2048), (45, 2048), (5, 2056), (523, 2056)]
P_LIST = [1, 33, 128, 131, 261]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _raw(name, *args):
    """A registered entry point called the way ``ops/bn.py`` calls it."""
    from mdtf.ops import bn  # noqa: F401  (registers the signatures)
    _native.check(_native.fn(name)(*args, _native.stream_ptr()), name)
    torch.cuda.synchronize()


def _p(g):
    return _native.ptr(g.t if isinstance(g, NH.Guarded) else g)


def G(t, dtype=None, shape=None):
    return NH.Guarded(t, "cuda", dtype, shape)


def _ws_floats(M, C):
    from mdtf.ops import bn  # noqa: F401
    return int(_native.fn("mdtf_bn_workspace_floats")(M, C))


def _k(device, M, C):
    """fp32 additions on the longest path of a statistics sum: the kernels' geometry, or any order (k = M); never
    more than M - 1: M terms meet in M - 1 additions, every other one has an exact zero for an operand."""
    return min(M if device == "cpu" else BH.reduce_k(M, C, _ws_floats(M, C)), M - 1)


def _one_minus(device):
    d = BH.f32(DECAY)
    return BH.f32(1.0 - DECAY) if device == "cpu" else 1.0 - d


def _slot(t, slot, device):
    """Give parameter ``t`` a non-zero fp32 gradient slot the backward accumulates onto."""
    if device == "cuda":
        class Var(object):                  # what variables.grad_sink looks for
            grad = slot
        t._mdtf_var = Var()
    else:
        t.grad = slot
    return t


def _param(v, slot0, device):
    t = v.to(device).requires_grad_(True)
    slot = slot0.to(device).clone()
    return _slot(t, slot, device), slot


def _zeroed_head(what, g, buf0, P):
    """A partial-statistics buffer after its finalize: guards intact, rows < P zero, rows >= P as they were."""
    assert g.guards_intact(), what + ": wrote outside the partials"
    assert not bool(g.t[:P].any()), what + ": partial rows not re-zeroed"
    assert NH.bits_equal(g.t[P:].cpu(), buf0[P:]), what + ": rows past P changed"


# ====================================================================================== training forward / backward
def _check_fwd(what, device, c, st, relu, with_res, y, mm, mv, mean=None, invstd=None, mask=None):
    bf = device == "cuda"
    if bf:
        assert bool(st.ok.all()), what + ": a bound is unbounded"
    pre, acc = BH.fwd_ref(c["x"], st, c["g"], c["b"], c["res"] if with_res else None)
    pos = None
    yref = pre
    if relu:
        ypos = y.detach().float().cpu() > 0
        got = BH.unpack_mask(mask, pre.shape) if mask is not None else ypos
        pos, _ = BH.relu_sign(pre, acc, got, what)
        yref = torch.where(pos, pre, torch.zeros_like(pre))
        if mask is not None:
            bad = got != pos
            assert not bool(bad.any()), "%s: %d mask bits wrong, first at element %d" % (
                what, int(bad.sum()), int(bad.flatten().nonzero()[0]))
            assert torch.equal(got, ypos), what + ": mask bits differ from [y > 0]"
    NH.check_bound(y, yref, NH.out_bound(yref, acc, bf), what + " y")
    if mm is not None:
        mmr, emm, mvr, emv = BH.moving_ref(st, c["mm0"], c["mv0"], BH.f32(DECAY), _one_minus(device))
        NH.check_bound(mm, mmr, emm, what + " mmean")
        NH.check_bound(mv, mvr, emv, what + " mvar")
    if mean is not None:
        NH.check_bound(mean, st.mean, st.emf + TINY, what + " mean")
        NH.check_bound(invstd, st.inv, st.einv + TINY, what + " invstd")
        if st.M > 1:            # the channel whose mean dwarfs its spread: how much of k U (1 + mean^2 / var) is used
            big = BH.CH_BIG
            print("BN_BIGMEAN %-56s invstd at %.3f of its bound" % (
                what, float((invstd.cpu().double()[big] - st.inv[big]).abs() / st.einv[big])))
    return pre, acc, pos


def _check_bwd(what, device, c, st, pos, k, dx, dres, dgamma, dbeta, accum=False, slots=True, sums=None):
    bf = device == "cuda"
    r = BH.bwd_ref(c["x"], c["dy"], pos, st, c["g"], k, sums=sums, dres0=c["dres0"] if accum else None,
                   dg0=c["dg0"] if slots else None, db0=c["db0"] if slots else None, bf=bf)
    NH.check_bound(dx, r["dx"], r["dx_bound"], what + " dx")
    if dres is not None:
        NH.check_bound(dres, r["dres"], r["dres_bound"], what + " dres")
    NH.check_bound(dgamma, r["dgamma"], r["dgamma_bound"], what + " dgamma")
    NH.check_bound(dbeta, r["dbeta"], r["dbeta_bound"], what + " dbeta")
    return r


def _train_autograd(device, c, relu, with_res, accum=False, eps=EPS):
    """``accum``: the residual's gradient already holds another consumer's contribution: ``res.grad`` on ``cpu``; on
    ``cuda`` the residual's gradient sink (ops.actsink), which the backward must accumulate into in place."""
    x = NH.put(c["x"], device).requires_grad_(True)
    res = NH.put(c["res"], device).requires_grad_(True) if with_res else None
    sink = None
    if accum and device == "cuda":
        from mdtf.ops import actsink
        sink = actsink.attach(res)
        assert sink is not None
    g, gs = _param(c["g"], c["dg0"], device)
    b, bs = _param(c["b"], c["db0"], device)
    mm, mv = c["mm0"].to(device).clone(), c["mv0"].to(device).clone()
    y = ops.batch_norm(x, g, b, mm, mv, True, DECAY, eps, relu, res)
    saved = y.grad_fn.saved_tensors if device == "cuda" else None
    if sink is not None:
        sink.adopt_or_add(NH.put(c["dres0"], device))           # the other consumer came first
    elif accum:
        res.grad = c["dres0"].clone()
    y.backward(NH.put(c["dy"], device))
    dg, db = (gs, bs) if device == "cuda" else (g.grad, b.grad)
    dres = res.grad if with_res else None
    if sink is not None:
        assert dres is None and sink.count == 2, "the backward did not deliver its residual gradient through the sink"
        dres = sink.buf
    return dict(y=y.detach(), mm=mm, mv=mv, mean=saved[3] if saved else None, invstd=saved[4] if saved else None,
                mask=saved[1] if (saved and relu) else None, dx=x.grad, dres=dres, dgamma=dg, dbeta=db)


def _train_raw_fwd(what, c, relu, with_res, eps=EPS):
    M, C = c["x"].shape
    gx, gres = G(c["x"].bfloat16()), G(c["res"].bfloat16())
    gg, gb, gmm, gmv = G(c["g"]), G(c["b"]), G(c["mm0"]), G(c["mv0"])
    gy = G(None, torch.bfloat16, (M, C))
    gmask = G(None, torch.uint8, (M * C // 8,))
    gmean, ginv = G(None, torch.float32, (C,)), G(None, torch.float32, (C,))
    gws = G(None, torch.float32, (_ws_floats(M, C),))
    _raw("mdtf_bn_fwd_train", _p(gx), _p(gres) if with_res else _native.ptr(None), _p(gy), _p(gmask), M, C, _p(gg),
         _p(gb), _p(gmm), _p(gmv), BH.f32(DECAY), BH.f32(eps), int(relu), _p(gmean), _p(ginv), _p(gws))
    NH.assert_contained(what, [gx, gres, gg, gb], [gy, gmean, ginv])
    for g_ in (gmm, gmv, gws, gmask):
        assert g_.guards_intact(), what + ": wrote outside a buffer"
    if not relu:
        assert gmask.unchanged(), what + ": mask written without ReLU"
    return dict(y=gy.t, mm=gmm.t, mv=gmv.t, mean=gmean.t, invstd=ginv.t, mask=gmask.t if relu else None)


def _train_raw_bwd(what, c, st, pos, dres_mode):
    """mdtf_bn_bwd on guarded buffers; the mask is packed from the oracle's decisions and the saved statistics are
    the oracle's, rounded to fp32: the backward is tested independently of the forward."""
    M, C = c["x"].shape
    relu = pos is not None
    gdy, gx, gg = G(c["dy"].bfloat16()), G(c["x"].bfloat16()), G(c["g"])
    gmask = G(BH.pack_mask(pos)) if relu else None
    gmean, ginv = G(st.mean.float()), G(st.inv.float())
    gdx = G(None, torch.bfloat16, (M, C))
    gdres = None
    if dres_mode == "written":
        gdres = G(None, torch.bfloat16, (M, C))
    elif dres_mode == "accumulated":
        gdres = G(c["dres0"].bfloat16())
    gdg, gdb = G(c["dg0"]), G(c["db0"])
    gws = G(None, torch.float32, (_ws_floats(M, C),))
    _raw("mdtf_bn_bwd", _p(gdy), _p(gx), _p(gmask) if relu else _native.ptr(None), _p(gdx),
         _p(gdres) if gdres else _native.ptr(None), M, C, _p(gg), _p(gmean), _p(ginv), _p(gdg), _p(gdb), int(relu),
         _p(gws), int(dres_mode == "accumulated"))
    NH.assert_contained(what, [gdy, gx, gg, gmean, ginv] + ([gmask] if relu else []),
                        [gdx] + ([gdres] if dres_mode == "written" else []))
    for g_ in [gdg, gdb, gws] + ([gdres] if gdres else []):
        assert g_.guards_intact(), what + ": wrote outside a buffer"
    return dict(dx=gdx.t, dres=gdres.t if gdres else None, dgamma=gdg.t, dbeta=gdb.t)


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("device", DEVICES)
def test_train_forward(device, relu, with_res):
    """y, the saved mean / invstd, the moving statistics from non-trivial starting values (the unbiased factor is
    5/4 at M = 5 and absent at M = 1) and every ReLU mask bit."""
    device = _device(device)
    for M, C in SHAPES:
        what = "%s/fwd_train relu=%d res=%d (%d,%d)" % (device, relu, with_res, M, C)
        c = BH.bn_case(M, C, 1200 + 7 * M + C)
        st = BH.stats_of(c["x"], _k(device, M, C))
        o = _train_autograd(device, c, relu, with_res)
        _check_fwd(what, device, c, st, relu, with_res, o["y"], o["mm"], o["mv"], o["mean"], o["invstd"], o["mask"])
        if device == "cuda":
            r = _train_raw_fwd(what + " raw", c, relu, with_res)
            _check_fwd(what + " raw", device, c, st, relu, with_res, r["y"], r["mm"], r["mv"], r["mean"], r["invstd"],
                       r["mask"])
            assert NH.bits_equal(r["y"], o["y"]) and NH.bits_equal(r["mv"], o["mv"])


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("device", DEVICES)
def test_train_backward(device, relu, with_res):
    """dx, dres (absent, written, accumulated onto a non-zero tensor) and dgamma / dbeta accumulated onto non-zero
    slots.  On ``cpu`` the sums get k = M + 4: M terms in any order and up to 4 roundings inside a term."""
    device = _device(device)
    for M, C in SHAPES:
        what = "%s/bwd relu=%d res=%d (%d,%d)" % (device, relu, with_res, M, C)
        c = BH.bn_case(M, C, 1200 + 7 * M + C)
        k = _k(device, M, C)
        st = BH.stats_of(c["x"], k)
        pre, acc = BH.fwd_ref(c["x"], st, c["g"], c["b"], c["res"] if with_res else None)
        kb = M + 4 if device == "cpu" else k
        for accum in ([False, True] if with_res else [False]):
            o = _train_autograd(device, c, relu, with_res, accum)
            pos = BH.relu_sign(pre, acc, o["y"].float().cpu() > 0, what)[0] if relu else None
            _check_bwd(what + " accum=%d" % accum, device, c, st, pos, kb, o["dx"], o["dres"], o["dgamma"],
                       o["dbeta"], accum)
        if device == "cuda":
            pos = (pre > 0) if relu else None
            for mode in (["absent", "written", "accumulated"] if with_res else ["absent"]):
                r = _train_raw_bwd("%s raw dres %s" % (what, mode), c, st, pos, mode)
                _check_bwd("%s raw dres %s" % (what, mode), device, c, BH.handed_stats(st), pos, kb, r["dx"],
                           r["dres"], r["dgamma"], r["dbeta"], mode == "accumulated")


@pytest.mark.parametrize("device", GPU_ONLY)
def test_train_eps_1e5(device):
    """The planted channels at the eps of the ResNet path: the constant channel's invstd is 316 and ten times as
    sensitive to an error of its variance.  ReLU and residual; forward (autograd and entry point) and backward."""
    device = _device(device)
    eps = 1e-5
    for M, C in SHAPES:
        what = "cuda/eps=1e-5 (%d,%d)" % (M, C)
        c = BH.bn_case(M, C, 1200 + 7 * M + C)
        k = _k(device, M, C)
        st = BH.stats_of(c["x"], k, BH.f32(eps))
        o = _train_autograd(device, c, True, True, eps=eps)
        _, _, pos = _check_fwd(what, device, c, st, True, True, o["y"], o["mm"], o["mv"], o["mean"], o["invstd"],
                               o["mask"])
        _check_bwd(what, device, c, st, pos, k, o["dx"], o["dres"], o["dgamma"], o["dbeta"])
        r = _train_raw_fwd(what + " raw", c, True, True, eps=eps)
        _check_fwd(what + " raw", device, c, st, True, True, r["y"], r["mm"], r["mv"], r["mean"], r["invstd"],
                   r["mask"])


# ============================================================================================ partial statistics
PM, PC = 300, 24


def _partials_case(P, seed):
    c = BH.bn_case(PM, PC, seed)
    x = c["x"].double()
    ps, S, aS = BH.split_partials(x, P, seed + 20)
    pq, Q, aQ = BH.split_partials(x * x, P, seed + 21)
    st = BH.stats_ref(S, Q, aS, aQ, PM, BH.fin_adds(P))              # k: only the finalize's fp32 adds
    return c, ps, pq, st


@pytest.mark.parametrize("P", P_LIST)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_fwd_stats_from_partials(device, P):
    """mdtf_bn_fwd_stats on hand-made partial rows (a buffer taller than P): the oracle sums the fp32 partials
    exactly, so the bound holds only the finalize's fp32 additions; the rows are re-zeroed, the rest untouched."""
    device = _device(device)
    M, C = PM, PC
    c, ps, pq, st = _partials_case(P, 2000 + P)
    what = "cuda/fwd_stats P=%d" % P
    gx, gres, gg, gb = G(c["x"].bfloat16()), G(c["res"].bfloat16()), G(c["g"]), G(c["b"])
    gmm, gmv, gps, gpq = G(c["mm0"]), G(c["mv0"]), G(ps), G(pq)
    gy, gmask = G(None, torch.bfloat16, (M, C)), G(None, torch.uint8, (M * C // 8,))
    gmean, ginv, gws = G(None, torch.float32, (C,)), G(None, torch.float32, (C,)), G(None, torch.float32, (2 * C,))
    _raw("mdtf_bn_fwd_stats", _p(gx), _p(gres), _p(gy), _p(gmask), M, C, _p(gg), _p(gb), _p(gmm), _p(gmv),
         BH.f32(DECAY), BH.f32(EPS), 1, _p(gmean), _p(ginv), _p(gps), _p(gpq), P, _p(gws))
    NH.assert_contained(what, [gx, gres, gg, gb], [gy, gmean, ginv, gws])
    for g_ in (gmm, gmv, gmask):
        assert g_.guards_intact(), what
    _zeroed_head(what + " psum", gps, ps, P)
    _zeroed_head(what + " psq", gpq, pq, P)
    _check_fwd(what, device, c, st, True, True, gy.t, gmm.t, gmv.t, gmean.t, ginv.t, gmask.t)


@pytest.mark.parametrize("P", P_LIST)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_fwd_coeffs_then_apply_ss(device, P):
    """mdtf_bn_fwd_coeffs (scale | shift into ws, statistics, moving statistics, partials re-zeroed) and the apply
    from those coefficients."""
    device = _device(device)
    M, C = PM, PC
    c, ps, pq, st = _partials_case(P, 2100 + P)
    what = "cuda/fwd_coeffs P=%d" % P
    gg, gb, gmm, gmv, gps, gpq = G(c["g"]), G(c["b"]), G(c["mm0"]), G(c["mv0"]), G(ps), G(pq)
    gmean, ginv, gws = G(None, torch.float32, (C,)), G(None, torch.float32, (C,)), G(None, torch.float32, (2 * C,))
    _raw("mdtf_bn_fwd_coeffs", M, C, _p(gg), _p(gb), _p(gmm), _p(gmv), BH.f32(DECAY), BH.f32(EPS), _p(gmean),
         _p(ginv), _p(gps), _p(gpq), P, _p(gws))
    NH.assert_contained(what, [gg, gb], [gmean, ginv, gws])
    _zeroed_head(what + " psum", gps, ps, P)
    _zeroed_head(what + " psq", gpq, pq, P)
    g64, b64 = c["g"].double(), c["b"].double()
    scale = g64 * st.inv
    # scale: the error of invstd and one product; shift = beta - mean gamma invstd: the errors of mean and invstd and
    # k = 3 roundings (two products, the subtraction)
    NH.check_bound(gws.t[:C], scale, g64.abs() * st.einv + U * g64.abs() * st.inv_hi + TINY, what + " scale")
    NH.check_bound(gws.t[C:], b64 - st.mean * scale,
                   g64.abs() * (st.inv_hi * st.emf + st.mean.abs() * st.einv)
                   + gamma(3) * (b64.abs() + g64.abs() * st.inv_hi * st.mu_hi) + TINY, what + " shift")
    gx, gss = G(c["x"].bfloat16()), G(gws.t)
    gy, gmask = G(None, torch.bfloat16, (M, C)), G(None, torch.uint8, (M * C // 8,))
    _raw("mdtf_bn_apply_ss", _p(gx), _p(gy), _p(gmask), M, C, _p(gss), 1)
    NH.assert_contained(what + " apply", [gx, gss], [gy])
    assert gmask.guards_intact()
    _check_fwd(what + " apply", device, c, st, True, False, gy.t, gmm.t, gmv.t, gmean.t, ginv.t, gmask.t)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_apply_ss_exact_zero(device, relu):
    """scale a power of two and shift = -scale x0: x scale is exact, so the planted x = x0 have pre-activation
    exactly 0 (output +0, mask bit 0) and every other element carries the one rounding of the add.  Without ReLU no
    mask byte is written."""
    device = _device(device)
    for M, C in [(5, 8), (37, 24), (129, 64)]:
        what = "cuda/apply_ss exact relu=%d (%d,%d)" % (relu, M, C)
        x = NH.randn((M, C), 2200 + M + C, 2.0)
        x0 = NH.randn((C,), 2201 + C)
        scale = torch.tensor([2.0 ** ((i % 5) - 2) * (-1.0 if i % 3 == 1 else 1.0) for i in range(C)])
        planted = torch.zeros((M, C), dtype=torch.bool)
        planted.view(-1)[::7] = True
        x = torch.where(planted, x0.expand(M, C), x)
        ss = torch.cat([scale, -scale * x0])
        gx, gss = G(x.bfloat16()), G(ss)
        gy, gmask = G(None, torch.bfloat16, (M, C)), G(None, torch.uint8, (M * C // 8,))
        _raw("mdtf_bn_apply_ss", _p(gx), _p(gy), _p(gmask), M, C, _p(gss), relu)
        NH.assert_contained(what, [gx, gss], [gy])
        pre = scale.double() * (x.double() - x0.double())
        ref = torch.relu(pre) if relu else pre
        NH.check_bound(gy.t, ref, NH.out_bound(ref, gamma(1) * pre.abs(), True), what + " y")      # k = 1: the add
        assert not bool(gy.t.cpu().view(torch.int16)[planted].any()), what + ": a planted element is not +0"
        if relu:
            assert gmask.guards_intact()
            assert torch.equal(BH.unpack_mask(gmask.t, pre.shape), pre > 0), what + ": mask bits"
        else:
            assert gmask.unchanged(), what + ": mask written without ReLU"


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("device", DEVICES)
def test_eval_forward(device, relu):
    """Inference: y from the moving statistics, which stay bitwise unchanged."""
    device = _device(device)
    for M, C in [(5, 8), (37, 24), (129, 64), (5, 2056)]:
        for with_res in (False, True):
            what = "%s/fwd_eval relu=%d res=%d (%d,%d)" % (device, relu, with_res, M, C)
            c = BH.bn_case(M, C, 2300 + M + C)
            st = BH.given_stats(c["mm0"], c["mv0"], BH.f32(EPS))
            mm, mv = c["mm0"].to(device).clone(), c["mv0"].to(device).clone()
            y = ops.batch_norm(NH.put(c["x"], device), c["g"].to(device), c["b"].to(device), mm, mv, False, DECAY,
                               EPS, relu, NH.put(c["res"], device) if with_res else None)
            assert NH.bits_equal(mm.cpu(), c["mm0"]) and NH.bits_equal(mv.cpu(), c["mv0"])
            _check_fwd(what, device, c, st, relu, with_res, y, None, None)
            if device == "cuda":
                gx, gres, gg, gb = G(c["x"].bfloat16()), G(c["res"].bfloat16()), G(c["g"]), G(c["b"])
                gmm, gmv = G(c["mm0"]), G(c["mv0"])
                gy, gws = G(None, torch.bfloat16, (M, C)), G(None, torch.float32, (2 * C,))
                _raw("mdtf_bn_fwd_eval", _p(gx), _p(gres) if with_res else _native.ptr(None), _p(gy), M, C, _p(gg),
                     _p(gb), _p(gmm), _p(gmv), BH.f32(EPS), int(relu), _p(gws))
                NH.assert_contained(what + " raw", [gx, gres, gg, gb, gmm, gmv], [gy, gws])
                _check_fwd(what + " raw", device, c, st, relu, with_res, gy.t, None, None)
                assert NH.bits_equal(gy.t, y)


@pytest.mark.parametrize("P", P_LIST)
@pytest.mark.parametrize("device", GPU_ONLY)
def test_bwd_stats_from_partials(device, P):
    """mdtf_bn_bwd_stats on hand-made sum dz / sum dz x partial rows, and the early finalize
    (mdtf_bn_bwd_finalize_ws: k1 | k2 | k3 | dgamma | dbeta WRITTEN over a pre-filled workspace) with its
    input-gradient pass (mdtf_bn_dx_ws: the slots receive exactly one addition of the workspace's dgamma / dbeta)."""
    device = _device(device)
    M, C = PM, PC
    c = BH.bn_case(M, C, 2400 + P)
    st = BH.stats_of(c["x"], _k(device, M, C))
    pre, _ = BH.fwd_ref(c["x"], st, c["g"], c["b"], c["res"])
    pos = pre > 0
    dz = c["dy"].double() * pos
    ps, S, aS = BH.split_partials(dz, P, 2450 + P)
    pq, Q, aQ = BH.split_partials(dz * c["x"].double(), P, 2451 + P)
    sums, k = (S, Q, aS, aQ), BH.fin_adds(P)
    hs = BH.handed_stats(st)                 # the kernels get the oracle's mean / invstd: one cast each
    what = "cuda/bwd_stats P=%d" % P

    def bufs():
        return dict(dy=G(c["dy"].bfloat16()), x=G(c["x"].bfloat16()), mask=G(BH.pack_mask(pos)), g=G(c["g"]),
                    mean=G(st.mean.float()), inv=G(st.inv.float()), dx=G(None, torch.bfloat16, (M, C)),
                    dres=G(None, torch.bfloat16, (M, C)), dg=G(c["dg0"]), db=G(c["db0"]), ps=G(ps), pq=G(pq))

    def contained(w, b, extra_in=()):
        NH.assert_contained(w, [b[n] for n in ("dy", "x", "mask", "g", "mean", "inv")] + list(extra_in),
                            [b["dx"], b["dres"]])
        assert b["dg"].guards_intact() and b["db"].guards_intact(), w
        _zeroed_head(w + " psum", b["ps"], ps, P)
        _zeroed_head(w + " psq", b["pq"], pq, P)

    b = bufs()
    gws = G(None, torch.float32, (3 * C,))
    _raw("mdtf_bn_bwd_stats", _p(b["dy"]), _p(b["x"]), _p(b["mask"]), _p(b["dx"]), _p(b["dres"]), M, C, _p(b["g"]),
         _p(b["mean"]), _p(b["inv"]), _p(b["dg"]), _p(b["db"]), 1, _p(b["ps"]), _p(b["pq"]), P, _p(gws), 0)
    contained(what, b)
    assert gws.guards_intact() and gws.all_written()
    _check_bwd(what, device, c, hs, pos, k, b["dx"].t, b["dres"].t, b["dg"].t, b["db"].t, sums=sums)

    what = "cuda/bwd_finalize_ws P=%d" % P
    b = bufs()
    gws = G(NH.randn((5 * C,), 2460 + P, 100.0))                            # garbage the finalize must overwrite
    _raw("mdtf_bn_bwd_finalize_ws", M, C, _p(b["g"]), _p(b["mean"]), _p(b["inv"]), _p(b["ps"]), _p(b["pq"]), P,
         _p(gws))
    assert gws.guards_intact()
    _zeroed_head(what + " psum", b["ps"], ps, P)
    _zeroed_head(what + " psq", b["pq"], pq, P)
    r = BH.bwd_ref(c["x"], c["dy"], pos, hs, c["g"], k, sums=sums)
    NH.check_bound(gws.t[3 * C:4 * C], r["dg"], r["edg"], what + " ws dgamma")
    NH.check_bound(gws.t[4 * C:], r["db"], r["edb"], what + " ws dbeta")
    ws_after = G(gws.t)
    _raw("mdtf_bn_dx_ws", _p(b["dy"]), _p(b["x"]), _p(b["mask"]), _p(b["dx"]), _p(b["dres"]), M, C, _p(ws_after),
         _p(b["dg"]), _p(b["db"]), 1, 0)
    contained(what + " dx_ws", b, [ws_after])
    fin = ws_after.t.cpu()
    assert NH.bits_equal(b["dg"].t.cpu(), c["dg0"] + fin[3 * C:4 * C]), what + ": dgamma slot != slot + ws"
    assert NH.bits_equal(b["db"].t.cpu(), c["db0"] + fin[4 * C:]), what + ": dbeta slot != slot + ws"
    _check_bwd(what + " dx_ws", device, c, hs, pos, k, b["dx"].t, b["dres"].t, b["dg"].t, b["db"].t, sums=sums)


# ============================================================================================================ dual
def _dual_case(M, C, seed):
    c = BH.bn_case(M, C, seed)
    c2 = BH.bn_case(M, C, seed + 50)
    c2["x"] = BH.plant(NH.bf16_exact(NH.randn((M, C), seed + 51, 0.7) - 0.2), seed + 52)
    c2["dy"] = c["dy"]
    return c, c2


def _dual_fwd_check(what, device, c, c2, st, st2, y, mms, means=None, mask=None):
    bf = device == "cuda"
    pre1, acc1 = BH.fwd_ref(c["x"], st, c["g"], c["b"])
    pre2, acc2 = BH.fwd_ref(c2["x"], st2, c2["g"], c2["b"])
    pre = pre1 + pre2
    acc = acc1 + acc2 + U * (pre.abs() + acc1 + acc2)                        # the add of the two normalisations
    ypos = y.detach().float().cpu() > 0
    got = BH.unpack_mask(mask, pre.shape) if mask is not None else ypos
    pos, _ = BH.relu_sign(pre, acc, got, what)
    if mask is not None:
        assert torch.equal(got, pos) and torch.equal(got, ypos), what + ": mask bits"
    yref = torch.where(pos, pre, torch.zeros_like(pre))
    NH.check_bound(y, yref, NH.out_bound(yref, acc, bf), what + " y")
    for (cc, s_, tag), (mm, mv) in zip(((c, st, ""), (c2, st2, "2")), mms):
        mmr, emm, mvr, emv = BH.moving_ref(s_, cc["mm0"], cc["mv0"], BH.f32(DECAY), _one_minus(device))
        NH.check_bound(mm, mmr, emm, what + " mmean" + tag)
        NH.check_bound(mv, mvr, emv, what + " mvar" + tag)
    if means is not None:
        for s_, (mean, inv), tag in zip((st, st2), means, ("", "2")):
            NH.check_bound(mean, s_.mean, s_.emf + TINY, what + " mean" + tag)
            NH.check_bound(inv, s_.inv, s_.einv + TINY, what + " invstd" + tag)
    return pos


def _dual_bwd_check(what, device, c, c2, st, st2, pos, k, k2, dx, dr, grads, sums=None):
    bf = device == "cuda"
    r1 = BH.bwd_ref(c["x"], c["dy"], pos, st, c["g"], k, sums=sums, dg0=c["dg0"], db0=c["db0"], bf=bf)
    r2 = BH.bwd_ref(c2["x"], c["dy"], pos, st2, c2["g"], k2, dg0=c2["dg0"], db0=c2["db0"], bf=bf)
    NH.check_bound(dx, r1["dx"], r1["dx_bound"], what + " dx")
    NH.check_bound(dr, r2["dx"], r2["dx_bound"], what + " dr")
    for got, r, n in zip(grads, (r1, r1, r2, r2), ("dgamma", "dbeta", "dgamma", "dbeta")):
        NH.check_bound(got, r[n], r[n + "_bound"], "%s %s%s" % (what, n, "2" if r is r2 else ""))


def _sum_partials(x2, P):
    """[P][C] partial sums as a conv epilogue would emit them, and the statistics the oracle takes from them."""
    x = x2.double()
    ps, S, aS = BH.split_partials(x, P, 77, extra=0)
    pq, Q, aQ = BH.split_partials(x * x, P, 78, extra=0)
    return ps, pq, BH.stats_ref(S, Q, aS, aQ, x.shape[0], BH.fin_adds(P))


@pytest.mark.parametrize("device,path", [pytest.param("cpu", "fused")] + [
    pytest.param("cuda", p, marks=pytest.mark.gpu) for p in ("fused", "two_pass", "two_pass_dz")])
def test_dual(device, path, monkeypatch):
    """relu(BN(x) + BN2(r)): y, both moving-statistics pairs, dx, dr and the four parameter gradients onto non-zero
    slots; on the GPU through _BNTrainDual with the one-pass backward or the two-pass paths."""
    device = _device(device)
    from mdtf.ops import bn as B
    monkeypatch.setattr(B, "DUAL_FUSED", path == "fused")
    monkeypatch.setattr(B, "DUAL_DZ", path == "two_pass_dz")
    for M, C in [(37, 24), (523, 64)]:
        what = "%s/dual %s (%d,%d)" % (device, path, M, C)
        c, c2 = _dual_case(M, C, 3000 + M + C)
        x = NH.put(c["x"], device).requires_grad_(True)
        r = NH.put(c2["x"], device).requires_grad_(True)
        ps = [_param(c["g"], c["dg0"], device), _param(c["b"], c["db0"], device),
              _param(c2["g"], c2["dg0"], device), _param(c2["b"], c2["db0"], device)]
        mms = [[cc["mm0"].to(device).clone(), cc["mv0"].to(device).clone()] for cc in (c, c2)]
        if device == "cuda":
            p1, q1, st = _sum_partials(c["x"], 3)
            p2, q2, st2 = _sum_partials(c2["x"], 1)
            parts = [t.cuda() for t in (p1, q1, p2, q2)]
            y = B._BNTrainDual.apply(x, ps[0][0], ps[1][0], mms[0][0], mms[0][1], r, ps[2][0], ps[3][0], mms[1][0],
                                     mms[1][1], DECAY, EPS, (parts[0], parts[1], 3), (parts[2], parts[3], 1))
            assert not any(bool(t.any()) for t in parts), what + ": partial rows not re-zeroed"
            sv = y.grad_fn.saved_tensors             # x, mask, gamma, mean, invstd, r, gamma2, mean2, invstd2
            saved = dict(means=[(sv[3], sv[4]), (sv[7], sv[8])], mask=sv[1])
            kb = _k(device, M, C)
        else:
            st, st2 = BH.stats_of(c["x"], M), BH.stats_of(c2["x"], M)
            sc = ops.batch_norm(r, ps[2][0], ps[3][0], mms[1][0], mms[1][1], True, DECAY, EPS, False, None)
            y = ops.batch_norm(x, ps[0][0], ps[1][0], mms[0][0], mms[0][1], True, DECAY, EPS, True, sc)
            kb = M + 4
            saved = dict(means=None, mask=None)
        pos = _dual_fwd_check(what, device, c, c2, st, st2, y.detach(), mms, saved["means"], saved["mask"])
        y.backward(NH.put(c["dy"], device))
        grads = [s for _, s in ps] if device == "cuda" else [t.grad for t, _ in ps]
        _dual_bwd_check(what, device, c, c2, st, st2, pos, kb, kb, x.grad, r.grad, grads)


@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_dual_entry_points(device, P):
    """mdtf_bn_fwd_dual (y, mask, both saved statistics, all four moving statistics, both partial buffers re-zeroed)
    and mdtf_bn_bwd_dual with its own reduction (P = 0) or the main BN's sums handed in (P > 0, re-zeroed)."""
    device = _device(device)
    for M, C in [(37, 24), (523, 64)]:
        what = "cuda/dual raw P=%d (%d,%d)" % (P, M, C)
        c, c2 = _dual_case(M, C, 3100 + M + C)
        P1, P2 = 131, 2
        x64, r64 = c["x"].double(), c2["x"].double()
        ps1, S1, a1 = BH.split_partials(x64, P1, 31)
        pq1, Q1, b1 = BH.split_partials(x64 * x64, P1, 32)
        ps2, S2, a2 = BH.split_partials(r64, P2, 33)
        pq2, Q2, b2 = BH.split_partials(r64 * r64, P2, 34)
        st = BH.stats_ref(S1, Q1, a1, b1, M, BH.fin_adds(P1))
        st2 = BH.stats_ref(S2, Q2, a2, b2, M, BH.fin_adds(P2))
        gx, gr = G(c["x"].bfloat16()), G(c2["x"].bfloat16())
        gy, gmask = G(None, torch.bfloat16, (M, C)), G(None, torch.uint8, (M * C // 8,))
        prm = [G(cc[n]) for cc in (c, c2) for n in ("g", "b")]
        mov = [G(cc[n]) for cc in (c, c2) for n in ("mm0", "mv0")]
        sav = [G(None, torch.float32, (C,)) for _ in range(4)]
        gp = [G(t) for t in (ps1, pq1, ps2, pq2)]
        gws = G(None, torch.float32, (4 * C,))
        _raw("mdtf_bn_fwd_dual", _p(gx), _p(gr), _p(gy), _p(gmask), M, C, _p(prm[0]), _p(prm[1]), _p(mov[0]),
             _p(mov[1]), _p(gp[0]), _p(gp[1]), P1, _p(sav[0]), _p(sav[1]), _p(prm[2]), _p(prm[3]), _p(mov[2]),
             _p(mov[3]), _p(gp[2]), _p(gp[3]), P2, _p(sav[2]), _p(sav[3]), BH.f32(DECAY), BH.f32(EPS), _p(gws))
        NH.assert_contained(what + " fwd", [gx, gr] + prm, [gy, gws] + sav)
        assert gmask.guards_intact() and all(m.guards_intact() for m in mov)
        for g_, t0, p_ in zip(gp, (ps1, pq1, ps2, pq2), (P1, P1, P2, P2)):
            _zeroed_head(what + " partials", g_, t0, p_)
        pos = _dual_fwd_check(what + " fwd", device, c, c2, st, st2, gy.t, [[mov[0].t, mov[1].t], [mov[2].t, mov[3].t]],
                              [(sav[0].t, sav[1].t), (sav[2].t, sav[3].t)], gmask.t)
        # backward, from the oracle's mask and statistics
        dz = c["dy"].double() * pos
        pz, Sz, az = BH.split_partials(dz, max(P, 1), 35)
        pzx, Szx, azx = BH.split_partials(dz * x64, max(P, 1), 36)
        gdy, gm = G(c["dy"].bfloat16()), G(BH.pack_mask(pos))
        stat = [G(t.float()) for t in (st.mean, st.inv, st2.mean, st2.inv)]
        gdx, gdr = G(None, torch.bfloat16, (M, C)), G(None, torch.bfloat16, (M, C))
        slots = [G(cc[n]) for cc in (c, c2) for n in ("dg0", "db0")]
        gpz, gpzx = G(pz), G(pzx)
        gws = G(None, torch.float32, (2 * _ws_floats(M, C),))
        _raw("mdtf_bn_bwd_dual", _p(gdy), _p(gx), _p(gr), _p(gm), _p(gdx), _p(gdr), M, C, _p(prm[0]), _p(stat[0]),
             _p(stat[1]), _p(slots[0]), _p(slots[1]), _p(gpz), _p(gpzx), P, _p(prm[2]), _p(stat[2]), _p(stat[3]),
             _p(slots[2]), _p(slots[3]), _p(gws))
        NH.assert_contained(what + " bwd", [gdy, gx, gr, gm, prm[0], prm[2]] + stat, [gdx, gdr])
        assert gws.guards_intact() and all(s.guards_intact() for s in slots)
        kr = _k(device, M, C)
        if P:
            _zeroed_head(what + " bwd psum", gpz, pz, P)
            _zeroed_head(what + " bwd psq", gpzx, pzx, P)
        else:
            assert gpz.unchanged() and gpzx.unchanged(), what + ": partials touched at P = 0"
        _dual_bwd_check(what + " bwd", device, c, c2, BH.handed_stats(st), BH.handed_stats(st2), pos,
                        BH.fin_adds(P) if P else kr, kr, gdx.t, gdr.t,
                        [s.t for s in slots], sums=(Sz, Szx, az, azx) if P else None)


# ============================================================================================================ stem
# (name, (H, W), k, s, padding)
STEM_GEO = [("k3s2same_15x13", (15, 13), 3, 2, "SAME"),       # odd sizes, padded borders
            ("k3s1valid_9x8", (9, 8), 3, 1, "VALID"),         # up to 9 windows over a pixel: the general gather
            ("k2s2_8x8", (8, 8), 2, 2, "SAME")]
STEM_N = 2
CH_NEGWIN, CH_DUP = 5, 6


def _stem_case(hw, C, k, s, padding, seed):
    """x NHWC with the planted channels of ``bn_case`` and: channel 5 (gamma 1, beta -0.5) at -4 over the whole
    window (1, 1) of image 0: everything there is rectified to zero; channel 6 (gamma 1) clamped to <= 4 with two taps
    of window (2, 2) at 6: one window, two exactly equal maxima."""
    H, W = hw
    M = STEM_N * H * W
    x = BH.plant(NH.bf16_exact(NH.randn((M, C), seed, 2.0) + 0.5), seed + 1)
    x[:, BH.CH_BIG] = NH.bf16_exact(NH.randn((M,), seed + 3, 2.0) + 0.5)     # no large-mean channel here
    x = x.reshape(STEM_N, H, W, C)
    g, b = BH.params(C, seed + 2)
    g[CH_NEGWIN], b[CH_NEGWIN], g[CH_DUP] = 1.0, -0.5, 1.0
    oh_n, ow_n, pt, pl = NH.pool_geometry(H, W, (k, k), (s, s), padding)
    x[:, :, :, CH_DUP] = x[:, :, :, CH_DUP].clamp(max=4.0)
    for kh in range(k):
        for kw in range(k):
            ih, iw = 1 * s - pt + kh, 1 * s - pl + kw
            if 0 <= ih < H and 0 <= iw < W:
                x[0, ih, iw, CH_NEGWIN] = -4.0
    h0, w0 = 2 * s - pt, 2 * s - pl
    x[0, h0, w0 + 1, CH_DUP] = 6.0
    x[0, h0 + 1, w0, CH_DUP] = 6.0
    dup = (2, 2, 0 * k + 1)                                     # the window and the tap that must win
    dy = NH.randn((STEM_N, oh_n, ow_n, C), seed + 5)
    return dict(x=x.reshape(M, C), x4=x, g=g, b=b, dy4=dy, mm0=NH.randn((C,), seed + 6, 0.5),
                mv0=BH._rand((C,), seed + 7) + 0.5, dg0=NH.randn((C,), seed + 9, 3.0),
                db0=NH.randn((C,), seed + 10, 3.0), geo=(oh_n, ow_n, k, k, s, s, pt, pl), dup=dup, res=None)


def _stem_k(pooled, hw, C, geo):
    """fp32 additions of the stem backward's two sums on the GPU, per variant: the pooled-output reduction has the
    statistics kernels' geometry over the N OH OW pooled rows, the generic input reduction over the N H W input rows,
    the input-row reduction (C / 8 a power of two) its own order (``bn_helpers.rows_k``)."""
    H, W = hw
    M, Mp, cv = STEM_N * H * W, STEM_N * geo[0] * geo[1], C // 8
    if pooled:
        return _k("cuda", Mp, C)
    if cv & (cv - 1) == 0:
        return min(BH.rows_k(STEM_N * H, W, C, _ws_floats(M, C)), M - 1)
    return _k("cuda", M, C)


def _stem_check(what, device, c, st, k, s, padding, y, arg, dx, dgamma, dbeta, mm, mv, mean=None, invstd=None,
                pooled_stats=False, k_sum=None):
    bf = device == "cuda"
    x4 = c["x4"]
    n, h, w, C = x4.shape
    pre, acc = BH.fwd_ref(c["x"], st, c["g"], c["b"])
    und = pre.abs() <= acc
    assert int(und.sum()) <= BH.CAP * und.numel(), what + ": undetermined ReLU signs"
    z = torch.relu(pre).reshape(x4.shape)
    # equal keys <=> bit-identical values in the kernel: rectified to zero for certain, the same x, or gamma = 0
    key = torch.where(pre < -acc, torch.full_like(pre, -BH.BIG), c["x"].double() * (c["g"].double() != 0))
    f = BH.stem_pool_ref(z, acc.reshape(x4.shape), key.reshape(x4.shape), (k, k), (s, s), padding, arg, bf)
    n_amb = int(f["amb"].sum())
    print("BN_AMBIG %-58s %d of %d windows ambiguous" % (what, n_amb, f["amb"].numel()))
    assert n_amb <= BH.CAP * f["amb"].numel(), what + ": ambiguous windows"
    oh, ow, tap = c["dup"]
    assert not bool(f["amb"][0, oh, ow, CH_DUP]) and int(f["first"][0, oh, ow, CH_DUP]) == tap
    assert not bool(f["amb"][0, 1, 1, CH_NEGWIN]) and float(f["y"][0, 1, 1, CH_NEGWIN].detach()) == 0.0
    NH.check_bound(y, f["y"], f["y_bound"], what + " y")
    if arg is not None:
        a = arg.cpu().to(torch.int64)
        bad = (a != f["first"]) & ~f["amb"]
        assert not bool(bad.any()), "%s: %d argmax bytes wrong" % (what, int(bad.sum()))
        assert bool(f["ingot"][f["amb"]].all()), what + ": an ambiguous window's tap is not near-maximal"
    if mm is not None:
        mmr, emm, mvr, emv = BH.moving_ref(st, c["mm0"], c["mv0"], BH.f32(DECAY), _one_minus(device))
        NH.check_bound(mm, mmr, emm, what + " mmean")
        NH.check_bound(mv, mvr, emv, what + " mvar")
    if mean is not None:
        NH.check_bound(mean, st.mean, st.emf + TINY, what + " mean")
        NH.check_bound(invstd, st.inv, st.einv + TINY, what + " invstd")
    # backward: dy of every window to its tap (a sum of up to nwin fp32 terms per pixel), masked by [pre > 0]; an
    # undetermined sign under a non-zero gradient is charged to the bound in full
    dy64 = c["dy4"].double()
    gq, sabs, nwin = NH.pool_bwd_ref(dy64, f, x4.shape, (k, k), (s, s), True)
    gq, sabs = gq.reshape(pre.shape), sabs.reshape(pre.shape)
    pos = pre > 0
    e_dz = gamma(int(nwin.max())) * sabs * pos + sabs * und                 # k = windows over a pixel
    xSx = 0.0
    if pooled_stats:
        # x rebuilt from the bf16 pooled output as (y - shift) / scale: half a bf16 ulp of y and 8 roundings over
        # |y| + |shift|, divided by |scale|; channels with |scale| < |shift| invstd / 8 gather x itself (exact)
        g64 = c["g"].double()
        sc, sc_lo = g64.abs() * st.inv, g64.abs() * (st.inv - st.einv)
        sh = (c["b"].double() - st.mean * g64 * st.inv).abs()
        gathered = sc < 0.125 * sh * st.inv * (1.0 - 1e-3)
        yv = f["y"] + f["y_bound"]
        rec = (NH.half_ulp_bf16(yv) + gamma(8) * (yv + sh)) / sc_lo.clamp(min=TINY)
        rec = torch.where(gathered.expand_as(rec), torch.zeros_like(rec), rec)
        xSx = (dy64.abs() * (f["y"] > 0) * rec).reshape(-1, C).sum(0)
    M = pre.shape[0]
    # cpu: k = M + 8, M terms in any order; cuda: the variant's own count (_stem_k).  The terms of the sums are the
    # windows' gradients (the pooled reduction never forms the per-pixel totals): their magnitudes, not the totals'
    dz, x64 = gq * pos, c["x"].double()
    sums = (dz.sum(0), (dz * x64).sum(0), (sabs * pos).sum(0), (sabs * pos * x64.abs()).sum(0))
    r = BH.bwd_ref(c["x"], None, None, st, c["g"], M + 8 if k_sum is None else k_sum, sums=sums, dg0=c["dg0"],
                   db0=c["db0"], bf=bf, e_dz=e_dz, xSx=xSx, dz=dz)
    planted = x4[0, :, :, CH_NEGWIN] == -4.0                                # the window rectified to zero: no gradient
    assert not bool(r["dz"].reshape(x4.shape)[0, :, :, CH_NEGWIN][planted].any()), what
    NH.check_bound(dx, r["dx"], r["dx_bound"], what + " dx")
    NH.check_bound(dgamma, r["dgamma"], r["dgamma_bound"], what + " dgamma")
    NH.check_bound(dbeta, r["dbeta"], r["dbeta_bound"], what + " dbeta")


@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("geo", STEM_GEO, ids=[g[0] for g in STEM_GEO])
@pytest.mark.parametrize("device", DEVICES)
def test_stem(device, geo, C, monkeypatch):
    """maxpool(relu(BN(x))): the pooled y, every argmax byte, the statistics outputs, dx of every input pixel and
    dgamma / dbeta; on the GPU with the pooled-output statistics (y given) and the input-row statistics (y null), the
    row-pair input-gradient kernel on and off, through autograd and the entry points."""
    device = _device(device)
    _, hw, k, s, padding = geo
    c = _stem_case(hw, C, k, s, padding, 4000 + 10 * hw[0] + C)
    M = c["x"].shape[0]
    what = "%s/stem %s C=%d" % (device, geo[0], C)
    if device == "cpu":
        st = BH.stats_of(c["x"], M)
        x = c["x4"].clone().requires_grad_(True)
        g, _ = _param(c["g"], c["dg0"], device)
        b, _ = _param(c["b"], c["db0"], device)
        mm, mv = c["mm0"].clone(), c["mv0"].clone()
        y = ops.max_pool(ops.batch_norm(x, g, b, mm, mv, True, DECAY, EPS, True, None), k, s, padding)
        y.backward(c["dy4"])
        _stem_check(what, device, c, st, k, s, padding, y.detach(), None, x.grad.reshape(M, C), g.grad, b.grad, mm, mv)
        return
    from mdtf.ops import bn as B
    _native.register("mdtf_bn_pool_dx_pairs", [_native.I], restype=None)
    N_, (H, W) = STEM_N, hw
    oh_n, ow_n = c["geo"][0], c["geo"][1]
    ps, pq, st = _sum_partials(c["x"], 3)
    try:
        for pairs in (1, 0):
            _native.fn("mdtf_bn_pool_dx_pairs")(pairs)
            for pooled in (True, False):
                w2 = "%s pairs=%d ystats=%d" % (what, pairs, pooled)
                # autograd
                monkeypatch.setattr(B, "STEM_POOLED_STATS", pooled)
                x = c["x4"].cuda().bfloat16().requires_grad_(True)
                (g, gs), (b, bs) = _param(c["g"], c["dg0"], device), _param(c["b"], c["db0"], device)
                mm, mv = c["mm0"].cuda(), c["mv0"].cuda()
                y = B.bn_relu_maxpool_nhwc(x, g, b, mm, mv, DECAY, EPS, (ps.cuda(), pq.cuda(), 3), c["geo"])
                saved = y.grad_fn.saved_tensors
                y.backward(c["dy4"].cuda().bfloat16())
                ks = _stem_k(pooled, hw, C, c["geo"])
                _stem_check(w2, device, c, st, k, s, padding, y.detach(), saved[1], x.grad.reshape(M, C), gs, bs, mm,
                            mv, saved[3], saved[4], pooled, ks)
                # entry points
                gx, gg, gb, gmm, gmv = G(c["x4"].bfloat16()), G(c["g"]), G(c["b"]), G(c["mm0"]), G(c["mv0"])
                gps, gpq = G(ps), G(pq)
                gy = G(None, torch.bfloat16, (N_, oh_n, ow_n, C))
                garg = G(None, torch.uint8, (N_, oh_n, ow_n, C))
                gmean, ginv, gss = (G(None, torch.float32, (C,)), G(None, torch.float32, (C,)),
                                    G(None, torch.float32, (2 * C,)))
                _raw("mdtf_bn_relu_maxpool_fwd", _p(gx), _p(gy), _p(garg), N_, H, W, C, *c["geo"], _p(gg), _p(gb),
                     _p(gmm), _p(gmv), BH.f32(DECAY), BH.f32(EPS), _p(gmean), _p(ginv), _p(gps), _p(gpq), 3, _p(gss))
                NH.assert_contained(w2 + " raw fwd", [gx, gg, gb], [gy, garg, gmean, ginv, gss])
                assert gmm.guards_intact() and gmv.guards_intact()
                _zeroed_head(w2 + " psum", gps, ps, 3)
                _zeroed_head(w2 + " psq", gpq, pq, 3)
                gdy, gy_in, garg_in, gss_in = G(c["dy4"].bfloat16()), G(gy.t), G(garg.t), G(gss.t)
                gmean_in, ginv_in = G(gmean.t), G(ginv.t)
                gdx, gdg, gdb = G(None, torch.bfloat16, (N_, H, W, C)), G(c["dg0"]), G(c["db0"])
                gws = G(None, torch.float32, (_ws_floats(M, C),))
                _raw("mdtf_maxpool_bn_bwd", _p(gdy), _p(garg_in), _p(gx), _p(gdx), N_, H, W, C, *c["geo"], _p(gg),
                     _p(gmean_in), _p(ginv_in), _p(gdg), _p(gdb), _p(gss_in), _p(gws),
                     _p(gy_in) if pooled else _native.ptr(None))
                NH.assert_contained(w2 + " raw bwd", [gdy, garg_in, gx, gg, gmean_in, ginv_in, gss_in, gy_in], [gdx])
                assert gdg.guards_intact() and gdb.guards_intact() and gws.guards_intact()
                _stem_check(w2 + " raw", device, c, st, k, s, padding, gy.t, garg.t, gdx.t.reshape(M, C), gdg.t,
                            gdb.t, gmm.t, gmv.t, gmean.t, ginv.t, pooled, ks)
                assert NH.bits_equal(gy.t, y.detach()) and NH.bits_equal(gdx.t, x.grad)
    finally:
        _native.fn("mdtf_bn_pool_dx_pairs")(1)
