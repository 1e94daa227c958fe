"""The memory-bound NHWC kernels of ``csrc/kernels.hip`` (bias/activation, column sums, max/avg pooling, global
average pooling, LRN, softmax cross-entropy) against the independent fp64 oracles of ``nhwc_helpers``, element by
element, at the smallest shapes at which each code path can break.

Every test takes a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.nn`` on fp32 tensors holding
bf16-representable values (this validates the oracle and the bounds, and tests that branch without a GPU); ``cuda``
runs the HIP kernels on bf16 tensors, through the autograd wrappers and once more through the registered entry points
with every buffer inside sentinel guard bands (guards intact, inputs bitwise unchanged, every output element stored).

The bounds are those of ``nhwc_helpers``; the operation count k of every ``gamma(k)`` stands next to its use.

Measured constants (see ``nhwc_helpers``): fp32 ``torch.logsumexp`` is within 1.59 units of ``U * max(|lse|, 1)`` and
fp32 ``F.cross_entropy`` within 1.58 units of ``U * (|lse| + |x_label|)`` of the fp64 oracle on these inputs, both
rounded up to 2; the ``test_xent_*`` tests on ``cpu`` assert that, the kernels get 8 times it for their fast
intrinsics.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from mdtf.ops import _native
from mdtf.ops import nn as ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import U, gamma  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
_ACT = {None: 0, "relu": 1, "gelu": 2}


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _raw(name, *args):
    """A registered entry point called the way ``ops/kernels.py`` calls it."""
    from mdtf.ops import kernels  # noqa: F401  (registers the signatures)
    _native.check(_native.fn(name)(*args, _native.stream_ptr()), name)
    torch.cuda.synchronize()


def _p(g):
    return _native.ptr(g.t if isinstance(g, NH.Guarded) else g)


# =========================================================================================== bias / activation
def _bias_act_inputs(M, C, seed, with_bias):
    """x in [-3, 3] (past that the fp32 evaluation of 1 + tanh cancels to more than the neighbour rule allows), a bias
    of bf16-representable values so that row 0 can be x = -b (pre-activation exactly 0), then +0 and -0 in x."""
    x = NH.randn((M, C), seed).clamp(-3.0, 3.0)
    b = NH.randn((C,), seed + 1, 0.25) if with_bias else None
    if with_bias:
        x[0] = -b
    x[-1, 0::3] = 0.0
    x[-1, 1::3] = -0.0
    dy = NH.randn((M, C), seed + 2)
    dy[0, 0::2] = 0.0
    return x, b, dy


def _bias_act_run(device, x, b, act, dy, slot=None):
    xd = NH.put(x, device).requires_grad_(True)
    bd = b.to(device).requires_grad_(True) if b is not None else None
    if slot is not None:
        if device == "cuda":
            class Var(object):                  # what variables.grad_sink looks for: an fp32 gradient slot
                grad = slot
            bd._mdtf_var = Var()
        else:
            bd.grad = slot
    if device == "cuda":
        from mdtf.ops import kernels as K
        y = K.relu(xd) if (b is None and act == "relu") else K.bias_act(xd, bd, act)
    else:
        v = xd if b is None else ops.bias_add(xd, bd)
        if act == "relu":
            y = ops.relu(xd) if b is None else ops.bias_add_relu(xd, bd)
        else:
            y = ops.gelu(v) if act == "gelu" else v
    y.backward(NH.put(dy, device))
    db = None
    if b is not None:
        db = slot if (slot is not None and device == "cuda") else bd.grad
    return y.detach(), xd.grad, db


def _gelu_grad_slop(pre):
    # the fp32 evaluation of gelu'(pre): 0.5 (1 + t) + 0.5 pre (1 - t^2) c (1 + 3 a pre^2), under 32 operations over
    # terms of at most 1 + |pre| + 0.11 |pre|^3
    return gamma(32) * (1.0 + pre.abs() + 0.11 * pre.abs() ** 3)


def _bias_act_check(what, device, x, b, act, dy, y, dx, db, slot0=None, pre_rounded=None):
    bf = device == "cuda"
    x64, dy64 = x.double(), dy.double()
    b64 = b.double() if b is not None else torch.zeros(x.shape[1], dtype=torch.float64)
    pre = x64 + b64
    yref = NH.act64(pre, act)
    if act == "gelu":
        NH.check_neighbour(y, yref, what + " y")
    else:
        # k = 1: the bias add (none without a bias: bf16 in, bf16 out, exact)
        NH.check_bound(y, yref, NH.out_bound(yref, gamma(1 if b is not None else 0) * (x64.abs() + b64.abs()), bf),
                       what + " y")
    dxref = dy64 * NH.act_grad64(pre, act)
    if act == "gelu":
        # the kernel differentiates at the bf16-rounded pre-activation: |dy| max|gelu''| (half a bf16 ulp of pre) on
        # top of the final rounding; the fp32 add of the bias (U |pre|) is inside the slop
        acc = dy64.abs() * ((NH.GELU_D2_MAX * NH.half_ulp_bf16(pre) if bf else 0.0) + _gelu_grad_slop(pre))
        dxb = NH.out_bound(dxref, acc, bf)
        if pre_rounded is not None:
            # against the oracle AT the rounded pre-activation the fast-intrinsic rule applies
            NH.check_neighbour(dx, dy64 * NH.act_grad64(pre_rounded.double(), act), what + " dx at bf16 pre")
    else:
        dxb = NH.out_bound(dxref, torch.zeros_like(dxref), False)      # dy or 0: exact
    NH.check_bound(dx, dxref, dxb, what + " dx")
    if db is not None:
        # k = M + 1: a sum of M terms in any order, + the slot; every term carries its own bound
        M = x.shape[0]
        s0 = slot0.double() if slot0 is not None else torch.zeros_like(b64)
        dbref = dxref.sum(0) + s0
        dbb = dxb.expand_as(dxref).sum(0) + gamma(M + 1) * (dxref.abs().sum(0) + dxb.expand_as(dxref).sum(0) + s0.abs())
        NH.check_bound(db, dbref, dbb + NH.TINY, what + " db")


def _bias_act_raw(what, x, b, act, dy):
    """mdtf_bias_act_fwd / mdtf_act_bwd on guarded buffers."""
    M, C = x.shape
    gx = NH.Guarded(x.bfloat16(), "cuda")
    gb = NH.Guarded(b, "cuda") if b is not None else None
    gy = NH.Guarded(None, "cuda", torch.bfloat16, (M, C))
    gpre = NH.Guarded(None, "cuda", torch.bfloat16, (M, C)) if act == "gelu" else None
    _raw("mdtf_bias_act_fwd", _p(gx), _p(gb), _p(gy), _p(gpre), M, C, _ACT[act])
    NH.assert_contained(what + " fwd", [gx] + ([gb] if gb else []), [gy] + ([gpre] if gpre else []))
    if gpre is not None:
        pre = x.double() + (b.double() if b is not None else 0.0)
        NH.check_bound(gpre.t, pre, NH.out_bound(pre, gamma(1) * (x.double().abs() + pre.abs()), True), what + " pre")
    dx, pre_rounded = dy.clone(), None
    if act is not None:
        gdy = NH.Guarded(dy.bfloat16(), "cuda")
        gsaved = NH.Guarded(gy.t if act == "relu" else gpre.t, "cuda")
        gdx = NH.Guarded(None, "cuda", torch.bfloat16, (M, C))
        null = _native.ptr(None)
        _raw("mdtf_act_bwd", _p(gdy), _p(gsaved) if act == "gelu" else null, _p(gsaved) if act == "relu" else null,
             _p(gdx), M * C, _ACT[act])
        NH.assert_contained(what + " bwd", [gdy, gsaved], [gdx])
        dx = gdx.t
        pre_rounded = gpre.t.float().cpu() if act == "gelu" else None
    return gy.t, dx, pre_rounded


# (1,8): one vector | (3,24): C not a power of two | (4,10): scalar forward (C % 8) and vector backward (n % 8 == 0)
# | (3,10): scalar both ways | (33,64): 264 vectors, a second block with 8 live threads
BIAS_ACT_SHAPES = [(1, 8), (3, 24), (4, 10), (3, 10), (33, 64)]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("act", [None, "relu", "gelu"])
@pytest.mark.parametrize("device", DEVICES)
def test_bias_act_direct(device, act, with_bias):
    device = _device(device)
    for M, C in BIAS_ACT_SHAPES:
        what = "%s/bias_act %s bias=%d (%d,%d)" % (device, act, with_bias, M, C)
        x, b, dy = _bias_act_inputs(M, C, 100 + M + C, with_bias)
        y, dx, db = _bias_act_run(device, x, b, act, dy)
        _bias_act_check(what, device, x, b, act, dy, y, dx, db)
        if with_bias:
            slot0 = NH.randn((C,), 7, 3.0)
            _, _, db2 = _bias_act_run(device, x, b, act, dy, slot=slot0.to(device).clone())
            _bias_act_check(what + " slot", device, x, b, act, dy, y, dx, db2, slot0=slot0)
        if device == "cuda":
            y2, dx2, pre_r = _bias_act_raw(what + " raw", x, b, act, dy)
            _bias_act_check(what + " raw", device, x, b, act, dy, y2, dx2, None, pre_rounded=pre_r)
            assert NH.bits_equal(y2, y) and (act is None or NH.bits_equal(dx2, dx))


@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("device", DEVICES)
def test_bias_act_second_grid_stride_trip(device, act):
    """8 * (4096 * 256 + 37) elements: the grid is capped at 4096 blocks of 256 threads, 37 threads go round again."""
    device = _device(device)
    M, C = 4096 * 256 + 37, 8
    x, b, dy = _bias_act_inputs(M, C, 140, True)
    y, dx, db = _bias_act_run(device, x, b, act, dy)
    _bias_act_check("%s/bias_act %s big" % (device, act), device, x, b, act, dy, y, dx, db)


# ================================================================================================ column sums
def _colsum(device, x, out0):
    if device == "cuda":
        from mdtf.ops import kernels as K
        return K.colsum_into(NH.put(x, device), out0.to(device).clone())
    b = torch.zeros(x.shape[1], requires_grad=True)             # the bias gradient of ops.bias_add is the column sum
    b.grad = out0.clone()
    ops.bias_add(torch.zeros_like(x), b).backward(x)
    return b.grad


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("device", DEVICES)
def test_colsum(device, deterministic):
    """M around the 16 rows of one block's pass (1, 15, 16, 17) and 300 (several blocks); C = 8 (one live lane), 10
    (scalar kernel), 520 (a second 512-column slab with one live lane)."""
    device = _device(device)
    was = _native.deterministic()
    try:
        _native.set_deterministic(deterministic)
        for M in (1, 15, 16, 17, 300):
            for C in (8, 10, 520):
                x = NH.randn((M, C), 200 + M + C)
                out0 = NH.randn((C,), 5, 3.0)
                got = _colsum(device, x, out0)
                ref = x.double().sum(0) + out0.double()
                # k = M + 1: M terms in any order and the add onto the slot (the two-stage tree is shorter)
                bound = gamma(M + 1) * (x.double().abs().sum(0) + out0.double().abs()) + NH.TINY
                NH.check_bound(got, ref, bound, "%s/colsum det=%d (%d,%d)" % (device, deterministic, M, C))
                if deterministic:
                    assert NH.bits_equal(_colsum(device, x, out0), got)
    finally:
        _native.set_deterministic(was)


# ==================================================================================================== pooling
# (name, (H, W), (KH, KW), (SH, SW), padding)
POOL_CASES = [
    ("k3s2same_odd", (7, 5), (3, 3), (2, 2), "SAME"),
    ("k3s2same_even", (8, 6), (3, 3), (2, 2), "SAME"),         # pad_top 0, pad_bottom 1
    ("k2s2same_odd", (7, 5), (2, 2), (2, 2), "SAME"),
    ("k3s1same", (7, 5), (3, 3), (1, 1), "SAME"),
    ("k3s1valid", (8, 6), (3, 3), (1, 1), "VALID"),
    ("k2s3valid", (8, 6), (2, 2), (3, 3), "VALID"),            # stride > kernel: rows 2, 5 and cols 2, 5 in no window
    ("k3s2same_2x2", (2, 2), (3, 3), (2, 2), "SAME"),          # window larger than the image
    ("k7valid_7x7", (7, 7), (7, 7), (1, 1), "VALID"),
    ("k23s12same", (7, 5), (2, 3), (1, 2), "SAME"),            # non-square kernel and stride
    ("k23s12valid", (8, 6), (2, 3), (1, 2), "VALID"),
]
POOL_C = (8, 24, 64)            # cv = 1, 3 (not a power of two), 8


def _pool_inputs(kind, shape, seed):
    if kind == "random":
        return NH.randn(shape, seed)
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "channel_const":                                  # every window is one tie
        return NH.randn((shape[-1],), seed).expand(shape).contiguous()
    return torch.relu(NH.randn(shape, seed))                     # post-ReLU: about half the taps tie at +0


def _pool_run(device, x, dy, k, s, padding, is_max):
    xd = NH.put(x, device).requires_grad_(True)
    y = (ops.max_pool if is_max else ops.avg_pool)(xd, k, s, padding)
    y.backward(NH.put(dy, device))
    return y.detach(), xd.grad


def _pool_check(what, bf, x, dy, k, s, is_max, fwd, bwd, y, dx):
    dxref, sabs, nwin = bwd
    if is_max:
        assert torch.equal(y.cpu().double(), fwd["y"]), what + ": max-pool forward is not the oracle's"
        assert not bf or NH.bits_equal(y, fwd["y"].bfloat16()), what + ": max-pool forward is not bitwise the oracle's"
        # k = windows over the pixel: one add per gathered term
        NH.check_bound(dx, dxref, NH.out_bound(dxref, gamma(nwin)[None, :, :, None] * sabs, bf), what + " dx")
    else:
        # k = KH*KW + 3: the taps' sum, the reciprocal and the product (the PyTorch branch: /(KH*KW), *(KH*KW), /count)
        NH.check_bound(y, fwd["y"], NH.out_bound(fwd["y"], gamma(k[0] * k[1] + 3) * fwd["sabs"], bf), what + " y")
        # k = windows + 3: per term the reciprocal and the product (the PyTorch branch: three scalings), then the sum
        NH.check_bound(dx, dxref, NH.out_bound(dxref, gamma(nwin + 3)[None, :, :, None] * sabs, bf), what + " dx")


def _pool_raw(what, x, dy, k, s, is_max, fwd):
    n, h, w, c = x.shape
    oh, ow, pt, pl = fwd["geo"]
    geo = [n, h, w, c, oh, ow, k[0], k[1], s[0], s[1], pt, pl]
    gx = NH.Guarded(x.bfloat16(), "cuda")
    gy = NH.Guarded(None, "cuda", torch.bfloat16, (n, oh, ow, c))
    garg = NH.Guarded(None, "cuda", torch.uint8, (n, oh, ow, c)) if is_max else None
    _raw("mdtf_pool_fwd", int(is_max), _p(gx), _p(gy), _p(garg), *geo)
    NH.assert_contained(what + " fwd", [gx], [gy] + ([garg] if is_max else []))
    if is_max:
        assert torch.equal(garg.t.cpu().long(), fwd["arg"]), what + ": argmax is not the first maximum in scan order"
    gdy = NH.Guarded(dy.bfloat16(), "cuda")
    gin = NH.Guarded(fwd["arg"].to(torch.uint8), "cuda") if is_max else None     # the oracle's argmax, not the kernel's
    gdx = NH.Guarded(None, "cuda", torch.bfloat16, (n, h, w, c))
    _raw("mdtf_pool_bwd", int(is_max), _p(gdy), _p(gin), _p(gdx), *geo)
    NH.assert_contained(what + " bwd", [gdy] + ([gin] if is_max else []), [gdx])
    return gy.t, gdx.t


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
@pytest.mark.parametrize("is_max", [True, False], ids=["max", "avg"])
@pytest.mark.parametrize("device", DEVICES)
def test_pool(device, is_max, case):
    device = _device(device)
    name, (h, w), k, s, padding = case
    for c in POOL_C:
        for kind in ("random", "zeros", "channel_const", "post_relu"):
            what = "%s/%s %s C=%d %s" % (device, "max" if is_max else "avg", name, c, kind)
            x = _pool_inputs(kind, (2, h, w, c), 300 + c)
            fwd = NH.pool_ref(x.double(), k, s, padding, is_max)
            dy = NH.randn(tuple(fwd["y"].shape), 301 + c)
            bwd = NH.pool_bwd_ref(dy.double(), fwd, x.shape, k, s, is_max)
            y, dx = _pool_run(device, x, dy, k, s, padding, is_max)
            assert tuple(y.shape) == tuple(fwd["y"].shape), (what, y.shape)
            _pool_check(what, device == "cuda", x, dy, k, s, is_max, fwd, bwd, y, dx)
            if device == "cuda":
                y2, dx2 = _pool_raw(what + " raw", x, dy, k, s, is_max, fwd)
                _pool_check(what + " raw", True, x, dy, k, s, is_max, fwd, bwd, y2, dx2)


@pytest.mark.parametrize("device", DEVICES)
def test_avg_pool_second_grid_stride_trip(device):
    """avgpool_fwd / avgpool_bwd cap their grid at 4096 blocks: 14565 images of 3 x 3 x 64 are 4096*256 + 104 vectors
    each way."""
    device = _device(device)
    k, s, padding = (3, 3), (1, 1), "SAME"
    x = NH.randn((14565, 3, 3, 64), 350)
    fwd = NH.pool_ref(x.double(), k, s, padding, False)
    dy = NH.randn(tuple(fwd["y"].shape), 351)
    bwd = NH.pool_bwd_ref(dy.double(), fwd, x.shape, k, s, False)
    y, dx = _pool_run(device, x, dy, k, s, padding, False)
    _pool_check("%s/avg big" % device, device == "cuda", x, dy, k, s, False, fwd, bwd, y, dx)


@pytest.mark.parametrize("is_max", [True, False], ids=["max", "avg"])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_pool_rejects_unsupported_shapes(device, is_max):
    """The argmax is one byte (KH*KW <= 255) and every access a bf16x8 vector (C % 8 == 0): anything else is an
    error, never data."""
    device = _device(device)
    pool = ops.max_pool if is_max else ops.avg_pool
    with pytest.raises(RuntimeError, match="invalid argument"):
        pool(torch.zeros((1, 16, 16, 8), dtype=torch.bfloat16, device=device), (16, 16), (1, 1), "VALID")
    with pytest.raises(RuntimeError, match="invalid argument"):
        pool(torch.zeros((1, 4, 4, 12), dtype=torch.bfloat16, device=device), (2, 2), (2, 2), "SAME")
    torch.cuda.synchronize()


@pytest.mark.parametrize("device", GPU_ONLY)
def test_maxpool_64bit_index_path(device):
    """N*H*W*C = 2^31: the ``long long`` instantiation of maxpool_fwd / maxpool_bwd.  Forward and backward on the
    whole tensor are bitwise the same calls on the two batch halves, which take the ``int`` path ``test_pool``
    verifies."""
    device = _device(device)
    free, _ = torch.cuda.mem_get_info()
    if free < 32 * 2 ** 30:
        pytest.skip("needs 32 GiB of free device memory, %.1f GiB free" % (free / 2 ** 30))
    shape = (2, 1024, 1024, 1024)
    gen = torch.Generator(device=device).manual_seed(5)
    x = torch.empty(shape, dtype=torch.bfloat16, device=device).normal_(generator=gen)
    x[1, -1, -1, -8:] = 100.0                                    # the last vector of the tensor matters
    k, s, padding = (3, 3), (2, 2), "SAME"
    dy = torch.empty((2, 512, 512, 1024), dtype=torch.bfloat16, device=device).normal_(generator=gen)

    def run(xs, dys):
        xs = xs.detach().requires_grad_(True)
        y = ops.max_pool(xs, k, s, padding)
        y.backward(dys)
        return y.detach(), xs.grad

    y, dx = run(x, dy)
    assert float(y[1, -1, -1, -1]) == 100.0 and float(dx[1, -1, -1, -1]) == float(dy[1, -1, -1, -1])
    for n in range(2):
        yh, dxh = run(x[n:n + 1], dy[n:n + 1])
        assert torch.equal(y[n:n + 1].view(torch.int16), yh.view(torch.int16)), "forward, batch half %d" % n
        assert torch.equal(dx[n:n + 1].view(torch.int16), dxh.view(torch.int16)), "backward, batch half %d" % n
        del yh, dxh


# ======================================================================================== global average pool
# (3,1,8): HW below the four row groups | (2,3,520): three of four groups live, a second 512-channel slab with one
# live lane | (2,49,512): ResNet's 7x7, one full slab | (1,50,1024): two full slabs, HW % 4 == 2
GAP_SHAPES = [(3, 1, 8), (2, 3, 520), (2, 49, 512), (1, 50, 1024)]


@pytest.mark.parametrize("shape", GAP_SHAPES, ids=["x".join(map(str, s)) for s in GAP_SHAPES])
@pytest.mark.parametrize("device", DEVICES)
def test_global_avg_pool(device, shape):
    device = _device(device)
    n, hw, c = shape
    bf = device == "cuda"
    x = NH.randn((n, hw, 1, c), 400 + hw) + 0.5
    x = NH.bf16_exact(x)
    dy = NH.randn((n, c), 401 + hw)
    x64, dy64 = x.double().view(n, hw, c), dy.double()
    yref = x64.sum(1) / hw
    dxref = (dy64 / hw)[:, None, :].expand(n, hw, c)
    # k = HW + 2: the sum in any order, the reciprocal and the product (the PyTorch branch: sum and division)
    yb = NH.out_bound(yref, gamma(hw + 2) * x64.abs().sum(1) / hw, bf)
    # k = 2: the reciprocal and the product
    dxb = NH.out_bound(dxref, gamma(2) * dxref.abs(), bf)
    xd = NH.put(x, device).requires_grad_(True)
    y = ops.global_avg_pool(xd)
    y.backward(NH.put(dy, device))
    what = "%s/gap %s" % (device, shape)
    NH.check_bound(y, yref, yb, what + " y")
    NH.check_bound(xd.grad.view(n, hw, c), dxref, dxb, what + " dx")
    if device == "cuda":
        gx, gdy = NH.Guarded(x.bfloat16(), device), NH.Guarded(dy.bfloat16(), device)
        gy = NH.Guarded(None, device, torch.bfloat16, (n, c))
        gdx = NH.Guarded(None, device, torch.bfloat16, (n, hw, c))
        _raw("mdtf_gap_fwd", _p(gx), _p(gy), n, hw, c)
        _raw("mdtf_gap_bwd", _p(gdy), _p(gdx), n, hw, c)
        NH.assert_contained(what + " raw", [gx, gdy], [gy, gdx])
        NH.check_bound(gy.t, yref, yb, what + " raw y")
        NH.check_bound(gdx.t, dxref, dxb, what + " raw dx")


@pytest.mark.parametrize("device", DEVICES)
def test_global_avg_pool_backward_second_grid_stride_trip(device):
    """gap_bwd's grid is capped at 4096 blocks: N*HW*C/8 = 4096*256 + 64 vectors."""
    device = _device(device)
    n, hw, c = 1, 4096 * 4 + 1, 512
    dy = NH.randn((n, c), 410)
    xd = NH.put(torch.zeros((n, hw, 1, c)), device).requires_grad_(True)
    ops.global_avg_pool(xd).backward(NH.put(dy, device))
    dxref = (dy.double() / hw)[:, None, :].expand(n, hw, c)
    NH.check_bound(xd.grad.view(n, hw, c), dxref, NH.out_bound(dxref, gamma(2) * dxref.abs(), device == "cuda"),
                   "%s/gap_bwd big" % device)


# ========================================================================================================= LRN
# bias = 2, alpha = 1 and |x| up to 4: the window's sum of squares is of the order of the bias or far above it, so
# the identity function (which the 1e-2 norm check of a bias = 1, alpha = 1e-4 LRN cannot tell from the kernel), a
# window off by one channel or a wrong edge all fail by whole bf16 steps.
# (32,4): interior and both edges | (8,5), (5,5): the window covers the whole axis | (96,2): narrow window, C not a
# power of two | (16,0): no neighbours at all | (136,64), (200,70): the largest radius lrn_bwd stages in LDS and the
# first that takes lrn_bwd_direct
LRN_CASES = [(32, 4), (8, 5), (5, 5), (96, 2), (16, 0), (136, 64), (200, 70)]


def _lrn(device, P, C, r, beta, seed, xmax=4.0, one_hot_dy=False):
    bias, alpha = 2.0, 1.0
    bf = device == "cuda"
    what = "%s/lrn P=%d C=%d r=%d beta=%g" % (device, P, C, r, beta)
    x = NH.bf16_exact((NH.randn((1, P, 1, C), seed) * 1.5).clamp(-xmax, xmax))
    dy = NH.randn((1, P, 1, C), seed + 1)
    if one_hot_dy:
        dy = dy * (torch.arange(C)[None, :] == (torch.arange(P) * 7 % C)[:, None]).view(1, P, 1, C)
    yref, dxref = NH.lrn_ref(x.double(), dy.double(), r, bias, alpha, beta)
    xd = NH.put(x, device).requires_grad_(True)
    y = ops.lrn(xd, r, bias, alpha, beta)
    y.backward(NH.put(dy, device))
    NH.check_neighbour(y.detach(), yref, what + " y")
    NH.check_neighbour(xd.grad, dxref, what + " dx")
    if bf:
        gx, gdy = NH.Guarded(x.bfloat16(), device), NH.Guarded(dy.bfloat16(), device)
        gy = NH.Guarded(None, device, torch.bfloat16, x.shape)
        gd = NH.Guarded(None, device, torch.float32, x.shape)
        _raw("mdtf_lrn_fwd", _p(gx), _p(gy), _p(gd), P, C, r, bias, alpha, beta)
        NH.assert_contained(what + " raw fwd", [gx], [gy, gd])
        gyi, gdi = NH.Guarded(gy.t, device), NH.Guarded(gd.t, device)
        gdx = NH.Guarded(None, device, torch.bfloat16, x.shape)
        _raw("mdtf_lrn_bwd", _p(gdy), _p(gx), _p(gyi), _p(gdi), _p(gdx), P, C, r, alpha, beta)
        NH.assert_contained(what + " raw bwd", [gdy, gx, gyi, gdi], [gdx])
        NH.check_neighbour(gy.t, yref, what + " raw y")
        NH.check_neighbour(gdx.t, dxref, what + " raw dx")
        # the saved denominator, fp32: k = 2r + 3 (the squares' sum, alpha *, bias +)
        x64 = x.double()
        win = torch.stack([(x64 * x64)[..., max(0, i - r):min(C, i + r + 1)].sum(-1) for i in range(C)], -1)
        NH.check_bound(gd.t, bias + alpha * win, gamma(2 * r + 3) * (bias + alpha * win), what + " raw d")


@pytest.mark.parametrize("beta", [0.75, 0.5])
@pytest.mark.parametrize("C,r", LRN_CASES)
@pytest.mark.parametrize("device", DEVICES)
def test_lrn(device, C, r, beta):
    _lrn(_device(device), 3, C, r, beta, 500 + C + r)


@pytest.mark.parametrize("device", DEVICES)
def test_lrn_second_grid_stride_trip(device):
    """P*C = 4096*256 + 96 elements: three positions go round the capped grid again.  dx is the difference of two
    terms, and among a million random elements some cancel to where no fp32 evaluation can give the neighbour rule.
    Here none can: dy is non-zero in one channel per position (another channel in every position), so dx is one
    product outside that channel, and in it dy d^(-beta-1) (bias + sum_{j != c} x_j^2 - 0.5 x_c^2) with
    0.5 x_c^2 <= 1.81 < bias."""
    _lrn(_device(device), 4096 * 8 + 3, 32, 4, 0.75, 540, xmax=1.9, one_hot_dy=True)


# ======================================================================================= softmax cross-entropy
def _xent_chain(K):
    # the longest path of the exp-sum: a thread's K/64 terms (one wave per row; the row kernels' 256 threads have
    # fewer) each with an add and, in the online form, a rescale, then 6 + 4 merges of three roundings each
    return 2 * -(-K // 64) + 30


def _xent_layout(x, device, dtype, ld, offset):
    """The logits as a [N, K] view of a device buffer of row stride ld, ``offset`` elements into the allocation;
    returns (leaf buffer, view)."""
    n, k = x.shape
    buf = torch.zeros(n * ld + offset, dtype=dtype, device=device)
    view = buf[offset:].view(n, ld)[:, :k]
    with torch.no_grad():
        view.copy_(x)
    buf.requires_grad_(True)
    return buf, buf[offset:].view(n, ld)[:, :k]


def _xent(device, x, labels, dloss, bf16_logits=True, ld=None, offset=0, what=""):
    """loss and dlogits through ops.sparse_softmax_cross_entropy_with_logits (and lse, loss, dlogits through the
    entry points on the GPU) against the fp64 oracle."""
    n, k = x.shape
    ld = k if ld is None else ld
    what = "%s/xent %s K=%d ld=%d off=%d %s" % (device, "bf16" if bf16_logits else "fp32", k, ld, offset, what)
    gpu = device == "cuda"
    lse_ref, loss_ref, dl_ref, p_ref = NH.xent_ref(x.double(), labels, dloss.double())
    e_lse, e_loss = NH.lse_bound(x.double(), labels, lse_ref, _xent_chain(k))
    dtype = torch.bfloat16 if (gpu and bf16_logits) else torch.float32
    buf, view = _xent_layout(x, device, dtype, ld, offset)
    seen = []
    view.register_hook(lambda g: seen.append(g))
    loss = ops.sparse_softmax_cross_entropy_with_logits(labels.to(device), view)
    loss.backward(dloss.to(device))
    NH.check_bound(loss.detach(), loss_ref, e_loss, what + " loss")
    dl = buf.grad[offset:].view(n, ld)
    assert not bool(dl[:, k:].any()), what + ": pad columns of the gradient"

    def check_dl(got, tag):
        if bf16_logits:
            NH.check_neighbour(got, dl_ref, what + tag)
        else:
            # fp32 out: p = exp(x - lse) inherits the error of lse, the subtraction's rounding and the exp's
            # argument and result roundings (8 ulp, as for lse); then the subtraction of the one-hot and the product
            a = (x.double() - lse_ref[:, None]).abs()
            eb = p_ref * (e_lse[:, None] + NH.INTRINSIC_FACTOR * U * (1.4427 * a + 2.0))
            NH.check_bound(got, dl_ref, dloss.double().abs()[:, None] * eb * (1 + 4 * U) + gamma(2) * dl_ref.abs()
                           + NH.TINY, what + tag)

    check_dl(dl[:, :k], " dlogits")
    if gpu and seen[0]._base is not None and ld != k:
        # what the decoder's backward reads: the whole padded rows behind the returned view
        base = seen[0]._base
        assert base.shape[1] >= k and not bool(base[:, k:].any()), what + ": pad columns behind the returned view"
    if not gpu:
        # the measured constants of the module header, asserted where they were measured
        lse32 = torch.logsumexp(x, 1).double()
        ce32 = F.cross_entropy(x, labels, reduction="none").double()
        xl = x.double().gather(1, labels[:, None]).squeeze(1).abs()
        fin = torch.isfinite(lse_ref)
        u_lse = float(((lse32 - lse_ref).abs() / (U * lse_ref.abs().clamp(min=1.0)))[fin].max())
        u_loss = float(((ce32 - loss_ref).abs() / (U * (lse_ref.abs() + xl)))[fin].max())
        print("NHWC_CPU %-58s logsumexp %.3f units, cross_entropy %.3f units" % (what, u_lse, u_loss))
        assert u_lse <= NH.LSE_UNITS_CPU and u_loss <= NH.LOSS_UNITS_CPU, (what, u_lse, u_loss)
        return
    # the entry points on guarded buffers; inputs keep the layout (stride, offset) of the wrapper's call
    labels_d = NH.Guarded(labels, device)
    gl = NH.Guarded(None, device, torch.float32, (n,))
    glse = NH.Guarded(None, device, torch.float32, (n,))
    before = buf.detach().clone()
    src = buf.detach()[offset:].view(n, ld)[:, :k]
    _raw("mdtf_xent_fwd", _native.ptr(src), int(bf16_logits), _p(labels_d), n, k, ld, _p(gl), _p(glse))
    NH.assert_contained(what + " raw fwd", [labels_d], [gl, glse])
    NH.check_bound(glse.t, lse_ref, e_lse, what + " raw lse")
    NH.check_bound(gl.t, loss_ref, e_loss, what + " raw loss")
    assert NH.bits_equal(gl.t, loss.detach())
    ldo = ld if (ld != k and ld % 8 == 0 and bf16_logits) else k
    gdl = NH.Guarded(None, device, dtype, (n, ldo))
    gdloss = NH.Guarded(dloss, device)
    glse_in = NH.Guarded(glse.t, device)
    _raw("mdtf_xent_bwd", _native.ptr(src), int(bf16_logits), _p(labels_d), _p(glse_in), _p(gdloss), _p(gdl), n, k, ld,
         ldo)
    vec = bf16_logits and ld % 8 == 0 and ldo % 8 == 0 and src.data_ptr() % 16 == 0
    assert gdl.guards_intact() and labels_d.unchanged() and gdloss.unchanged() and glse_in.unchanged()
    assert torch.equal(buf.detach().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       before.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), what + ": logits modified"
    if vec or ldo == k:
        assert gdl.all_written(), what + ": dlogits has elements no thread stored"
    if vec:
        assert not bool(gdl.t[:, k:].any()), what + ": pad columns of the raw gradient"
    check_dl(gdl.t[:, :k], " raw dlogits")


# 10: K < 64, lanes without a term | 64, 65: one term per lane, one lane with two | 1000 | 2048: the row kernels'
# threshold, exactly one vector per thread | 2049: odd, generic | 2050: even, no multiple of 8: the pair kernel |
# 8200: the four-loads-in-flight loop (kv = 1025 > 4 * 256) and a tail
XENT_K = [10, 64, 65, 1000, 2048, 2049, 2050, 8200]


@pytest.mark.parametrize("K", XENT_K)
@pytest.mark.parametrize("device", DEVICES)
def test_xent_contiguous(device, K):
    device = _device(device)
    x, labels, dloss = NH.xent_case(3, K, 600 + K)
    _xent(device, x, labels, dloss)


@pytest.mark.parametrize("device", DEVICES)
def test_xent_backward_second_grid_stride_trip(device):
    """The generic xent_bwd caps its grid at 4096 blocks: 513 rows of 2049 (odd: no vector path) are 4096*256 + 2561
    elements."""
    device = _device(device)
    x, labels, dloss = NH.xent_case(513, 2049, 650)
    _xent(device, x, labels, dloss)


# 2052 of 2056: a v8 row whose last vector is half masked | 8199 of 8208: odd K on the v8 kernel, 7 of the last
# vector's 8 live, the four-in-flight loop
@pytest.mark.parametrize("K,ld", [(2052, 2056), (8199, 8208)])
@pytest.mark.parametrize("device", DEVICES)
def test_xent_strided_rows(device, K, ld):
    device = _device(device)
    x, labels, dloss = NH.xent_case(3, K, 700 + K)
    _xent(device, x, labels, dloss, ld=ld)


@pytest.mark.parametrize("K,ld", [(2050, 2056), (1000, 1008)])
@pytest.mark.parametrize("device", DEVICES)
def test_xent_two_byte_offset_view(device, K, ld):
    """Rows that start 2 bytes past a 4-byte boundary: neither row kernel applies, the generic kernels run and the
    wrapper zero-fills the pad columns."""
    device = _device(device)
    x, labels, dloss = NH.xent_case(3, K, 800 + K)
    _xent(device, x, labels, dloss, ld=ld, offset=1)


@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("device", DEVICES)
def test_xent_fp32_logits(device, K):
    device = _device(device)
    x, labels, dloss = NH.xent_case(3, K, 900 + K)
    gen = torch.Generator().manual_seed(K)
    x = x + torch.rand(x.shape, generator=gen) * 2.0 ** -6       # not bf16-representable
    _xent(device, x, labels, dloss, bf16_logits=False)


# (K, ld, first masked column, one past the last): the classes a caller masked out are -inf.  [0, 2048) of 8200: the
# first 16-byte vector of every thread of xent_fwd_row_v8; [0, 16) of 2050: the first pair of threads 0-7 of
# xent_fwd_row_bf16; the same as a view of 2056-wide rows: the first vector of threads 0-1 of the v8 kernel;
# [0, 16) of 1000: the one-wave kernel, which always handled this
XENT_MASKED = [(8200, 8200, 0, 2048), (2050, 2050, 0, 16), (2050, 2056, 0, 16), (1000, 1000, 0, 16)]


@pytest.mark.parametrize("K,ld,lo,hi", XENT_MASKED)
@pytest.mark.parametrize("device", DEVICES)
def test_xent_masked_classes(device, K, ld, lo, hi):
    """A thread whose first pair / vector is all -inf must not accumulate exp(-inf - (-inf)) = NaN."""
    device = _device(device)
    x, labels, dloss = NH.xent_case(3, K, 1000 + K)
    x[:, lo:hi] = float("-inf")
    x[:, hi] = x[:, hi].abs() + 3.0
    labels = torch.tensor([hi, K - 1, (K // 2) | 1])
    _xent(device, NH.bf16_exact(x), labels, dloss, ld=ld, what="masked [%d,%d)" % (lo, hi))
