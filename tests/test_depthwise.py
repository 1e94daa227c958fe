"""``mdtf.nn.depthwise_conv2d`` / ``separable_conv2d`` and the kernels of ``csrc/depthwise.hip`` against the
independent fp64 oracles of ``depthwise_helpers``, element by element, at the smallest shapes at which the index
arithmetic can still be wrong.

Every test takes a device: ``cpu`` runs the PyTorch expression of ``mdtf.ops.nn`` on fp32 tensors holding
bf16-representable values (this validates the oracle and the bounds, and tests that branch without a GPU); ``cuda``
runs the HIP kernels on bf16 tensors, through the autograd wrapper and once more through the registered entry points
with every buffer inside sentinel guard bands (guards intact, inputs bitwise unchanged, every output element stored).

All bounds are derived (``depthwise_helpers``): y and dx within ``gamma(T) * sum |terms|`` of the oracle for the T taps
inside the image plus the final bf16 rounding; dw within ``gamma(N * OH * OW + 2) * sum |terms|``.
"""
import functools
import math
import os
import sys

import pytest
import torch

import mdtf
from mdtf.ops import _native
from mdtf.ops import nn as ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthwise_helpers as DH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import gamma  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
EINVAL = -1

#        name                 N  H   W   C    filter  s  d  padding
CASES = [("1_7x7x8",          (2, 7, 7, 8),   (3, 3), 1, 1, "SAME"),
         ("2_8x8x24_s2",      (2, 8, 8, 24),  (3, 3), 2, 1, "SAME"),
         ("3_9x9x16_5x5_s2",  (1, 9, 9, 16),  (5, 5), 2, 1, "SAME"),
         ("4_5x11x8_valid",   (2, 5, 11, 8),  (3, 3), 1, 1, "VALID"),
         ("5a_6x6x8_3x1",     (1, 6, 6, 8),   (3, 1), 1, 1, "SAME"),
         ("5b_6x6x8_1x3",     (1, 6, 6, 8),   (1, 3), 1, 1, "SAME"),
         ("6_2x2x8",          (1, 2, 2, 8),   (3, 3), 1, 1, "SAME"),
         ("7_9x9x8_dil2",     (1, 9, 9, 8),   (3, 3), 1, 2, "SAME"),
         ("8_8x8x8_7x7",      (1, 8, 8, 8),   (7, 7), 1, 1, "SAME"),
         ("9_13x13x16",       (3, 13, 13, 16), (3, 3), 1, 1, "SAME")]
CASE_IDS = [c[0] for c in CASES]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


class _Case(object):
    """Inputs (bf16-representable fp32) and the fp64 oracle of one geometry, computed once and left unchanged."""

    def __init__(self, shape, k, s, d, padding, seed, mult=1):
        self.geo = g = DH.Geo(shape, k, s, d, padding)
        self.mult = mult
        self.x = NH.randn(shape, seed)
        self.w = NH.randn((g.kh, g.kw, g.c, mult), seed + 1, 0.5)
        self.dy = NH.randn((g.n, g.oh, g.ow, g.c * mult), seed + 2)
        x64, w64, dy64 = self.x.double(), self.w.double(), self.dy.double()
        self.y, self.y_abs, self.y_cnt = DH.fwd_ref(x64, w64, g)
        self.dx, self.dx_abs, self.dx_cnt = DH.dgrad_ref(dy64, w64, g)
        self.dw, self.dw_abs = DH.wgrad_ref(x64, dy64, g, mult)


@functools.lru_cache(maxsize=None)
def _case(i):
    _, shape, k, s, d, padding = CASES[i]
    return _Case(shape, k, s, d, padding, 100 + 10 * i)


class _Slot(object):
    """What ``variables.grad_sink`` looks for: an fp32 gradient slot."""

    def __init__(self, grad):
        self.grad = grad


def _public(device, case, slot0=None):
    """forward + backward through ``mdtf.nn.depthwise_conv2d``.  cuda: the weight gradient lands in an fp32 slot
    (pre-filled with ``slot0`` or zeros), cpu: in ``w.grad``."""
    g = case.geo
    xd = NH.put(case.x, device).requires_grad_(True)
    wd = NH.put(case.w, device).requires_grad_(True)
    slot = None
    if device == "cuda":
        slot = (slot0.to(device) if slot0 is not None else torch.zeros(case.w.shape, device=device)).contiguous()
        wd._mdtf_var = _Slot(slot)
    y = ops.depthwise_conv2d(xd, wd, [1, g.sh, g.sw, 1], g.padding, dilations=(g.dh, g.dw))
    y.backward(NH.put(case.dy, device))
    dw = wd.grad if slot is None else slot
    if slot is None and slot0 is not None:
        dw = dw + slot0
    return y.detach(), xd.grad, dw


def _check(what, device, case, y, dx, dw, slot0=None):
    bf = device == "cuda"
    assert y.dtype == (torch.bfloat16 if bf else torch.float32) and dx.dtype == y.dtype
    NH.check_bound(y, case.y, DH.y_bound(case.y, case.y_abs, case.y_cnt, bf), what + " y")
    NH.check_bound(dx, case.dx, DH.y_bound(case.dx, case.dx_abs, case.dx_cnt, bf), what + " dx")
    assert dw.dtype == torch.float32
    ref, sabs = case.dw, case.dw_abs
    if slot0 is not None:
        ref, sabs = ref + slot0.double(), sabs + slot0.double().abs()
    NH.check_bound(dw, ref, DH.dw_bound(sabs, case.geo), what + " dw")


def _p(g):
    return _native.ptr(g.t if isinstance(g, NH.Guarded) else g)


def _call(name, *args):
    from mdtf.ops import depthwise  # noqa: F401  (registers the signatures)
    rc = _native.fn(name)(*args, _native.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _raw(case, accumulate=None):
    """The three entry points on guarded buffers; returns y, dx, dw (and the workspace size in floats)."""
    from mdtf.ops import depthwise
    g = case.geo
    ints = g.ints()
    gx, gw = NH.Guarded(case.x.bfloat16(), "cuda"), NH.Guarded(case.w.bfloat16(), "cuda")
    gdy = NH.Guarded(case.dy.bfloat16(), "cuda")
    gy = NH.Guarded(None, "cuda", torch.bfloat16, case.dy.shape)
    gdx = NH.Guarded(None, "cuda", torch.bfloat16, case.x.shape)
    floats = int(_native.fn("mdtf_dwconv_wgrad_ws")(g.n, g.oh, g.ow, g.c, g.kh, g.kw))
    assert floats >= g.kh * g.kw * g.c and floats == depthwise.wgrad_workspace(
        g.n, g.oh, g.ow, g.c, g.kh, g.kw, "cuda").numel()
    gws = NH.Guarded(None, "cuda", torch.float32, (floats,))
    assert _call("mdtf_dwconv_fwd", _p(gx), _p(gw), _p(gy), *ints) == 0
    NH.assert_contained("dwconv_fwd", [gx, gw], [gy])
    assert _call("mdtf_dwconv_dgrad", _p(gdy), _p(gw), _p(gdx), *ints) == 0
    NH.assert_contained("dwconv_dgrad", [gdy, gw], [gdx])
    assert _call("mdtf_dwconv_wgrad", _p(gx), _p(gdy), _p(gws), *ints) == 0
    NH.assert_contained("dwconv_wgrad", [gx, gdy], [gws])
    gws.before = gws.buf.clone()                       # now an input: the finalize must leave the partials alone
    if accumulate is None:
        gdw = NH.Guarded(None, "cuda", torch.float32, case.w.shape)
    else:
        gdw = NH.Guarded(accumulate, "cuda")
    assert _call("mdtf_dwconv_wgrad_finalize", _p(gws), _p(gdw), g.n, g.oh, g.ow, g.c, g.kh, g.kw,
                 int(accumulate is not None)) == 0
    NH.assert_contained("dwconv_wgrad_finalize", [gws], [gdw])
    return gy.t.clone(), gdx.t.clone(), gdw.t.clone(), floats


# ================================================================================================== the oracle
def test_geometry_restated():
    g = _case(1).geo                                   # 8x8, 3x3 / 2 SAME: pads (0, 1)
    assert (g.oh, g.ow, g.pt, g.pb, g.pl, g.pr) == (4, 4, 0, 1, 0, 1)
    g = _case(2).geo                                   # 9x9, 5x5 / 2 SAME
    assert (g.oh, g.ow, g.pt, g.pb) == (5, 5, 2, 2)
    g = _case(7).geo                                   # 9x9, 3x3 dilation 2: effective 5x5
    assert (g.oh, g.ow, g.pt, g.pb) == (9, 9, 2, 2)
    g = _case(3).geo
    assert (g.oh, g.ow, g.pt, g.pl) == (3, 9, 0, 0)


@pytest.mark.parametrize("i", [1, 2, 5, 6, 7], ids=[CASE_IDS[i] for i in (1, 2, 5, 6, 7)])
def test_oracle_matches_the_definition(i):
    """The sliced tap loops against the definition evaluated one output pixel at a time, and dx / dw against autograd
    through that fp64 expression."""
    c = _case(i)
    x = c.x.double().requires_grad_(True)
    w = c.w.double().requires_grad_(True)
    y = DH.brute_fwd(x, w, c.geo)
    assert torch.allclose(y.detach(), c.y, rtol=1e-13, atol=1e-13)
    dx, dw = torch.autograd.grad((y * c.dy.double()).sum(), (x, w))
    assert torch.allclose(dx, c.dx, rtol=1e-13, atol=1e-13)
    assert torch.allclose(dw, c.dw, rtol=1e-13, atol=1e-13)


# ============================================================================================= geometry cases
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_geometry_case(i, device):
    device = _device(device)
    case = _case(i)
    y, dx, dw = _public(device, case)
    _check("case %s %s" % (CASE_IDS[i], device), device, case, y, dx, dw)
    if device == "cuda":
        ry, rdx, rdw, _ = _raw(case)
        assert NH.bits_equal(ry, y) and NH.bits_equal(rdx, dx), "entry points and autograd wrapper disagree"
        _check("case %s raw" % CASE_IDS[i], device, case, ry, rdx, rdw)
        assert NH.bits_equal(rdw, dw)                  # 0 + dw in fp64, rounded once: the stored value


@pytest.mark.parametrize("device", DEVICES)
def test_weight_gradient_adds_into_a_filled_slot(device):
    device = _device(device)
    case = _case(0)
    slot0 = NH.randn(case.w.shape, 7, 4.0)
    y, dx, dw = _public(device, case, slot0=slot0)
    _check("slot " + device, device, case, y, dx, dw, slot0=slot0)
    if device == "cuda":
        _, _, rdw, _ = _raw(case, accumulate=slot0)
        assert NH.bits_equal(rdw, dw)


@pytest.mark.parametrize("device", GPU_ONLY)
def test_weight_gradient_sums_across_chunks(device):
    """More than two chunks of output pixels and a ragged last one: the finalize's cross-chunk sum."""
    device = _device(device)
    from mdtf.ops import depthwise
    c, k = 8, 3
    side = 8
    while True:                                        # the plan depends on the sizes: search with the code's own
        chunk = depthwise.wgrad_chunk(1, side, side, c, k, k)
        assert chunk > 0
        if side * side > 2 * chunk and (side * side) % chunk:
            break
        side += 1
        assert side < 512
    case = _Case((1, side, side, c), (k, k), 1, 1, "SAME", 900)
    ry, rdx, rdw, floats = _raw(case)
    assert floats >= 3 * k * k * c, "fewer than 3 partials: %d floats" % floats
    assert floats == -(-side * side // chunk) * k * k * c
    _check("chunks %dx%d" % (side, side), device, case, ry, rdx, rdw)
    y, dx, dw = _public(device, case)
    assert NH.bits_equal(ry, y) and NH.bits_equal(rdx, dx) and NH.bits_equal(rdw, dw)


# ==================================================================================================== fallback
def _fallback_check(what, device, case, fp32_in=False):
    """The PyTorch expression: y against the oracle (channel order c * mult + m included); dx and dw where the
    arithmetic is fp32 end to end."""
    g = case.geo
    dev_in = "cpu" if fp32_in else device                # put(..., "cpu") keeps fp32
    xd = NH.put(case.x, dev_in).to(device).requires_grad_(True)
    wd = NH.put(case.w, dev_in).to(device).requires_grad_(True)
    y = ops.depthwise_conv2d(xd, wd, g.sh, g.padding)
    assert tuple(y.shape) == (g.n, g.oh, g.ow, g.c * case.mult) and y.dtype == xd.dtype
    bf = y.dtype == torch.bfloat16
    NH.check_bound(y, case.y, DH.y_bound(case.y, case.y_abs, case.y_cnt, bf), what + " y")
    if device == "cpu":
        y.backward(case.dy)
        NH.check_bound(xd.grad, case.dx, DH.y_bound(case.dx, case.dx_abs, case.dx_cnt, False), what + " dx")
        NH.check_bound(wd.grad, case.dw, DH.dw_bound(case.dw_abs, g), what + " dw")


@pytest.mark.parametrize("device", DEVICES)
def test_fallback_channels_not_a_multiple_of_8(device):
    device = _device(device)
    _fallback_check("C=12 " + device, device, _Case((2, 7, 7, 12), (3, 3), 1, 1, "SAME", 300))


@pytest.mark.parametrize("device", DEVICES)
def test_fallback_channel_multiplier(device):
    device = _device(device)
    case = _Case((2, 6, 6, 8), (3, 3), 2, 1, "SAME", 310, mult=2)
    _fallback_check("mult=2 " + device, device, case)
    # output channel c * mult + m is input channel c with filter [:, :, c, m]: one (c, m) at a time
    c, m = 5, 1
    w1 = torch.zeros_like(case.w)
    w1[:, :, c, m] = case.w[:, :, c, m]
    y = ops.depthwise_conv2d(NH.put(case.x, device), NH.put(w1, device), 2, "SAME").float().cpu()
    others = [ch for ch in range(16) if ch != c * 2 + m]
    assert float(y[..., others].abs().max()) == 0.0 and float(y[..., c * 2 + m].abs().max()) > 0.0


@pytest.mark.parametrize("device", GPU_ONLY)
def test_fallback_fp32_input_on_the_gpu(device):
    device = _device(device)
    _fallback_check("fp32 cuda", device, _case(0), fp32_in=True)


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("bad", ["channels", "taps", "misaligned"])
def test_entry_points_refuse_before_any_launch(bad, device):
    """MDTF_EINVAL for C = 12, kh * kw = 50 and a misaligned pointer: nothing is written."""
    device = _device(device)
    shape, k = ((1, 6, 6, 12), (3, 3)) if bad == "channels" else ((1, 12, 12, 8), (5, 10)) if bad == "taps" else (
        (1, 6, 6, 8), (3, 3))
    g = DH.Geo(shape, k, 1, 1, "SAME")
    ints = g.ints()
    off = 1 if bad == "misaligned" else 0              # one bf16 element: 2 bytes past a 16-byte boundary

    def guarded(shp, dtype, extra=0):
        n = 1
        for s in shp:
            n *= s
        return NH.Guarded(NH.randn((n + extra,), 5).to(dtype), "cuda")
    gx = guarded(shape, torch.bfloat16, off)
    gw = guarded((k[0], k[1], g.c, 1), torch.bfloat16)
    gdy = guarded((g.n, g.oh, g.ow, g.c), torch.bfloat16)
    gy = guarded((g.n, g.oh, g.ow, g.c), torch.bfloat16)
    gdx = guarded(shape, torch.bfloat16, off)
    gws = guarded((4 * k[0] * k[1] * g.c,), torch.float32)
    gdw = guarded((k[0], k[1], g.c, 1), torch.float32)
    px = _native.ptr(gx.t[off:])
    pdx = _native.ptr(gdx.t[off:])
    assert _call("mdtf_dwconv_fwd", px, _p(gw), _p(gy), *ints) == EINVAL
    assert _call("mdtf_dwconv_dgrad", _p(gdy), _p(gw), pdx, *ints) == EINVAL
    assert _call("mdtf_dwconv_wgrad", px, _p(gdy), _p(gws), *ints) == EINVAL
    if bad != "misaligned":
        assert _native.fn("mdtf_dwconv_wgrad_ws")(g.n, g.oh, g.ow, g.c, g.kh, g.kw) == 0
        assert _call("mdtf_dwconv_wgrad_finalize", _p(gws), _p(gdw), g.n, g.oh, g.ow, g.c, g.kh, g.kw, 0) == EINVAL
    for b in (gx, gw, gdy, gy, gdx, gws, gdw):
        assert b.unchanged()
    # a geometry whose output size does not follow from the rest
    if bad == "misaligned":
        wrong = list(ints)
        wrong[4] += 1
        assert _call("mdtf_dwconv_fwd", _p(gx), _p(gw), _p(gy), *wrong) == EINVAL
        assert gy.unchanged()


# ================================================================================================== API errors
def test_api_errors():
    x = torch.zeros(1, 6, 6, 8)
    w = torch.zeros(3, 3, 8, 1)
    with pytest.raises(ValueError):
        mdtf.nn.depthwise_conv2d(x, torch.zeros(3, 3, 4, 1), 1, "SAME")              # channel mismatch
    with pytest.raises(ValueError):
        mdtf.nn.depthwise_conv2d(x, w, 1, "SAME", rate=2, dilations=2)                # both
    with pytest.raises(ValueError):
        mdtf.nn.depthwise_conv2d(x, w, 2, "SAME", rate=2)                             # TF's rule
    with pytest.raises(ValueError):
        mdtf.nn.depthwise_conv2d(x, w, [1, 1, 2, 1], "SAME", dilations=[1, 2, 1, 1])
    with pytest.raises(ValueError):
        mdtf.nn.depthwise_conv2d(x, w, 1, "SAME", data_format="NCHW")
    assert mdtf.nn.depthwise_conv2d(x, w, 1, "SAME", data_format="NHWC").shape == (1, 6, 6, 8)
    assert mdtf.nn.depthwise_conv2d(x, w, [1, 2, 2, 1], "VALID", rate=1).shape == (1, 2, 2, 8)
    assert mdtf.nn.depthwise_conv2d(x, w, 1, "SAME", rate=[2, 2]).shape == (1, 6, 6, 8)
    with pytest.raises(ValueError):
        mdtf.nn.separable_conv2d(x, w, torch.zeros(3, 3, 8, 4), 1, "SAME")            # pointwise not 1x1
    with pytest.raises(ValueError):
        mdtf.nn.separable_conv2d(x, w, torch.zeros(1, 1, 16, 4), 1, "SAME")           # depth != C * mult
    with pytest.raises(ValueError):
        mdtf.nn.separable_conv2d(x, w, torch.zeros(1, 1, 8, 4), 1, "SAME", data_format="NCHW")
    assert mdtf.nn.separable_conv2d(x, torch.zeros(3, 3, 8, 2), torch.zeros(1, 1, 16, 4), 1, "SAME").shape == (
        1, 6, 6, 4)


# ============================================================================================ separable_conv2d
@pytest.mark.parametrize("device", DEVICES)
def test_separable_is_depthwise_then_pointwise(device):
    device = _device(device)
    case = _Case((2, 8, 8, 16), (3, 3), 1, 1, "SAME", 400)
    pw = NH.randn((1, 1, 16, 16), 403, 0.25)
    xd, wd, pd = NH.put(case.x, device), NH.put(case.w, device), NH.put(pw, device)
    got = ops.separable_conv2d(xd, wd, pd, [1, 1, 1, 1], "SAME")
    mid = ops.depthwise_conv2d(xd, wd, 1, "SAME")
    assert NH.bits_equal(got, ops.conv2d(mid, pd, 1, "VALID"))
    pw64 = pw.double()[0, 0]
    if device == "cpu":
        # the depthwise bound through the 1x1, then the 1x1's own sum of C = 16 terms
        e1 = gamma(case.y_cnt)[None, :, :, None] * case.y_abs
        ref = case.y @ pw64
        acc = e1 @ pw64.abs() + gamma(16) * ((case.y.abs() + e1) @ pw64.abs())
        NH.check_bound(got, ref, NH.out_bound(ref, acc, False), "separable cpu")
    else:
        assert mid.dtype == torch.bfloat16
        NH.check_neighbour(got, NH.round_bf16(case.y) @ pw64, "separable cuda")


# =========================================================================================== gradient plumbing
def _plumbing_model(rec):
    from mdtf.layers import tools
    from mdtf.runtime import Model
    from mdtf.train import variables as V

    class M(Model):
        def inference(self, x):
            store = V.get_store()
            if store.compute_dtype is not None:
                x = x.to(store.compute_dtype)
            y = tools.depthwise_conv_nonacti("dw1", x, 16)
            if y.requires_grad:
                rec["x"] = x.detach()
                y.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
            y = tools.batch_norm(y, training=True, relu=True)
            y = tools.separable_conv("sep", y, 16, 32)
            y = ops.global_avg_pool(y)
            return tools.dense("logits", y, 16)
    return M()


@pytest.mark.parametrize("device", DEVICES)
def test_gradient_reaches_the_fp32_slot(device):
    """A small net through one engine step: the depthwise variable's fp32 gradient slot holds the oracle's dw for
    the dy that reached the op; a second step on the same inputs (learning rate 0) gives the same bits again."""
    device = _device(device)
    from mdtf.models import SoftmaxCrossEntropyLoss
    from mdtf.runtime import Net, Tower
    from mdtf.train import variables as V
    store = V.get_store()
    store.device = torch.device(device)
    store.compute_dtype = torch.bfloat16 if device == "cuda" else None
    store.generator.manual_seed(11)
    x = NH.randn((2, 8, 8, 16), 500)
    labels = torch.tensor([3, 6])
    xp = mdtf.placeholder(torch.float32, [None, 8, 8, 16])
    yp = mdtf.placeholder(torch.int64, [None])
    opt = mdtf.train.GradientDescentOptimizer(0.0)
    rec, tg = {}, []
    t = Tower(Net(_plumbing_model(rec)), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), opt, batch_size=2)
    _, loss, _ = t.process()
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    names = [v.name for v in store.trainable_variables()]
    assert "dw1/depthwise_weights" in names and "sep/depthwise_weights" in names
    assert "sep/pointwise_weights" in names and "sep/biases" in names
    var = store.vars["dw1/depthwise_weights"]
    slots = []
    for _ in range(2):
        rec.clear()
        sess.run([op, loss], feed_dict={xp: x, yp: labels})
        assert var.grad.dtype == torch.float32 and tuple(var.grad.shape) == (3, 3, 16, 1)
        slots.append((var.grad.detach().clone(), rec["dy"], rec["x"]))
    grad, dy, xin = slots[0]
    assert float(dy.float().abs().max()) > 0.0
    geo = DH.Geo((2, 8, 8, 16), (3, 3), 1, 1, "SAME")
    dw, sabs = DH.wgrad_ref(xin.double().cpu(), dy.double().cpu(), geo)
    NH.check_bound(grad, dw, DH.dw_bound(sabs, geo), "slot " + device)
    assert NH.bits_equal(slots[1][1], dy), "the second step saw another dy"
    assert NH.bits_equal(slots[1][0], grad), "the second step's slot differs: a stale accumulate"


def _distinct_bf16(shape, seed):
    """bf16-representable values, all distinct (no ties for a max pool), in random order."""
    n = 1
    for s in shape:
        n *= s
    bits = (0x3000 + torch.arange(n, dtype=torch.int32)).to(torch.int16)
    vals = bits.view(torch.bfloat16).float()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return vals[perm].reshape(shape)


def _small_ints(shape, seed, hi):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=gen).float()


@pytest.mark.parametrize("device", GPU_ONLY)
def test_fanned_out_input_gradient(device, monkeypatch):
    """One max-pool output (it carries an act-grad sink) feeds a depthwise conv and a dense conv: the pool's input
    gradient equals the MDTF_KERNELS=torch run's.  Filters and upstream gradients are small integers, so both
    contributions and their sum are exact in bf16 on either path."""
    device = _device(device)
    x0 = _distinct_bf16((2, 12, 12, 16), 600)
    dwf, wf = _small_ints((3, 3, 16, 1), 601, 1), _small_ints((3, 3, 16, 16), 602, 1) * (
        torch.rand((3, 3, 16, 16), generator=torch.Generator().manual_seed(603)) < 0.25)
    g1, g2 = _small_ints((2, 6, 6, 16), 604, 1), _small_ints((2, 6, 6, 16), 605, 1)

    def run():
        xd = x0.to(device).bfloat16().requires_grad_(True)
        a = ops.max_pool(xd, 3, 2, "SAME")
        y1 = ops.depthwise_conv2d(a, dwf.to(device).bfloat16(), 1, "SAME")
        y2 = ops.conv2d(a, wf.to(device).bfloat16(), 1, "SAME")
        torch.autograd.backward([y1, y2], [g1.to(device).bfloat16(), g2.to(device).bfloat16()])
        return xd.grad.detach().clone()
    native = run()
    monkeypatch.setenv("MDTF_KERNELS", "torch")
    stock = run()
    monkeypatch.setenv("MDTF_KERNELS", "native")
    assert float(native.float().abs().max()) > 1.0
    d = (NH._ordered(native.cpu()) - NH._ordered(stock.cpu())).abs()
    assert int(d.max()) <= 1, "%d elements differ by more than a bf16 neighbour" % int((d > 1).sum())
    # and both contributions are in it: against the oracle of the sum
    geo = DH.Geo((2, 6, 6, 16), (3, 3), 1, 1, "SAME")
    a64 = torch.nn.functional.max_pool2d(torch.nn.functional.pad(x0.permute(0, 3, 1, 2), (0, 1, 0, 1),
                                                                 value=float("-inf")), 3, 2, return_indices=True)
    da = DH.dgrad_ref(g1.double(), dwf.double(), geo)[0]
    for o in range(16):                                 # the dense conv's data gradient: 16 depthwise-shaped terms
        da += DH.dgrad_ref(g2.double()[..., o:o + 1].expand(-1, -1, -1, 16), wf.double()[:, :, :, o:o + 1], geo)[0]
    idx = a64[1]                                        # [N, C, 6, 6] flat indices into the padded 13 x 13 plane
    want = torch.zeros(2, 16, 13 * 13, dtype=torch.float64)
    want.scatter_add_(2, idx.reshape(2, 16, -1), da.permute(0, 3, 1, 2).reshape(2, 16, -1))
    want = want.reshape(2, 16, 13, 13)[:, :, :12, :12].permute(0, 2, 3, 1)
    assert torch.equal(native.double().cpu(), want)


# ==================================================================================== determinism and capture
@pytest.mark.parametrize("device", GPU_ONLY)
def test_bitwise_repeatable_and_replays_in_a_graph(device):
    device = _device(device)
    case = _case(9)
    g = case.geo
    xd = NH.put(case.x, device).requires_grad_(True)
    wd = NH.put(case.w, device).requires_grad_(True)
    dyd = NH.put(case.dy, device)
    slot = torch.zeros(case.w.shape, device=device)
    wd._mdtf_var = _Slot(slot)

    def step():
        xd.grad = None
        slot.zero_()
        y = ops.depthwise_conv2d(xd, wd, g.sh, g.padding)
        y.backward(dyd)
        return y.detach(), xd.grad

    def snap(out):
        torch.cuda.synchronize()
        return out[0].clone(), out[1].clone(), slot.clone()
    first, second = snap(step()), snap(step())
    _check("case 9 eager", device, case, *first)
    for a, b in zip(first, second):
        assert NH.bits_equal(a, b), "two eager runs differ"
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
    for _ in range(2):
        slot.fill_(float("nan"))
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        for a, b in zip(first, snap(out)):
            assert NH.bits_equal(a, b), "a replay differs from the eager run"
    del graph
    assert math.isfinite(float(slot.sum()))
