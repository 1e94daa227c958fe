"""``mdtf.nn.conv2d(..., groups=G)``, the kernels of ``csrc/conv_group.hip`` and the ResNeXt models against the fp64
oracle of ``conv_group_helpers``, element by element, at the smallest shapes at which the index arithmetic can still be
wrong.  ``cpu`` runs the PyTorch expression on fp32 tensors of bf16-representable values (it validates the oracle and
the bounds); ``cuda`` runs the HIP kernels on bf16 tensors, the weight gradient landing in an fp32 slot.  The bounds
are derived in ``conv_group_helpers``.
"""
import functools
import os
import sys

import pytest
import torch

import mdtf
from mdtf.ops import _native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_group_helpers as GH  # noqa: E402
import nhwc_helpers as NH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
UNSUPPORTED = -2

#        name                  N  H     W   C    Cg  k  s  padding
CASES = [("1_7x7x32_g8",      (2, 7,    7,  32), 4,  3, 1, "SAME"),
         ("2_5x17x32_cg16",   (1, 5,    17, 32), 16, 3, 1, "SAME"),
         ("3_6x6x64_dense",   (2, 6,    6,  64), 32, 3, 1, "VALID"),
         ("4_8x8x64_s2",      (2, 8,    8,  64), 8,  3, 2, "SAME"),
         ("5_9x9x32_s2",      (1, 9,    9,  32), 4,  3, 2, "SAME"),
         ("6_2x2x32",         (1, 2,    2,  32), 32, 3, 1, "SAME"),
         ("7_three_bands",    (1, None, 20, 32), 8,  3, 1, "SAME"),
         ("8_13x13x32_s2_explicit", (3, 13, 13, 32), 16, 3, 2, (2, 1, 2, 1)),
         ("cg2_fallback",     (2, 6,    6,  32), 2,  3, 1, "SAME"),
         ("5x5_fallback",     (1, 7,    7,  32), 8,  5, 1, "SAME")]
CASE_IDS = [c[0] for c in CASES]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _pads(n, k, s, padding):
    """One axis of TF's geometry: (out, pad_before, pad_after)."""
    if padding == "SAME":
        out = -(-n // s)
        total = max((out - 1) * s + k - n, 0)
        return out, total // 2, total - total // 2
    before, after = (0, 0) if padding == "VALID" else padding
    return (n + before + after - k) // s + 1, before, after


def _ints(shape, cg, k, s, pads, oh, ow):
    n, h, w, c = shape
    return [n, h, w, c, cg, oh, ow, k, k, s, 1] + list(pads)


class _Case(object):
    """Inputs (bf16-representable fp32) and the oracle of one geometry, computed once and left unchanged."""

    def __init__(self, shape, cg, k, s, padding, seed):
        n, h, w, c = shape
        self.shape, self.cg, self.k, self.s, self.padding, self.groups = shape, cg, k, s, padding, c // cg
        self.oh, pt, pb = _pads(h, k, s, padding if isinstance(padding, str) else padding[:2])
        self.ow, pl, pr = _pads(w, k, s, padding if isinstance(padding, str) else padding[2:])
        self.pads = (pt, pb, pl, pr)
        self.x = NH.randn(shape, seed)
        self.w = NH.randn((k, k, cg, c), seed + 1, 0.5)
        self.dy = NH.randn((n, self.oh, self.ow, c), seed + 2)
        self.ref = GH.Oracle(self.x, self.w, self.dy, self.groups, s, self.pads)
        self.ints = _ints(shape, cg, k, s, self.pads, self.oh, self.ow)


@functools.lru_cache(maxsize=None)
def _case(i, device):
    _, shape, cg, k, s, padding = CASES[i]
    if shape[1] is None:                               # more than two row bands of the forward kernel
        band = 16
        if device == "cuda":
            from mdtf.ops import grouped
            band = grouped.band(_ints((1, 1024, 20, 32), cg, k, s, (1, 1, 1, 1), 1024, 20))
            assert 0 < band and grouped.band(_ints((1, 2 * band + 3, 20, 32), cg, k, s, (1, 1, 1, 1), 2 * band + 3,
                                                   20)) <= band
        shape = (shape[0], 2 * band + 3) + shape[2:]
    return _Case(shape, cg, k, s, padding, 100 + 10 * i)


class _Slot(object):
    """What ``variables.grad_sink`` looks for: an fp32 gradient slot."""

    def __init__(self, grad):
        self.grad = grad


def _public(device, case, slot0=None):
    """forward + backward through ``mdtf.nn.conv2d(groups=G)``.  cuda: the weight gradient lands in an fp32 slot
    (pre-filled with ``slot0`` or zeros), cpu: in ``w.grad``."""
    xd = NH.put(case.x, device).requires_grad_(True)
    wd = NH.put(case.w, device).requires_grad_(True)
    slot = None
    if device == "cuda":
        slot = (slot0.to(device) if slot0 is not None else torch.zeros(case.w.shape, device=device)).contiguous()
        wd._mdtf_var = _Slot(slot)
    y = mdtf.nn.conv2d(xd, wd, [1, case.s, case.s, 1], case.padding, groups=case.groups)
    y.backward(NH.put(case.dy, device))
    return y.detach(), xd.grad, (wd.grad if slot is None else slot)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("i", range(8), ids=CASE_IDS[:8])
def test_geometry_case(i, device):
    device = _device(device)
    case = _case(i, device)
    y, dx, dw = _public(device, case)
    assert y.dtype == (torch.bfloat16 if device == "cuda" else torch.float32) and dx.dtype == y.dtype
    assert dw.dtype == torch.float32
    case.ref.check("%s %s" % (CASE_IDS[i], device), y, dx, dw, device == "cuda")


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("i", [3, 6], ids=[CASE_IDS[3], CASE_IDS[6]])
def test_weight_gradient_adds_into_a_filled_slot_and_repeats(i, device):
    """``+=`` into a non-zero slot over at least two partials, and two runs give the same bits."""
    device = _device(device)
    from mdtf.ops import grouped
    case = _case(i, device)
    n, oh, ow = case.shape[0], case.oh, case.ow
    assert 0 < grouped.wgrad_chunk(case.ints) < n * oh * ow
    assert grouped.wgrad_workspace(case.ints, device).numel() >= 2 * case.w.numel()
    slot0 = NH.randn(case.w.shape, 7, 4.0)
    _, _, dw = _public(device, case, slot0=slot0)
    case.ref.check("slot %s" % CASE_IDS[i], None, None, dw, True, slot0=slot0)
    assert NH.bits_equal(_public(device, case, slot0=slot0)[2], dw)


@pytest.mark.parametrize("device", GPU_ONLY)
@pytest.mark.parametrize("i", [8, 9], ids=CASE_IDS[8:])
def test_entry_points_refuse(i, device):
    """Two channels per group and a 5x5 filter: MDTF_EUNSUPPORTED from every launcher."""
    device = _device(device)
    from mdtf.ops import grouped  # noqa: F401  (registers the signatures)
    case = _case(i, device)
    x, w, dy = (NH.put(t, device) for t in (case.x, case.w, case.dy))
    out, ws = torch.zeros_like(x), torch.zeros(4096, device=device)
    for name, a, b, c in (("mdtf_gconv_fwd", x, w, dy), ("mdtf_gconv_dgrad", dy, w, out), ("mdtf_gconv_wgrad", x, dy, ws)):
        rc = _native.fn(name)(_native.ptr(a), _native.ptr(b), _native.ptr(c), *case.ints, _native.stream_ptr())
        assert rc == UNSUPPORTED, name


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("i", [8, 9], ids=CASE_IDS[8:])
def test_fallback_meets_the_oracle(i, device):
    """The same calls through ``conv2d(groups=G)``: the PyTorch expression.  y on both devices; dx and dw where the
    arithmetic is fp32 end to end."""
    device = _device(device)
    case = _case(i, device)
    if device == "cpu":
        y, dx, dw = _public(device, case)
    else:
        y, dx, dw = mdtf.nn.conv2d(NH.put(case.x, device), NH.put(case.w, device), case.s, case.padding,
                                   groups=case.groups), None, None
    case.ref.check("%s %s" % (CASE_IDS[i], device), y, dx, dw, device == "cuda")


def test_groups_1_is_the_present_path_and_bad_groups_raise():
    x, w = NH.randn((2, 6, 6, 8), 1), NH.randn((3, 3, 8, 12), 2)
    b = NH.randn((12,), 3)
    assert torch.equal(mdtf.nn.conv2d(x, w, 2, "SAME", bias=b, act="relu", groups=1),
                       mdtf.nn.conv2d(x, w, 2, "SAME", bias=b, act="relu"))
    for groups, cg in ((3, 2), (5, 2), (0, 8)):         # 3 divides Cout only, 5 neither, 0 nothing
        with pytest.raises(ValueError):
            mdtf.nn.conv2d(x, NH.randn((3, 3, cg, 12), 4), 1, "SAME", groups=groups)
    with pytest.raises(ValueError):
        mdtf.nn.conv2d(x, w, 1, "SAME", groups=2)        # the filter's input count is not C / groups
    y = mdtf.nn.conv2d(x, NH.randn((3, 3, 4, 12), 5), 1, "SAME", bias=b, act="relu", groups=2)
    assert tuple(y.shape) == (2, 6, 6, 12) and float(y.min()) >= 0.0


def test_resnext50_builds_and_trains_on_cpu_beside_an_unchanged_resnet50():
    from mdtf.models import ResNet, ResNeXt50_32x4d, SoftmaxCrossEntropyLoss
    from mdtf.runtime import Net, Tower
    from mdtf.train import step as S
    from mdtf.train import variables as V

    def build(model):
        V.reset_default_graph()
        S.reset()
        store = V.get_store()
        store.device, store.compute_dtype = torch.device("cpu"), None
        store.generator.manual_seed(3)
        xp, yp = mdtf.placeholder(torch.float32, [None, 64, 64, 3]), mdtf.placeholder(torch.int64, [None])
        opt, tg = mdtf.train.GradientDescentOptimizer(0.0), []
        tower = Tower(Net(model), "tower_0/", tg, xp, yp, SoftmaxCrossEntropyLoss(), opt, batch_size=2)
        _, loss, logits = tower.process()
        op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
        return store, xp, yp, op, loss, logits

    store, xp, yp, op, loss, logits = build(ResNeXt50_32x4d())
    shapes = {v.name: tuple(v.shape) for v in store.trainable_variables()}
    for stage, (cg, c) in enumerate(((4, 128), (8, 256), (16, 512), (32, 1024)), 1):
        assert shapes["resnext_50_32x4d/block%d/unit_1/conv2/weights" % stage] == (3, 3, cg, c)
    assert shapes["resnext_50_32x4d/block1/unit_1/conv3/weights"] == (1, 1, 128, 256)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    _, lv, lg = sess.run([op, loss, logits], feed_dict={xp: NH.randn((2, 64, 64, 3), 9), yp: torch.tensor([1, 7])})
    assert tuple(lg.shape) == (2, 1000) and torch.isfinite(torch.as_tensor(lv)).all()
    for v in store.trainable_variables():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), v.name

    store = build(ResNet(50))[0]
    shapes = {v.name: tuple(v.shape) for v in store.trainable_variables()}
    assert len(shapes) == 161
    assert shapes["resnet_v1_50/block1/unit_1/conv2/weights"] == (3, 3, 64, 64)
    assert shapes["resnet_v1_50/block1/unit_1/conv1/weights"] == (1, 1, 64, 64)
    assert shapes["resnet_v1_50/block4/unit_3/conv2/weights"] == (3, 3, 512, 512)
    assert shapes["resnet_v1_50/block2/unit_1/shortcut/weights"] == (1, 1, 256, 512)
    assert shapes["resnet_v1_50/logits/kernel"] == (2048, 1000)
