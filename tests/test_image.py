"""``mdtf.image`` (``mdtf.ops.image`` / ``csrc/image.hip``): the copy path bit for bit, per-image standardization from
exact integer sums, the bilinear path against an fp64 oracle under a derived bound, the device-drawn boxes and flips
against the integer mirror of the hash, hipGraph replay, the TF-named ops and a LeNet step that preprocesses uint8
images inside the step program.

Kernel tests take a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.image``, ``cuda`` the HIP kernels.  The
oracles (``image_helpers``) are numpy, written from the definitions in ``mdtf.ops.image``'s docstring.
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

import mdtf
from mdtf import image as I
from mdtf.ops import image as OI

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_helpers as IH  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
BF, FP, U8 = torch.bfloat16, torch.float32, torch.uint8


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from mdtf.ops import _native
        _native.lib()
        assert _native.mode() != "torch"
    return device


@contextlib.contextmanager
def _counter(device, value):
    """The device step counter the draws are mixed with, set to ``value`` and put back afterwards."""
    from mdtf.train.graph import rng_offset_tensor
    dev = torch.device("cuda", torch.cuda.current_device()) if device == "cuda" else torch.device("cpu")
    t = rng_offset_tensor(dev)
    before = t.clone()
    t.fill_(value)
    try:
        yield t
    finally:
        t.copy_(before)


def _dev_boxes(rows, device):
    return torch.tensor(np.asarray(rows), dtype=torch.int32, device=device)


def test_counter_layout_is_the_documented_one():
    assert (OI.K_CROP_Y, OI.K_CROP_X, OI.K_FLIP, OI.K_ATTEMPT) == (IH.K_CROP_Y, IH.K_CROP_X, IH.K_FLIP, IH.K_ATTEMPT)
    for line in ("k = 0             crop row offset", "k = 1             crop column offset",
                 "k = 2             flip", "k = 4 + 4a + 0    attempt a: area fraction"):
        assert line in OI.__doc__


# ------------------------------------------------------------------------------------------------------ copy path
# (B, H, W, C) -> (OH, OW): rows of 63 bytes (nothing aligned) | one channel, the whole image | four channels |
# several blocks per image | 45 outputs per image: every 8-group is partial or shared with a neighbour | C = 3 whole
COPY_SHAPES = [((3, 20, 21, 3), (16, 16)), ((2, 9, 9, 1), (9, 9)), ((2, 12, 10, 4), (8, 6)),
               ((2, 70, 90, 3), (64, 64)), ((1, 5, 7, 3), (3, 5)), ((5, 32, 32, 3), (32, 32))]
MEAN, STD = (123.68, 116.78, 103.94, 99.5), (58.393, 57.12, 57.375, 0.3)


def _copy_id(s):
    return "%dx%dx%dx%d-%dx%d" % (s[0] + s[1])


def _check_copy(device, img, view, boxes, flips, OH, OW, scaled):
    C = img.shape[3]
    want_u8 = IH.copy_values(img, boxes, flips, OH, OW)
    db, df = _dev_boxes(boxes, device), torch.tensor(flips, dtype=torch.int32, device=device)
    if scaled:
        mean, inv = IH.channel_scale(MEAN[:C], STD[:C])
        kw = dict(mean=MEAN[:C], std=STD[:C])
    else:
        mean, inv, kw = np.zeros(C, np.float32), np.ones(C, np.float32), {}
    want = IH.f32_scale(want_u8, mean, inv)
    got = I.transform(view, (OH, OW), boxes=db, flips=df, dtype=FP, **kw)
    assert got.dtype == FP and got.shape == want.shape and not got.requires_grad
    assert np.array_equal(IH.bits(got), want.view(np.int32)), "fp32 %s" % (boxes,)
    got = I.transform(view, (OH, OW), boxes=db, flips=df, dtype=BF, **kw)
    assert got.dtype == BF and np.array_equal(IH.bits(got), IH.bf16_bits(want)), "bf16 %s" % (boxes,)
    if not scaled:
        got = I.transform(view, (OH, OW), boxes=db, flips=df, dtype=U8)
        assert got.dtype == U8 and np.array_equal(got.cpu().numpy(), want_u8), "uint8 %s" % (boxes,)


@pytest.mark.parametrize("scaled", [True, False], ids=["mean_std", "identity"])
@pytest.mark.parametrize("shape", COPY_SHAPES, ids=_copy_id)
@pytest.mark.parametrize("device", DEVICES)
def test_copy_path_is_exact(device, shape, scaled):
    """Boxes of the output size at each corner, at an odd x0, over the full image and hanging over each edge by 1 to
    4 pixels (zeros outside), flips 0, 1, 0, ...: fp32 bitwise the numpy mirror ``(float32(v) - mean) * inv``, bf16
    bitwise its round-to-nearest-even value, uint8 equal to the source."""
    device = _device(device)
    (B, H, W, C), (OH, OW) = shape
    img = IH.random_images(B, H, W, C, seed=H * W)
    view = torch.from_numpy(img).to(device)
    flips = [b & 1 for b in range(B)]
    seen_zero_pad = False
    for boxes in IH.corner_and_pad_boxes(B, H, W, OH, OW):
        _check_copy(device, img, view, boxes, flips, OH, OW, scaled)
        seen_zero_pad |= any(y < 0 or x < 0 or y + OH > H or x + OW > W for y, x, _, _ in boxes)
    assert seen_zero_pad


@pytest.mark.parametrize("device", DEVICES)
def test_copy_from_a_misaligned_view(device):
    """The images are bytes [5, 5 + n) of a buffer of 255s: the base is odd and any byte fetched from outside the
    view would show in a result whose own pixels are all below 200."""
    device = _device(device)
    B, H, W, C, OH, OW = 3, 20, 21, 3, 16, 16
    img = (IH.random_images(B, H, W, C, seed=77) % 200).astype(np.uint8)
    n = img.size
    buf = torch.full((n + 64,), 255, dtype=U8)
    buf[5:5 + n] = torch.from_numpy(img).reshape(-1)
    buf = buf.to(device)
    view = buf[5:5 + n].view(B, H, W, C)
    assert view.data_ptr() % 2 == 1 or device == "cpu"
    flips = [0, 1, 0]
    for boxes in IH.corner_and_pad_boxes(B, H, W, OH, OW):
        _check_copy(device, img, view, boxes, flips, OH, OW, scaled=False)
    # the resize path over boxes that touch the first and the last byte of the view
    boxes = [(0, 0, 20, 21), (0, 0, 7, 5), (9, 10, 11, 11)]
    want = IH.oracle_resize(img, np.asarray(boxes), flips, OH, OW, "legacy")
    got = I.transform(view, (OH, OW), boxes=_dev_boxes(boxes, device), flips=torch.tensor(flips), dtype=FP)
    tol = IH.resize_tolerance(want, boxes, 1.0, False)
    assert (np.abs(got.cpu().numpy() - want) <= tol).all() and want.max() < 200.0
    assert bool((buf[:5] == 255).all()) and bool((buf[5 + n:] == 255).all())


@pytest.mark.parametrize("device", DEVICES)
def test_long_rows_and_a_large_reduction(device):
    """A flipped copy out of 36000-byte rows (the offsets inside one image leave 16 bits far behind), and a 16-fold
    reduction whose single block reaches over 50 source rows of 2100 bytes."""
    device = _device(device)
    img = IH.random_images(1, 3, 12000, 3, seed=13)
    boxes, flips = [(1, 499, 2, 11000)], [1]
    _check_copy(device, img, torch.from_numpy(img).to(device), boxes, flips, 2, 11000, scaled=False)
    img = IH.random_images(1, 64, 700, 3, seed=14)
    rows = np.asarray([(0, 0, 64, 700)])
    want = IH.oracle_resize(img, rows, [0], 4, 4, "legacy")
    got = _resize(device, img, 4, 4, None, [0], "legacy", FP)
    assert (np.abs(got.cpu().numpy() - want) <= IH.resize_tolerance(want, rows, 1.0, False)).all()


# ------------------------------------------------------------------------------------------------ standardization
def _std_cases():
    g = IH.random_images(2, 12, 10, 3, seed=3)
    const = np.full((2, 9, 9, 1), 37, dtype=np.uint8)
    const[1] = 0
    white = np.full((1, 64, 64, 3), 255, dtype=np.uint8)
    odd = IH.random_images(3, 20, 21, 3, seed=4)
    return {"random": (g, None), "constant": (const, None), "all_255": (white, None),
            "padded_box": (odd, [(-2, -3, 20, 21), (4, 4, 20, 21), (0, 0, 20, 21)])}


@pytest.mark.parametrize("case", ["random", "constant", "all_255", "padded_box"])
@pytest.mark.parametrize("device", DEVICES)
def test_per_image_standardization(device, case):
    """fp32 bitwise the mirror built from the exact integer sums: fp64 mean and adj = max(stddev, 1 / sqrt(N)),
    {mean, 1 / adj} rounded to fp32, then a subtraction and a multiplication in fp32.  Against the plain fp64 formula
    the two fp32 constants and the two fp32 operations each contribute at most one relative 2^-24:
    |err| <= 4 * 2^-24 * (|v - mean| / adj + 1).  A constant image has adj = 1 / sqrt(N); 64 * 64 * 3 values of 255
    make every thread flush its 32-bit partial sums."""
    device = _device(device)
    img, boxes = _std_cases()[case]
    B, H, W, C = img.shape
    x = torch.from_numpy(img).to(device)
    if boxes is None:
        got = I.per_image_standardization(x)
        v = img
    else:
        got = I.transform(x, (H, W), boxes=_dev_boxes(boxes, device), standardize=True, dtype=FP)
        v = IH.copy_values(img, boxes, [0] * B, H, W)
        assert (v == 0).any()
    assert got.dtype == FP and got.shape == img.shape
    for b, (mean, adj) in enumerate(IH.oracle_stats(v)):
        want = IH.f32_scale(v[b], np.float32(mean), np.float32(1.0 / adj))
        assert np.array_equal(IH.bits(got[b]), want.view(np.int32)), (case, b)
        exact = (v[b].astype(np.float64) - mean) / adj
        err = np.abs(got[b].cpu().numpy().astype(np.float64) - exact)
        assert (err <= 4 * IH.U * (np.abs(exact) + 1.0)).all(), (case, b, float(err.max()))
        if case == "constant":
            assert adj == 1.0 / np.sqrt(81.0) and not got[b].any()
    if case == "all_255":
        assert IH.oracle_stats(v)[0][0] == 255.0


# ---------------------------------------------------------------------------------------------------- resize path
MAPPINGS = {"legacy": {}, "half_pixel": dict(half_pixel_centers=True), "align_corners": dict(align_corners=True)}
# (B, H, W, C) -> (OH, OW), boxes (None: the whole image), flips
RESIZE_SHAPES = {
    "up_down": ((2, 10, 13, 3), (16, 7), None, [0, 0]),
    "to_one": ((1, 7, 7, 1), (1, 1), None, [0]),
    "mixed": ((2, 40, 40, 3), (24, 24), [(3, 5, 24, 24), (1, 2, 37, 30)], [1, 1]),
    "mixed_b": ((2, 40, 40, 3), (24, 24), [(0, 0, 13, 40), (16, 16, 24, 24)], [0, 1]),
}


def _resize(device, img, OH, OW, boxes, flips, mapping, dtype, **scale):
    x = torch.from_numpy(img).to(device)
    db = None if boxes is None else _dev_boxes(boxes, device)
    return I.transform(x, (OH, OW), boxes=db, flips=torch.tensor(flips, dtype=torch.int32), dtype=dtype,
                       **dict(MAPPINGS[mapping], **scale))


@pytest.mark.parametrize("pattern", ["random", "checkerboard"])
@pytest.mark.parametrize("mapping", sorted(MAPPINGS))
@pytest.mark.parametrize("shape", sorted(RESIZE_SHAPES))
@pytest.mark.parametrize("device", DEVICES)
def test_resize_against_fp64(device, shape, mapping, pattern):
    """The oracle evaluates the definition in fp64 from the same fp32 scales.  The bound, with u = 2^-24 and n a bound
    on |in| (the box side plus one):

    * ``in = (o + 0.5?) * s - 0.5?`` is two fp32 roundings of magnitudes below n (one with a fused multiply-add), and
      ``t = in - floor(in)`` is exact for in >= 0 and one rounding of a value below 1 otherwise: d_in <= u (2 n + 1)
      per axis.  The interpolant is continuous and piecewise linear in ``in`` (across an integer the two taps swap
      roles at t = 0 / 1, and the clamps keep it constant outside the box) with a slope of at most the largest
      neighbour difference, 255: 255 * d_in per axis.
    * ``top`` and ``bot`` each take two roundings of magnitudes <= 255 (the differences of two pixels are exact) and
      enter the last lerp as a convex combination; the last lerp adds three more: at most 5, counted as 6, * 255 u.
    * the subtraction of the mean and the multiplication by ``inv`` scale all of that by |inv| and add two relative
      roundings of the result.

    tol = |inv| (2 * 255 d_in + 6 * 255 u) + 2 u |want|, plus half a bf16 ulp of the oracle value for bf16 output."""
    device = _device(device)
    (B, H, W, C), (OH, OW), boxes, flips = RESIZE_SHAPES[shape]
    img = IH.random_images(B, H, W, C, seed=H + W) if pattern == "random" else IH.checkerboard(B, H, W, C)
    rows = np.asarray(boxes if boxes is not None else [(0, 0, H, W)] * B)
    raw = IH.oracle_resize(img, rows, flips, OH, OW, mapping)
    mean, std = MEAN[:C], STD[:C]
    m32, i32 = IH.channel_scale(mean, std)
    for scaled in (False, True):
        want = (raw - m32.astype(np.float64)) * i32.astype(np.float64) if scaled else raw
        kw = dict(mean=mean, std=std) if scaled else {}
        inv = float(np.abs(i32).max()) if scaled else 1.0
        for dtype in (FP, BF):
            got = _resize(device, img, OH, OW, boxes, flips, mapping, dtype, **kw)
            assert got.dtype == dtype and tuple(got.shape) == (B, OH, OW, C)
            err = np.abs(got.float().cpu().numpy().astype(np.float64) - want)
            tol = IH.resize_tolerance(want, rows, inv, dtype == BF)
            worst = float((err / tol).max())
            print("%s %s %s %s scaled=%d: worst err / tol %.3f" % (shape, mapping, pattern, dtype, scaled, worst))
            assert worst <= 1.0
    assert raw.max() > raw.min() or shape == "to_one"


@pytest.mark.parametrize("pattern", ["random", "checkerboard"])
@pytest.mark.parametrize("device", DEVICES)
def test_resize_by_an_integer_factor_is_exact(device, pattern):
    """(16, 16) -> (8, 8) in the legacy mapping: scale 2, every t = 0, so the result is the source pixel."""
    device = _device(device)
    B, H, W, C = 2, 16, 16, 3
    img = IH.random_images(B, H, W, C, seed=5) if pattern == "random" else IH.checkerboard(B, H, W, C)
    got = _resize(device, img, 8, 8, None, [0, 1], "legacy", FP)
    want = img[:, ::2, ::2].astype(np.float32)
    want[1] = want[1][:, ::-1].copy()                                # flipped: output x reads source column 2 (7 - x)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(I.resize_bilinear(torch.from_numpy(img).to(device), (8, 8)).cpu().numpy(),
                          img[:, ::2, ::2].astype(np.float32))


# ----------------------------------------------------------------------------------------------------- parameters
COUNTERS = [0, 1, 2 ** 32 + 1]
CROPS = [(32, 32, 24, 28), (20, 21, 20, 5), (10, 64, 8, 64), (256, 256, 224, 224)]     # H == th; H - th + 1 == 3


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("seed", [1, 0x7FFFFFFE])
@pytest.mark.parametrize("device", DEVICES)
def test_boxes_and_flips_equal_the_integer_mirror(device, seed, counter):
    device = _device(device)
    B = 257
    with _counter(device, counter):
        for H, W, th, tw in CROPS:
            got = I.random_boxes(B, (H, W), (th, tw), seed=seed, device=device)
            assert got.dtype == torch.int32 and got.device.type == device
            want = IH.oracle_random_boxes(B, H, W, th, tw, seed, counter)
            assert np.array_equal(got.cpu().numpy(), want), (H, W, th, tw)
            assert want[:, 0].min() >= 0 and (want[:, 0] + th).max() <= H and (want[:, 1] + tw).max() <= W
        assert set(IH.oracle_random_boxes(B, 20, 21, 20, 5, seed, counter)[:, 0]) == {0}
        assert set(IH.oracle_random_boxes(B, 10, 64, 8, 64, seed, counter)[:, 0]) == {0, 1, 2}
        got = I.random_boxes(B, (32, 32), (32, 32), seed=seed, pad=4, device=device)
        want = IH.oracle_random_boxes(B, 32, 32, 32, 32, seed, counter, pad=4)
        assert np.array_equal(got.cpu().numpy(), want) and want[:, :2].min() == -4 and want[:, :2].max() == 4
        flips = I.random_flips(B, seed=seed, device=device)
        assert flips.dtype == torch.int32 and np.array_equal(flips.cpu().numpy(), IH.oracle_flips(B, seed, counter))


def test_mirror_depends_on_seed_and_counter():
    a = IH.oracle_random_boxes(257, 32, 32, 24, 28, 1, 0)
    assert (a != IH.oracle_random_boxes(257, 32, 32, 24, 28, 2, 0)).any()
    assert (a != IH.oracle_random_boxes(257, 32, 32, 24, 28, 1, 1)).any()
    assert (IH.oracle_flips(257, 1, 1) != IH.oracle_flips(257, 1, 2 ** 32 + 1)).sum() == 0        # 32-bit counter
    assert (IH.oracle_flips(257, 1, 0) != IH.oracle_flips(257, 1, 1)).any()


@pytest.mark.parametrize("device", DEVICES)
def test_draws_are_uniform(device):
    """B = 4096 draws from a fixed seed: the flip rate and each of 3 row offsets within 5 standard deviations of
    the binomial around 1/2 and 1/3."""
    device = _device(device)
    B = 4096
    with _counter(device, 0):
        flips = I.random_flips(B, seed=11, device=device).cpu().numpy()
        boxes = I.random_boxes(B, (10, 64), (8, 60), seed=11, device=device).cpu().numpy()
    assert abs(flips.mean() - 0.5) <= 5 * np.sqrt(0.25 / B), flips.mean()
    for off in range(3):
        p = (boxes[:, 0] == off).mean()
        assert abs(p - 1 / 3) <= 5 * np.sqrt((1 / 3) * (2 / 3) / B), (off, p)
    assert set(boxes[:, 1]) == set(range(5))


@pytest.mark.parametrize("image_size", [(64, 64), (50, 70)])
@pytest.mark.parametrize("device", DEVICES)
def test_distorted_boxes_properties(device, image_size):
    """Every box lies inside the image; with h, w the sides before rounding (each within half a pixel of the box's),
    h * w / (H * W) lies in the area range and w / h in the aspect range; same seed and counter, same boxes; another
    counter, other boxes; an impossible request falls back to the whole image."""
    device = _device(device)
    B, (H, W) = 4096, image_size
    area, aspect = (0.08, 1.0), (0.75, 1.3333)
    with _counter(device, 0) as t:
        got = I.distorted_boxes(B, (H, W), area, aspect, seed=21, device=device)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, 4)
        again = I.distorted_boxes(B, (H, W), area, aspect, seed=21, device=device)
        assert torch.equal(got, again)
        t.fill_(1)
        other = I.distorted_boxes(B, (H, W), area, aspect, seed=21, device=device)
        assert int((other != got).any(1).sum()) > B // 2
        whole = I.distorted_boxes(B, (64, 64), (1.0, 1.0), (2.0, 2.0), max_attempts=7, seed=21, device=device)
        assert np.array_equal(whole.cpu().numpy(), np.tile([0, 0, 64, 64], (B, 1)))
    y0, x0, bh, bw = (got.cpu().numpy()[:, i].astype(np.float64) for i in range(4))
    assert (y0 >= 0).all() and (x0 >= 0).all() and (bh >= 1).all() and (bw >= 1).all()
    assert (y0 + bh <= H).all() and (x0 + bw <= W).all()
    eps = 1e-5
    assert ((bh + 0.5) * (bw + 0.5) >= area[0] * H * W * (1 - eps)).all()
    assert ((bh - 0.5) * (bw - 0.5) <= area[1] * H * W * (1 + eps)).all()
    assert ((bw + 0.5) / (bh - 0.5) >= aspect[0] * (1 - eps)).all()
    assert ((bw - 0.5) / (bh + 0.5) <= aspect[1] * (1 + eps)).all()
    assert len(set(zip(bh, bw))) > 100 and len(set(y0)) > 10
    with pytest.raises(ValueError):
        I.distorted_boxes(4, (H, W), max_attempts=256, device=device)


# ------------------------------------------------------------------------------------------------------- hipGraph
@pytest.mark.parametrize("device", GPU_ONLY)
def test_hip_graph_replay_draws_anew(device):
    """``imagenet_preprocess(is_training=True)`` captured once on one stream and replayed three times, the device
    step counter advanced between replays: every replay is bitwise the eager call with the same host seed at that
    counter value, and the replays differ from each other."""
    _device(device)
    from mdtf.train.graph import rng_offset_tensor
    x = torch.from_numpy(IH.random_images(4, 40, 40, 3, seed=9)).cuda()
    counter = rng_offset_tensor(x.device)
    before = counter.clone()
    counter.zero_()
    seed = 1234

    def call():
        return I.imagenet_preprocess(x, is_training=True, output_height=24, output_width=24, dtype=BF, seed=seed)

    eager = []
    for _ in range(3):
        eager.append(call().clone())
        counter.add_(1)
    counter.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = call()
    replays = []
    try:
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            replays.append(out.clone())
            counter.add_(1)
    finally:
        counter.copy_(before)
    for e, r in zip(eager, replays):
        assert r.dtype == BF and tuple(r.shape) == (4, 24, 24, 3)
        assert torch.equal(e.view(torch.int16), r.view(torch.int16))
    assert not torch.equal(replays[0], replays[1]) or not torch.equal(replays[1], replays[2])
    del graph


# ------------------------------------------------------------------------------------------------------------ API
@pytest.mark.parametrize("device", DEVICES)
def test_tf_named_ops(device):
    device = _device(device)
    img = IH.random_images(3, 12, 10, 3, seed=31)
    x = torch.from_numpy(img).to(device)
    with _counter(device, 5):
        # random_crop / random_flip_left_right are their transform spelling with the drawn parameters
        boxes = I.random_boxes(3, (12, 10), (7, 6), seed=8, device=device)
        assert torch.equal(I.random_crop(x, (7, 6), seed=8), I.transform(x, (7, 6), boxes=boxes, dtype=U8))
        assert torch.equal(I.random_crop(x, (3, 7, 6, 3), seed=8), I.random_crop(x, (7, 6), seed=8))
        assert np.array_equal(I.random_crop(x, (7, 6), seed=8).cpu().numpy(),
                              IH.copy_values(img, IH.oracle_random_boxes(3, 12, 10, 7, 6, 8, 5), [0] * 3, 7, 6))
        flips = I.random_flips(3, seed=9, device=device)
        assert torch.equal(I.random_flip_left_right(x, seed=9), I.transform(x, (12, 10), flips=flips, dtype=U8))
    assert torch.equal(I.flip_left_right(x), I.transform(x, (12, 10), flips=[1, 1, 1], dtype=U8))
    assert np.array_equal(I.flip_left_right(x).cpu().numpy(), img[:, :, ::-1])
    assert np.array_equal(I.crop_to_bounding_box(x, 2, 3, 5, 4).cpu().numpy(), img[:, 2:7, 3:7])
    assert torch.equal(I.crop_to_bounding_box(x, 2, 3, 5, 4), I.transform(x, (5, 4), boxes=[2, 3, 5, 4], dtype=U8))
    padded = np.zeros((3, 16, 15, 3), np.uint8)
    padded[:, 1:13, 4:14] = img
    assert np.array_equal(I.pad_to_bounding_box(x, 1, 4, 16, 15).cpu().numpy(), padded)
    # central_crop(0.5): start int((12 - 6) / 2) = 3 and int((10 - 5) / 2) = 2, size 12 - 6 and 10 - 4
    assert np.array_equal(I.central_crop(x, 0.5).cpu().numpy(), img[:, 3:9, 2:8])
    # crop the height 12 -> 7 (offset 2) and pad the width 10 -> 15 (offset 2) at once, and the other way round
    both = np.zeros((3, 7, 15, 3), np.uint8)
    both[:, :, 2:12] = img[:, 2:9]
    assert np.array_equal(I.resize_image_with_crop_or_pad(x, 7, 15).cpu().numpy(), both)
    both = np.zeros((3, 17, 5, 3), np.uint8)
    both[:, 2:14] = img[:, :, 2:7]
    assert np.array_equal(I.resize_image_with_crop_or_pad(x, 17, 5).cpu().numpy(), both)
    # convert_image_dtype: v * float32(1 / 255), and the identity
    want = img.astype(np.float32) * np.float32(1.0 / 255.0)
    assert np.array_equal(IH.bits(I.convert_image_dtype(x, FP)), want.view(np.int32))
    assert np.array_equal(IH.bits(I.convert_image_dtype(x, BF)), IH.bf16_bits(want))
    assert I.convert_image_dtype(x, torch.float64).dtype == torch.float64 and I.convert_image_dtype(x, U8) is x
    # resize_bilinear and per_image_standardization are fp32 whatever the compute dtype
    assert I.resize_bilinear(x, (5, 5)).dtype == FP and I.per_image_standardization(x).dtype == FP
    # a 3-D image is a batch of one
    one = x[1]
    assert torch.equal(I.flip_left_right(one), I.flip_left_right(x)[1]) and I.flip_left_right(one).dim() == 3
    assert torch.equal(I.transform(one, (5, 4), boxes=[2, 3, 5, 4], mean=1.0, dtype=FP),
                       I.transform(x, (5, 4), boxes=[[2, 3, 5, 4]] * 3, mean=1.0, dtype=FP)[1])
    assert tuple(I.imagenet_preprocess(one, False, 8, 8).shape) == (8, 8, 3)
    # float images take the PyTorch path and keep their dtype through the crops
    assert torch.equal(I.crop_to_bounding_box(x.float(), 2, 3, 5, 4), x.float()[:, 2:7, 3:7])


@pytest.mark.parametrize("device", DEVICES)
def test_argument_errors(device):
    device = _device(device)
    x = torch.zeros(2, 12, 10, 3, dtype=U8, device=device)
    with pytest.raises(ValueError, match="inside"):
        I.transform(x, (5, 4), boxes=[8, 3, 5, 4])                                  # rows 8 .. 12 of 12
    with pytest.raises(ValueError, match="inside"):
        I.crop_to_bounding_box(x, 0, 7, 5, 4)
    with pytest.raises(NotImplementedError):
        I.transform(x, (6, 5), standardize=True)
    with pytest.raises(NotImplementedError):
        I.transform(x, (6, 5), boxes=[0, 0, 12, 10], standardize=True)
    with pytest.raises(ValueError):
        I.transform(x, (12, 10), mean=1.0, dtype=U8)
    with pytest.raises(ValueError):
        I.transform(x, (6, 5), dtype=U8)
    with pytest.raises(ValueError):
        I.transform(x, (6, 5), align_corners=True, half_pixel_centers=True)
    with pytest.raises(ValueError, match="channels"):
        I.transform(torch.zeros(2, 12, 10, 5, dtype=U8, device=device), (12, 10))
    with pytest.raises(ValueError, match="channels"):
        I.per_image_standardization(torch.zeros(2, 12, 10, 5, dtype=U8, device=device))
    with pytest.raises(ValueError):
        I.transform(x, (12, 10), mean=(1.0, 2.0))
    with pytest.raises(ValueError):
        I.random_crop(x, (13, 4))
    with pytest.raises(ValueError):
        I.pad_to_bounding_box(x, 1, 1, 12, 10)
    with pytest.raises(NotImplementedError):
        I.convert_image_dtype(x.float(), U8)


@pytest.mark.parametrize("device", DEVICES)
def test_recipes_follow_training_mode(device):
    device = _device(device)
    from mdtf.train import step as S
    img = IH.random_images(4, 40, 40, 3, seed=41)
    x = torch.from_numpy(img).to(device)
    with _counter(device, 0):
        _recipes(device, img, x)


def _recipes(device, img, x):
    from mdtf.train import step as S
    with S.training_mode(False):
        ev = I.imagenet_preprocess(x, output_height=24, output_width=24, dtype=FP)
        cev = I.cifar_preprocess(x, dtype=FP)
    with S.training_mode(True):
        tr = I.imagenet_preprocess(x, output_height=24, output_width=24, dtype=FP, seed=3)
        ctr = I.cifar_preprocess(x, dtype=FP, seed=3)
    assert torch.equal(ev, I.imagenet_preprocess(x, False, 24, 24, dtype=FP))
    assert torch.equal(tr, I.imagenet_preprocess(x, True, 24, 24, dtype=FP, seed=3)) and not torch.equal(tr, ev)
    # evaluation: the central 0.875 box (start int(40 * 0.125 / 2) = 2, size 36) resized, means subtracted
    box = np.tile([2, 2, 36, 36], (4, 1))
    want = IH.oracle_resize(img, box, [0] * 4, 24, 24, "legacy") - np.float32([123.68, 116.78, 103.94]).astype(float)
    assert (np.abs(ev.cpu().numpy() - want) <= IH.resize_tolerance(want, box, 1.0, False)).all()
    # training: the transform of the drawn boxes and flips
    boxes = I.distorted_boxes(4, (40, 40), seed=3, device=device)
    flips = I.random_flips(4, seed=3, device=device)
    assert torch.equal(tr, I.transform(x, (24, 24), boxes=boxes, flips=flips, mean=(123.68, 116.78, 103.94),
                                       dtype=FP))
    # CIFAR: evaluation standardizes, training standardizes a shifted, flipped crop of the padded image
    assert torch.equal(cev, I.per_image_standardization(x))
    cb = IH.oracle_random_boxes(4, 40, 40, 40, 40, 3, 0, pad=4)
    v = IH.copy_values(img, cb, IH.oracle_flips(4, 3, 0), 40, 40)
    for b, (mean, adj) in enumerate(IH.oracle_stats(v)):
        want = IH.f32_scale(v[b], np.float32(mean), np.float32(1.0 / adj))
        assert np.array_equal(IH.bits(ctr[b]), want.view(np.int32))
    assert torch.equal(ctr, I.cifar_preprocess(x, True, dtype=FP, seed=3)) and not torch.equal(ctr, cev)
    # dtype=None is the store's compute dtype, fp32 when there is none
    store = IH.fresh("cpu")
    assert I.imagenet_preprocess(x, False, 24, 24).dtype == FP
    store.compute_dtype = BF
    try:
        assert I.imagenet_preprocess(x, False, 24, 24).dtype == BF
    finally:
        store.compute_dtype = None


def test_synthetic_image_loader():
    from mdtf.data.loaders import SyntheticImageLoader
    IH.fresh("cpu")
    loader = SyntheticImageLoader(stored_shape=(9, 8, 3), num_classes=7, seed=2)
    loader.batch_size = 5
    x, y = loader._next()
    assert x.dtype == U8 and tuple(x.shape) == (5, 9, 8, 3) and y.dtype == torch.int64 and tuple(y.shape) == (5,)
    assert int(x.max()) > 200 and int(x.min()) < 50 and 0 <= int(y.min()) and int(y.max()) < 7
    assert loader._next()[0] is x and len(loader.load_train_batch()) == 2
    default = SyntheticImageLoader()
    assert default.shape == (256, 256, 3) and default.num_classes == 1000


# ----------------------------------------------------------------------------------------------------- end to end
def test_lenet_step_preprocesses_uint8_on_the_cpu():
    """Three training steps of LeNet over a uint8 [8, 28, 28, 1] source with ``cifar_preprocess`` as the tower's
    ``pre_process_fn``: the model sees standardized fp32 images, the loss is finite."""
    op, loss, checksum, seen = IH.lenet_step("cpu", hip_graph=False)
    sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
    del seen[:]
    sums = []
    for _ in range(3):
        _, lv, cs = sess.run([op, loss, checksum])
        assert np.isfinite(float(lv))
        sums.append(torch.as_tensor(cs).clone())
    assert len(seen) == 3
    for dtype, shape, mean in seen:
        assert dtype == FP and shape == (8, 28, 28, 1) and float(mean) < 1e-5
    assert any(not torch.equal(sums[0], s) for s in sums[1:])                # a new host seed every eager step
    IH.fresh("cpu")


@pytest.mark.gpu
def test_lenet_step_under_hip_graph_augments_every_step():
    """The same step with ``hip_graph=True``: two eager steps, the capture and two replays.  The checksum of the
    preprocessed input is a program output (no host read inside the step); the replays carry the captured host seed,
    so only the device step counter can make them differ."""
    _device("cuda")
    from mdtf.train import step as S
    from mdtf.train.graph import rng_offset_tensor
    counter = rng_offset_tensor(torch.device("cuda", 0))       # the captured step advances it: put it back afterwards
    before = counter.clone()
    try:
        op, loss, checksum, seen = IH.lenet_step("cuda", hip_graph=True)
        sess = mdtf.train.MonitoredTrainingSession(log_step_count_steps=0)
        sums = []
        for _ in range(5):
            _, lv, cs = sess.run([op, loss, checksum])
            sums.append(torch.as_tensor(cs).detach().clone())
            assert bool(torch.isfinite(torch.as_tensor(lv)).all())
        torch.cuda.synchronize()
        g = op.graph
        assert g is not None and g.graph is not None and g.replays == 3 and g.fallbacks == 0 and not g.disabled, vars(g)
        sums = [s.cpu() for s in sums]
        assert all(tuple(s.shape) == (8,) and bool(torch.isfinite(s).all()) for s in sums)
        assert all(dtype == BF and shape == (8, 28, 28, 1) for dtype, shape, _ in seen)
        assert not torch.equal(sums[2], sums[3]) and not torch.equal(sums[3], sums[4])
        assert len(set(tuple(s.tolist()) for s in sums)) >= 2
        assert int(counter) == int(before) + 3
    finally:
        S.release_graphs()
        counter.copy_(before)
        IH.fresh("cpu")
