"""``tf.image`` for uint8 NHWC batches, preprocessed on the device (``mdtf.ops.image`` / ``csrc/image.hip``).

Images are ``[B, H, W, C]`` with 1 to 4 channels; a 3-D image is a batch of one and comes back 3-D.  Everything here
is one call of :func:`transform`, a single fused pass on the GPU: crop box, left-right flip, bilinear resize, mean /
stddev normalization, and the conversion to the dtype the model reads (bf16 NHWC for the stem).  Random boxes and
flips are drawn on the device from a host seed and the device step counter of the dropout kernels
(``mdtf.train.graph.rng_offset_tensor``), so the ops can sit in ``pre_process_fn`` / ``Net.pre_process`` inside a
captured step and still augment differently on every replay.  The definitions are in ``mdtf.ops.image``.

Deviations from TensorFlow:

* crops and flips are drawn per image of a batch (``tf.image.random_crop`` / ``random_flip_left_right`` on a 4-D tensor
  use one draw for the whole batch);
* :func:`distorted_boxes` is the attempt loop of ``sample_distorted_bounding_box`` over the whole image as documented
  in ``mdtf.ops.image``, not TF's sampler bit for bit;
* :func:`imagenet_preprocess` in evaluation crops the central box and resizes it (TF's recipes resize, then crop);
* float images run the PyTorch expression of the same definitions, not a kernel;
* with uint8 output or ``standardize=True`` the size of a device-side box is taken to be the output size.

No gradient flows through any of it: outputs are detached.
"""
import torch

from .ops import image as O
from .train import variables as V

__all__ = ["random_boxes", "distorted_boxes", "random_flips", "transform", "random_crop", "random_flip_left_right",
           "flip_left_right", "crop_to_bounding_box", "pad_to_bounding_box", "resize_image_with_crop_or_pad",
           "central_crop", "resize_bilinear", "per_image_standardization", "convert_image_dtype",
           "imagenet_preprocess", "cifar_preprocess"]


def _pair(size, what):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s must be (height, width), got %r" % (what, size))
    if h < 1 or w < 1:
        raise ValueError("%s must be positive, got %r" % (what, size))
    return h, w


def _device(device):
    device = torch.device(V.get_store().device if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _batched(images):
    if not isinstance(images, torch.Tensor) or images.dim() not in (3, 4):
        raise ValueError("images must be a [B, H, W, C] or [H, W, C] tensor")
    return (images.unsqueeze(0), True) if images.dim() == 3 else (images, False)


# ------------------------------------------------------------------------------------------------------ parameters
def random_boxes(batch, image_size, crop_size, seed=None, pad=0, device=None):
    """int32 [batch, 4] ``{y0, x0, th, tw}``: a ``crop_size`` box placed uniformly inside every image of
    ``image_size`` (zero-padded by ``pad`` on every side: offsets then start at ``-pad``)."""
    return O.params(batch, _device(device), O.BOX_CROP, _pair(image_size, "image_size"),
                    _pair(crop_size, "crop_size"), pad=pad, seed=seed)[0]


def distorted_boxes(batch, image_size, area_range=(0.08, 1.0), aspect_ratio_range=(0.75, 1.3333), max_attempts=100,
                    seed=None, device=None):
    """int32 [batch, 4] ``{y0, x0, bh, bw}``: the Inception / ResNet distorted crop over the whole image.  Up to
    ``max_attempts`` (at most 255) draws of an area fraction and an aspect ratio ``bw / bh``; the first box that fits
    the image is placed uniformly, and after the last attempt the box is the whole image."""
    return O.params(batch, _device(device), O.BOX_DISTORTED, _pair(image_size, "image_size"), area=area_range,
                    aspect=aspect_ratio_range, max_attempts=max_attempts, seed=seed)[0]


def random_flips(batch, seed=None, device=None):
    """int32 [batch] of 0 / 1, each with probability one half."""
    return O.params(batch, _device(device), flips=True, seed=seed)[1]


# ------------------------------------------------------------------------------------------------------- transform
def _host_boxes(boxes, batch, H, W):
    """A host list of one ``(y0, x0, bh, bw)`` or of ``batch`` of them -> ([batch, 4] ints, the common size or None)."""
    rows = list(boxes)
    if len(rows) == 4 and not isinstance(rows[0], (list, tuple)):
        rows = [rows] * batch
    if len(rows) != batch:
        raise ValueError("expected one box or %d boxes, got %d" % (batch, len(rows)))
    out = []
    for r in rows:
        if len(r) != 4:
            raise ValueError("a box is (y0, x0, height, width), got %r" % (r,))
        y0, x0, bh, bw = (int(v) for v in r)
        if bh < 1 or bw < 1 or y0 < 0 or x0 < 0 or y0 + bh > H or x0 + bw > W:
            raise ValueError("box %r does not lie inside the %d x %d image" % (tuple(r), H, W))
        out.append((y0, x0, bh, bw))
    sizes = set(r[2:] for r in out)
    return out, (sizes.pop() if len(sizes) == 1 else None)


def _scale(C, mean, std):
    if mean is None and std is None:
        return O.SCALE_NONE, None

    def per_channel(v, default, what):
        if v is None:
            return [default] * C
        vals = [float(x) for x in v] if isinstance(v, (list, tuple)) else [float(v)] * C
        if len(vals) != C:
            raise ValueError("%s must be a number or have one value per channel (%d), got %r" % (what, C, v))
        return vals
    m, s = per_channel(mean, 0.0, "mean"), per_channel(std, 1.0, "std")
    if any(x == 0.0 for x in s):
        raise ValueError("std must not be zero")
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float64).to(torch.float32))     # rounded once, from double
    pad = [0.0] * (4 - C)
    return O.SCALE_CHANNEL, [f32(x) for x in m] + pad + [f32(1.0 / x) for x in s] + [1.0] * (4 - C)


def _run(images, size, boxes=None, box_size=None, flips=None, mean=None, std=None, standardize=False, dtype=None,
         mapping=O.MAP_LEGACY):
    """``boxes``: a device tensor or an already checked host list; ``box_size``: the size every box is known to have
    (None: only the device knows)."""
    x, squeeze = _batched(images)
    B, H, W, C = x.shape
    OH, OW = size
    if dtype is None:
        dtype = V.get_store().compute_dtype or torch.float32
    if boxes is None:
        box_size = (H, W)
    elif not isinstance(boxes, torch.Tensor):
        boxes = [tuple(r) for r in boxes]
        if len(set(boxes)) == 1:
            boxes = boxes[0]                                 # by value: no upload, nothing for a capture to keep
        else:
            boxes = torch.tensor(boxes, dtype=torch.int32).reshape(B, 4).to(x.device)
    copy = None if box_size is None else tuple(box_size) == (OH, OW)
    scale_mode, mean_inv = _scale(C, mean, std)
    st = None
    if standardize:
        if scale_mode != O.SCALE_NONE:
            raise ValueError("standardize=True takes no mean / std")
        if copy is False:
            raise NotImplementedError("per-image standardization of a resized image")
        if not 1 <= C <= 4:
            raise ValueError("images must have 1 to 4 channels, got %d" % C)
        scale_mode, st = O.SCALE_IMAGE, O.stats(x, boxes, OH, OW)
    if dtype == torch.uint8 and copy is False:
        raise ValueError("uint8 output of a resized image")
    post = None
    if dtype not in O.OUT_DTYPES:
        if not dtype.is_floating_point:
            raise ValueError("output dtype must be a float type or uint8, got %s" % dtype)
        dtype, post = torch.float32, dtype
    out = O.transform(x, OH, OW, boxes, flips, mapping, scale_mode, mean_inv, st, dtype, copy)
    if post is not None:
        out = out.to(post)
    return out[0] if squeeze else out


def transform(images, size, boxes=None, flips=None, mean=None, std=None, standardize=False, dtype=None,
              align_corners=False, half_pixel_centers=False):
    """The fused pass: for every image the box ``boxes[b] = (y0, x0, bh, bw)`` (default: the whole image), flipped
    left to right where ``flips[b]``, resized bilinearly to ``size`` (copied when the box already has that size, and
    then zero outside the image), then ``(v - mean) / std`` per channel or, with ``standardize``,
    ``tf.image.per_image_standardization``, as ``dtype`` (default: the store's compute dtype, or fp32).

    ``boxes`` is an int32 ``[B, 4]`` device tensor (never read by the host: out-of-image parts are clamped, on the
    copy path zero) or a host list of one or ``B`` boxes, checked against the image.  ``flips`` is an int ``[B]``
    tensor.  uint8 output needs the identity scale and no resize."""
    if align_corners and half_pixel_centers:
        raise ValueError("align_corners and half_pixel_centers cannot both be set")
    mapping = O.MAP_ALIGN_CORNERS if align_corners else O.MAP_HALF_PIXEL if half_pixel_centers else O.MAP_LEGACY
    x, _ = _batched(images)
    box_size = None
    if boxes is not None and not isinstance(boxes, torch.Tensor):
        boxes, box_size = _host_boxes(boxes, x.shape[0], x.shape[1], x.shape[2])
        if box_size is None and (standardize or dtype == torch.uint8):
            raise NotImplementedError("boxes of several sizes with standardize=True or uint8 output")
    if flips is not None and not isinstance(flips, torch.Tensor):
        flips = torch.tensor([int(bool(f)) for f in flips], dtype=torch.int32)
    return _run(images, _pair(size, "size"), boxes, box_size, flips, mean, std, standardize, dtype, mapping)


def _same_dtype(images):
    return images.dtype if images.dtype == torch.uint8 or images.dtype.is_floating_point else torch.float32


# ------------------------------------------------------------------------------------------------------- TF names
def random_crop(images, size, seed=None, name=None):
    """A ``size`` = (height, width[, channels]) box at a random offset, drawn per image; the dtype is kept."""
    x, _ = _batched(images)
    size = tuple(int(v) for v in size)
    B, H, W, C = x.shape
    if len(size) == images.dim():                            # TF's form: the shape of the result
        if size[-1] != C or (len(size) == 4 and size[0] != B):
            raise ValueError("random_crop keeps batch and channels of %s, got size %r" % (tuple(images.shape), size))
        size = size[-3:-1]
    th, tw = _pair(size, "size")
    if th > H or tw > W:
        raise ValueError("crop %s larger than the image %s" % ((th, tw), (H, W)))
    boxes = random_boxes(B, (H, W), (th, tw), seed=seed, device=x.device)
    return _run(images, (th, tw), boxes, (th, tw), dtype=_same_dtype(x))


def flip_left_right(images):
    x, _ = _batched(images)
    flips = torch.ones(x.shape[0], dtype=torch.int32, device=x.device)
    return _run(images, tuple(x.shape[1:3]), flips=flips, dtype=_same_dtype(x))


def random_flip_left_right(images, seed=None):
    """Every image flipped with probability one half, drawn per image; the dtype is kept."""
    x, _ = _batched(images)
    return _run(images, tuple(x.shape[1:3]), flips=random_flips(x.shape[0], seed=seed, device=x.device),
                dtype=_same_dtype(x))


def crop_to_bounding_box(images, offset_height, offset_width, target_height, target_width):
    x, _ = _batched(images)
    box = (int(offset_height), int(offset_width), int(target_height), int(target_width))
    boxes, size = _host_boxes(box, x.shape[0], x.shape[1], x.shape[2])
    return _run(images, size, boxes, size, dtype=_same_dtype(x))


def pad_to_bounding_box(images, offset_height, offset_width, target_height, target_width):
    """The image at ``(offset_height, offset_width)`` of a ``target_height`` x ``target_width`` canvas of zeros."""
    x, _ = _batched(images)
    B, H, W, _ = x.shape
    oh, ow, th, tw = int(offset_height), int(offset_width), int(target_height), int(target_width)
    if oh < 0 or ow < 0 or th < oh + H or tw < ow + W:
        raise ValueError("the %d x %d image at (%d, %d) does not fit a %d x %d canvas" % (H, W, oh, ow, th, tw))
    return _run(images, (th, tw), [(-oh, -ow, th, tw)] * B, (th, tw), dtype=_same_dtype(x))


def resize_image_with_crop_or_pad(images, target_height, target_width):
    """Central crop and / or symmetric zero padding to the target size, each axis on its own (TF's offsets)."""
    x, _ = _batched(images)
    B, H, W, _ = x.shape
    th, tw = _pair((target_height, target_width), "target size")

    def offset(n, t):
        diff = t - n
        return max(-diff // 2, 0) - max(diff // 2, 0)
    return _run(images, (th, tw), [(offset(H, th), offset(W, tw), th, tw)] * B, (th, tw), dtype=_same_dtype(x))


def _central_box(H, W, fraction):
    fraction = float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError("central_fraction must lie in (0, 1], got %r" % fraction)
    y0, x0 = int((H - H * fraction) / 2), int((W - W * fraction) / 2)
    return y0, x0, H - 2 * y0, W - 2 * x0


def central_crop(images, central_fraction):
    x, _ = _batched(images)
    B, H, W, _ = x.shape
    box = _central_box(H, W, central_fraction)
    return _run(images, box[2:], [box] * B, box[2:], dtype=_same_dtype(x))


def resize_bilinear(images, size, align_corners=False, half_pixel_centers=False):
    """``tf.image.resize_bilinear``: fp32 out."""
    return transform(images, size, dtype=torch.float32, align_corners=align_corners,
                     half_pixel_centers=half_pixel_centers)


def per_image_standardization(images):
    """``(x - mean) / max(stddev, 1 / sqrt(N))`` over each image; fp32 out.  The sums of a uint8 image are exact."""
    x, _ = _batched(images)
    return _run(images, tuple(x.shape[1:3]), standardize=True, dtype=torch.float32)


def convert_image_dtype(images, dtype):
    """uint8 -> a float type, scaled by 1 / 255 (uint8 -> uint8 is the identity)."""
    if images.dtype != torch.uint8:
        raise NotImplementedError("convert_image_dtype from %s" % images.dtype)
    if dtype == torch.uint8:
        return images
    if not dtype.is_floating_point:
        raise NotImplementedError("convert_image_dtype to %s" % dtype)
    x, _ = _batched(images)
    return _run(images, tuple(x.shape[1:3]), std=255.0, dtype=dtype)


# -------------------------------------------------------------------------------------------------------- recipes
def _is_training(flag):
    if flag is None:
        from .train import step as S
        return S.is_training()
    return bool(flag)


def imagenet_preprocess(images, is_training=None, output_height=224, output_width=224, central_fraction=0.875,
                        mean=(123.68, 116.78, 103.94), std=None, dtype=None, seed=None):
    """The ImageNet input recipe in two launches (training) or one (evaluation).

    Training: a distorted box (area 8 % to 100 %, aspect ratio 3/4 to 4/3) and a flip per image, the box resized
    bilinearly to the output size, the channel means subtracted.  Evaluation: the central ``central_fraction`` box
    resized to the output size (TF resizes first and crops after), the means subtracted.  ``is_training=None`` reads
    ``mdtf.train.step.is_training()``."""
    x, _ = _batched(images)
    B, H, W, C = x.shape
    size = _pair((output_height, output_width), "output size")
    if mean is not None and isinstance(mean, (list, tuple)) and len(mean) != C:
        raise ValueError("mean has %d values for %d channels" % (len(mean), C))
    if _is_training(is_training):
        boxes, flips = O.params(B, x.device, O.BOX_DISTORTED, (H, W), flips=True, seed=seed)
        return _run(images, size, boxes, None, flips, mean, std, dtype=dtype)
    box = _central_box(H, W, central_fraction)
    return _run(images, size, [box] * B, box[2:], None, mean, std, dtype=dtype)


def cifar_preprocess(images, is_training=None, pad=4, dtype=None, seed=None):
    """The CIFAR input recipe: in training a random crop of the image's own size out of the image zero-padded by
    ``pad`` and a flip, per image, then per-image standardization of the crop (three launches); in evaluation the
    standardization alone (two)."""
    x, _ = _batched(images)
    B, H, W, _ = x.shape
    if not _is_training(is_training):
        return _run(images, (H, W), standardize=True, dtype=dtype)
    boxes, flips = O.params(B, x.device, O.BOX_CROP, (H, W), (H, W), pad=pad, flips=True, seed=seed)
    return _run(images, (H, W), boxes, (H, W), flips, standardize=True, dtype=dtype)
