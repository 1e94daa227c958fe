"""``tf.image`` on a uint8 NHWC batch (``csrc/image.hip``): device-drawn crop boxes and flips, exact box statistics,
and one fused pass crop / flip / bilinear resize / normalize.

Random draws.  ``r(i, k) = mix((i * 1024 + k) * 0x9E3779B1 ^ s)`` in 32-bit arithmetic for image ``i`` and counter
``k``; ``mix`` is the finalizer of the dropout hash (``x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
x ^= x >> 16``) and ``s = seed ^ (uint32(step_counter) * 0x85EBCA6B)`` with the device step counter
``mdtf.train.graph.rng_offset_tensor``, so a replayed hipGraph draws anew every step.  The counter layout::

    k = 0             crop row offset        y0 = mulhi_u32(r, H - th + 1) - pad
    k = 1             crop column offset     x0 = mulhi_u32(r, W - tw + 1) - pad
    k = 2             flip                   r >> 31
    k = 4 + 4a + 0    attempt a: area fraction   area_lo + u * (area_hi - area_lo),  u = (r >> 8) * 2^-24
    k = 4 + 4a + 1    attempt a: aspect ratio    ar_lo + u * (ar_hi - ar_lo)
    k = 4 + 4a + 2    attempt a: row offset      mulhi_u32(r, H - bh + 1)
    k = 4 + 4a + 3    attempt a: column offset   mulhi_u32(r, W - bw + 1)

``mulhi_u32(r, n) = (r * n) >> 32`` is uniform over ``[0, n)`` in integers.  Attempt ``a`` (at most 255 of them) of
the distorted box takes ``bw = round(sqrt(area * H * W * ar))`` and ``bh = round(sqrt(area * H * W / ar))`` in fp32
and is accepted when ``1 <= bh <= H`` and ``1 <= bw <= W``; after the last attempt the box is the whole image.

The pass, for output element ``(b, y, x, c)`` with ``xs = OW - 1 - x`` where image ``b`` is flipped, else ``x``::

    copy path (bh == OH and bw == OW):  v = src[b, y0 + y, x0 + xs, c], 0 outside the image
    resize path:  in = (y + o) * sy - o;  lo = max(floor(in), 0), hi = min(ceil(in), bh - 1), t = in - floor(in)
                  (o = 0.5 with half_pixel_centers else 0; sy = bh / OH, or (bh - 1) / (OH - 1) with align_corners);
                  the same in x;  top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx, v = top + (bot - top) * ty;
                  every source index is clamped into the image
    out = (v - mean) * inv     per channel, per image (statistics of the box: copy path only) or the identity

all in fp32, then rounded once to the output dtype.  uint8 output and per-image statistics always take the copy path:
the box size is then the output size.  On the GPU these are at most three launches with no host read.  CPU tensors,
``MDTF_KERNELS=torch`` and non-uint8 images run the PyTorch expression of the same definitions in the same fp32
order, with the draws computed in int64.
"""
import ctypes

import torch

from . import _native as N

N.register("mdtf_image_params", [N.P, N.P, N.I, N.I, N.I, N.I, N.I, N.I, N.I, N.F, N.F, N.F, N.F, N.I, N.U, N.P, N.P])
N.register("mdtf_image_stats", [N.P, N.I, N.I, N.I, N.I, N.P, N.I, N.I, N.I, N.I, N.P, N.P])
N.register("mdtf_image_transform", [N.P, N.I, N.I, N.I, N.I, N.P, N.I, N.I, N.I, N.I, N.P, N.P, N.I, N.I, N.I, N.I,
                                    N.I, N.P, N.P, N.P])

BOX_CROP, BOX_DISTORTED = 1, 2
MAP_LEGACY, MAP_HALF_PIXEL, MAP_ALIGN_CORNERS = 0, 1, 2
SCALE_NONE, SCALE_CHANNEL, SCALE_IMAGE = 0, 1, 2
OUT_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.uint8: 2}
MAX_ATTEMPTS = 255
K_CROP_Y, K_CROP_X, K_FLIP, K_ATTEMPT = 0, 1, 2, 4

_M = 0xFFFFFFFF


def host_seed(seed):
    """A 32-bit host seed: the caller's, or one drawn from torch's generator (as the dropout call sites do)."""
    if seed is None:
        return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    return int(seed) & _M


def _counter(device):
    from ..train.graph import rng_offset_tensor
    return rng_offset_tensor(device)


# ----------------------------------------------------------------------------------------------------- reference
def _mix(x):
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & _M
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & _M
    return x ^ (x >> 16)


def _draw(i, k, s):
    """r(i, k) for int64 image indices ``i``, a counter ``k`` (int or int64 tensor) and the 0-d step seed ``s``."""
    return _mix(((((i * 1024 + k) & _M) * 0x9E3779B1) & _M) ^ s)


def _step_seed(seed, counter):
    return (((counter.reshape(()) & _M) * 0x85EBCA6B) & _M) ^ seed


def _below(r, n):
    return (r * n) >> 32


def _unit(r):
    return (r >> 8).to(torch.float32) * (2.0 ** -24)


def _params_reference(batch, device, mode, H, W, th, tw, pad, area, aspect, attempts, want_flips, seed, counter):
    i = torch.arange(batch, dtype=torch.int64, device=device)
    s = _step_seed(seed, counter.to(device))
    flips = (_draw(i, K_FLIP, s) >> 31).to(torch.int32) if want_flips else None
    if mode is None:
        return None, flips
    if mode == BOX_CROP:
        y0 = _below(_draw(i, K_CROP_Y, s), H - th + 1) - pad
        x0 = _below(_draw(i, K_CROP_X, s), W - tw + 1) - pad
        boxes = torch.stack([y0, x0, torch.full_like(y0, th), torch.full_like(y0, tw)], 1)
        return boxes.to(torch.int32), flips
    f32 = torch.float32
    # (constants by fill, not by upload: this path may be captured too)
    hw = torch.full((), float(H), dtype=f32, device=device) * torch.full((), float(W), dtype=f32, device=device)
    a_lo, a_hi, r_lo, r_hi = (torch.full((), v, dtype=f32, device=device) for v in area + aspect)
    zero = torch.zeros(batch, dtype=torch.int64, device=device)
    boxes = torch.stack([zero, zero, zero + H, zero + W], 1)
    done = torch.zeros(batch, dtype=torch.bool, device=device)
    for a in range(attempts):
        k = K_ATTEMPT + 4 * a
        ar_a = a_lo + _unit(_draw(i, k, s)) * (a_hi - a_lo)
        ar_r = r_lo + _unit(_draw(i, k + 1, s)) * (r_hi - r_lo)
        fw, fh = torch.round(torch.sqrt(ar_a * hw * ar_r)), torch.round(torch.sqrt(ar_a * hw / ar_r))
        ok = (fh >= 1) & (fh <= H) & (fw >= 1) & (fw <= W) & ~done
        bh, bw = fh.to(torch.int64).clamp(1, H), fw.to(torch.int64).clamp(1, W)
        y0, x0 = _below(_draw(i, k + 2, s), H - bh + 1), _below(_draw(i, k + 3, s), W - bw + 1)
        boxes = torch.where(ok[:, None], torch.stack([y0, x0, bh, bw], 1), boxes)
        done = done | ok
        if device.type == "cpu" and bool(done.all()):
            break
    return boxes.to(torch.int32), flips


def _box_columns(boxes, batch, H, W, device):
    if boxes is None or isinstance(boxes, tuple):            # one box for every image (default: the whole image)
        y0, x0, bh, bw = boxes or (0, 0, H, W)
        z = torch.zeros(batch, dtype=torch.int64, device=device)
        return z + y0, z + x0, z + bh, z + bw
    b = boxes.to(torch.int64)
    return b[:, 0], b[:, 1], b[:, 2], b[:, 3]


def _copy_reference(images, boxes, flips, OH, OW):
    """[B, OH, OW, C] of the OH x OW box at (y0, x0), zeros outside the image, in the images' dtype."""
    B, H, W, _ = images.shape
    dev = images.device
    y0, x0, _, _ = _box_columns(boxes, B, H, W, dev)
    ys, xs = torch.arange(OH, device=dev), torch.arange(OW, device=dev)
    xs = xs[None, :].expand(B, OW)
    if flips is not None:
        xs = torch.where(flips.to(torch.bool)[:, None], OW - 1 - xs, xs)
    yy, xx = y0[:, None] + ys[None, :], x0[:, None] + xs
    inside = ((yy >= 0) & (yy < H))[:, :, None] & ((xx >= 0) & (xx < W))[:, None, :]
    bi = torch.arange(B, device=dev)[:, None, None]
    v = images[bi, yy.clamp(0, H - 1)[:, :, None], xx.clamp(0, W - 1)[:, None, :]]
    return torch.where(inside[..., None], v, torch.zeros((), dtype=v.dtype, device=dev))


def _axis_reference(n_out, flipped, box0, boxn, limit, mapping, dev):
    """Source indices (clamped into the image) and weights of one axis: ([B, n_out] lo, hi, t)."""
    f32 = torch.float32
    o = torch.arange(n_out, device=dev)[None, :].expand(box0.shape[0], n_out)
    if flipped is not None:
        o = torch.where(flipped.to(torch.bool)[:, None], n_out - 1 - o, o)
    if mapping == MAP_ALIGN_CORNERS:
        scale = (boxn - 1).to(f32) / float(n_out - 1) if n_out > 1 else torch.zeros_like(boxn, dtype=f32)
    else:
        scale = boxn.to(f32) / float(n_out)
    half = 0.5 if mapping == MAP_HALF_PIXEL else 0.0
    pos = (o.to(f32) + half) * scale[:, None] - half
    fl = torch.floor(pos)
    lo = fl.to(torch.int64).clamp(min=0)
    hi = torch.minimum(torch.ceil(pos).to(torch.int64), (boxn - 1)[:, None])
    return ((box0[:, None] + lo).clamp(0, limit - 1), (box0[:, None] + hi).clamp(0, limit - 1), pos - fl)


def _resize_reference(images, boxes, flips, OH, OW, mapping):
    B, H, W, _ = images.shape
    dev = images.device
    y0, x0, bh, bw = _box_columns(boxes, B, H, W, dev)
    yl, yh, ty = _axis_reference(OH, None, y0, bh, H, mapping, dev)
    xl, xh, tx = _axis_reference(OW, flips, x0, bw, W, mapping, dev)
    bi = torch.arange(B, device=dev)[:, None, None]
    f = torch.float32
    tl, tr = images[bi, yl[:, :, None], xl[:, None, :]].to(f), images[bi, yl[:, :, None], xh[:, None, :]].to(f)
    bl, br = images[bi, yh[:, :, None], xl[:, None, :]].to(f), images[bi, yh[:, :, None], xh[:, None, :]].to(f)
    tx, ty = tx[:, None, :, None], ty[:, :, None, None]
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    return top + (bot - top) * ty


def _stats_reference(images, boxes, OH, OW):
    v = _copy_reference(images, boxes, None, OH, OW)
    n = float(OH * OW * images.shape[3])
    if images.dtype == torch.uint8:
        v = v.to(torch.int64)
        S, Q = v.sum((1, 2, 3)).double(), (v * v).sum((1, 2, 3)).double()
    else:
        v = v.double()
        S, Q = v.sum((1, 2, 3)), (v * v).sum((1, 2, 3))
    mean = S / n
    adj = torch.sqrt((Q / n - mean * mean).clamp(min=0.0)).clamp(min=1.0 / n ** 0.5)
    return torch.stack([mean, 1.0 / adj], 1).to(torch.float32)


def _transform_reference(images, boxes, flips, OH, OW, mapping, scale_mode, mean_inv, stats, out_dtype, copy):
    B, H, W, C = images.shape
    dev = images.device
    if copy is None:                                         # device boxes: which path is known per image only there
        _, _, bh, bw = _box_columns(boxes, B, H, W, dev)
        same = ((bh == OH) & (bw == OW))[:, None, None, None]
        v = torch.where(same, _copy_reference(images, boxes, flips, OH, OW).to(torch.float32),
                        _resize_reference(images, boxes, flips, OH, OW, mapping))
    elif copy:
        v = _copy_reference(images, boxes, flips, OH, OW)
        if out_dtype == torch.uint8:
            return v
        v = v.to(torch.float32)
    else:
        v = _resize_reference(images, boxes, flips, OH, OW, mapping)
    if scale_mode == SCALE_CHANNEL:
        mi = torch.stack([torch.full((), v, dtype=torch.float32, device=dev) for v in mean_inv])
        v = (v - mi[:C]) * mi[4:4 + C]
    elif scale_mode == SCALE_IMAGE:
        v = (v - stats[:, 0, None, None, None]) * stats[:, 1, None, None, None]
    return v.to(out_dtype)


# ---------------------------------------------------------------------------------------------------------- ops
def params(batch, device, mode=None, image_size=None, crop_size=None, pad=0, area=(0.08, 1.0),
           aspect=(0.75, 1.3333), max_attempts=100, flips=False, seed=None):
    """``(boxes, flips)``: int32 [batch, 4] ``{y0, x0, bh, bw}`` (None without a ``mode``) and int32 [batch] (None
    unless ``flips``), drawn in one launch from ``seed`` and the device step counter."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:       # the counter is kept per indexed device, as x.device is
        device = torch.device("cuda", torch.cuda.current_device())
    batch = int(batch)
    if mode is None and not flips:
        raise ValueError("nothing to draw")
    H = W = th = tw = 1
    if mode is not None:
        H, W = (int(v) for v in image_size)
        if H < 1 or W < 1:
            raise ValueError("image size must be positive, got %s" % (image_size,))
    if mode == BOX_CROP:
        th, tw = (int(v) for v in crop_size)
        pad = int(pad)
        if pad < 0 or th < 1 or tw < 1 or th > H + 2 * pad or tw > W + 2 * pad:
            raise ValueError("crop %s does not fit the image %s padded by %d" % ((th, tw), (H, W), pad))
        H, W = H + 2 * pad, W + 2 * pad
    elif mode == BOX_DISTORTED:
        area, aspect = tuple(float(v) for v in area), tuple(float(v) for v in aspect)
        max_attempts = int(max_attempts)
        if not (0.0 < area[0] <= area[1] <= 1.0) or not (0.0 < aspect[0] <= aspect[1]):
            raise ValueError("area_range %s / aspect_ratio_range %s" % (area, aspect))
        if not 1 <= max_attempts <= MAX_ATTEMPTS:
            raise ValueError("max_attempts must lie in [1, %d], got %d" % (MAX_ATTEMPTS, max_attempts))
    elif mode is not None:
        raise ValueError("unknown box mode %r" % (mode,))
    seed = host_seed(seed)
    counter = _counter(device)
    if not (device.type == "cuda" and N.mode() != "torch" and batch > 0):
        return _params_reference(batch, device, mode, H, W, th, tw, pad, area, aspect, max_attempts, flips, seed,
                                 counter)
    N.lib()
    with torch.cuda.device(device):
        boxes = torch.empty(batch, 4, dtype=torch.int32, device=device) if mode is not None else None
        fl = torch.empty(batch, dtype=torch.int32, device=device) if flips else None
        N.check(N.fn("mdtf_image_params")(N.ptr(boxes), N.ptr(fl), batch, mode or 0, H, W, th, tw, pad, area[0],
                                          area[1], aspect[0], aspect[1], max_attempts, seed, N.ptr(counter),
                                          N.stream_ptr()), "image_params")
    return boxes, fl


def _device_ints(t, shape, images, what):
    if t is None:
        return None
    if isinstance(t, (tuple, list)):                         # boxes: one host box shared by every image
        if len(t) != 4:
            raise ValueError("a shared box is (y0, x0, height, width), got %r" % (t,))
        return tuple(int(v) for v in t)
    if tuple(t.shape) != shape:
        raise ValueError("%s must have shape %s, got %s" % (what, shape, tuple(t.shape)))
    return t.detach().to(device=images.device, dtype=torch.int32).contiguous()


def _box_ptr(boxes):
    return N.ptr(None if isinstance(boxes, tuple) else boxes)


def stats(images, boxes, OH, OW):
    """fp32 [B, 2] ``{mean, 1 / adjusted stddev}`` of the OH x OW box of every image (the copy path's values)."""
    images = images.detach()
    B, H, W, C = images.shape
    boxes = _device_ints(boxes, (B, 4), images, "boxes")
    if not (images.dtype == torch.uint8 and N.use_native(images) and B > 0):
        return _stats_reference(images, boxes, OH, OW)
    images = images.contiguous()
    out = torch.empty(B, 2, dtype=torch.float32, device=images.device)
    shared = boxes if isinstance(boxes, tuple) else (0, 0, OH, OW)
    N.check(N.fn("mdtf_image_stats")(N.ptr(images), B, H, W, C, _box_ptr(boxes), shared[0], shared[1], OH, OW,
                                     N.ptr(out), N.stream_ptr()), "image_stats")
    return out


def transform(images, OH, OW, boxes=None, flips=None, mapping=MAP_LEGACY, scale_mode=SCALE_NONE, mean_inv=None,
              stats=None, out_dtype=torch.float32, copy=None):
    """The fused pass over ``images`` [B, H, W, C] -> [B, OH, OW, C] of ``out_dtype``.  ``boxes`` is an int32 [B, 4]
    device tensor, one host ``(y0, x0, bh, bw)`` shared by every image (passed by value: nothing is uploaded) or None
    (the whole image); ``flips`` an int32 [B] device tensor or None; ``mean_inv`` 8 host floats ``{mean[4], inv[4]}`` already rounded
    to fp32; ``copy``: whether every image is known to take the copy path (None: decided per image from its box; the
    kernel decides per image in any case)."""
    images = images.detach()
    if images.dim() != 4:
        raise ValueError("images must be [B, H, W, C], got %s" % (tuple(images.shape),))
    B, H, W, C = images.shape
    if not 1 <= C <= 4:
        raise ValueError("images must have 1 to 4 channels, got %d" % C)
    if H < 1 or W < 1 or OH < 1 or OW < 1:
        raise ValueError("empty image or output size: %s -> %s" % ((H, W), (OH, OW)))
    if out_dtype not in OUT_DTYPES:
        raise ValueError("output dtype must be bfloat16, float32 or uint8, got %s" % out_dtype)
    if out_dtype == torch.uint8 and (scale_mode != SCALE_NONE or images.dtype != torch.uint8):
        raise ValueError("uint8 output takes uint8 images and the identity scale")
    if out_dtype == torch.uint8 or scale_mode == SCALE_IMAGE:
        copy = True
    boxes = _device_ints(boxes, (B, 4), images, "boxes")
    flips = _device_ints(flips, (B,), images, "flips")
    if not (images.dtype == torch.uint8 and N.use_native(images) and B > 0):
        return _transform_reference(images, boxes, flips, OH, OW, mapping, scale_mode, mean_inv, stats, out_dtype,
                                    copy)
    images = images.contiguous()
    out = torch.empty(B, OH, OW, C, dtype=out_dtype, device=images.device)
    mi = (ctypes.c_float * 8)(*mean_inv) if scale_mode == SCALE_CHANNEL else None
    shared = boxes if isinstance(boxes, tuple) else (0, 0, H, W)
    N.check(N.fn("mdtf_image_transform")(N.ptr(images), B, H, W, C, _box_ptr(boxes), *shared, N.ptr(flips), N.ptr(out),
                                         OUT_DTYPES[out_dtype], OH, OW, mapping, scale_mode, mi, N.ptr(stats),
                                         N.stream_ptr()), "image_transform")
    return out
