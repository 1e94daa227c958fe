"""Oracles and case builders of ``tests/test_image.py``, written in numpy from the definitions in the module docstring
of ``mdtf.ops.image`` (the counter layout is mirrored from there); nothing here calls ``mdtf.ops.image``."""
import numpy as np
import torch

U = 2.0 ** -24                                   # fp32 unit roundoff
K_CROP_Y, K_CROP_X, K_FLIP, K_ATTEMPT = 0, 1, 2, 4
_M = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------- hash
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix(x):
    x = _u64(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M
    return x ^ (x >> np.uint64(16))


def step_seed(seed, counter):
    return np.uint64(seed) ^ ((np.uint64(counter & 0xFFFFFFFF) * np.uint64(0x85EBCA6B)) & _M)


def draw(batch, k, seed, counter):
    i = np.arange(batch, dtype=np.uint64)
    idx = (i * np.uint64(1024) + np.uint64(k)) & _M
    return mix(((idx * np.uint64(0x9E3779B1)) & _M) ^ step_seed(seed, counter))


def mulhi(r, n):
    return ((r * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def oracle_random_boxes(batch, H, W, th, tw, seed, counter, pad=0):
    y0 = mulhi(draw(batch, K_CROP_Y, seed, counter), H + 2 * pad - th + 1) - pad
    x0 = mulhi(draw(batch, K_CROP_X, seed, counter), W + 2 * pad - tw + 1) - pad
    return np.stack([y0, x0, np.full(batch, th), np.full(batch, tw)], 1)


def oracle_flips(batch, seed, counter):
    return (draw(batch, K_FLIP, seed, counter) >> np.uint64(31)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- copy
def copy_values(img, boxes, flips, OH, OW):
    """uint8 [B, OH, OW, C]: src[b, y0 + y, x0 + xs, c], 0 outside the image."""
    B, H, W, C = img.shape
    out = np.zeros((B, OH, OW, C), dtype=np.uint8)
    for b in range(B):
        y0, x0 = int(boxes[b][0]), int(boxes[b][1])
        for y in range(OH):
            yy = y0 + y
            if not 0 <= yy < H:
                continue
            for x in range(OW):
                xx = x0 + (OW - 1 - x if flips[b] else x)
                if 0 <= xx < W:
                    out[b, y, x] = img[b, yy, xx]
    return out


def f32_scale(v, mean, inv):
    """The fp32 mirror ``(float32(v) - mean) * inv``: a subtraction, then a multiplication, each rounded to fp32."""
    return (v.astype(np.float32) - np.asarray(mean, dtype=np.float32)) * np.asarray(inv, dtype=np.float32)


def channel_scale(mean, std):
    """fp32 ``mean[c]`` and ``1 / std[c]``, formed in double and rounded once."""
    return (np.asarray(mean, dtype=np.float64).astype(np.float32),
            (1.0 / np.asarray(std, dtype=np.float64)).astype(np.float32))


def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (int16) of an fp32 array without NaNs."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return b.astype(np.uint16).view(np.int16)


def bits(t):
    """The bit patterns of a torch fp32 / bf16 tensor as a numpy integer array."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def corner_and_pad_boxes(B, H, W, OH, OW):
    """B lists of boxes of the output size: the four corners, an odd x0, the middle, and pad boxes that hang over each
    edge by 1 to 4 pixels; every image cycles through them from a different start."""
    inside = [(0, 0), (0, W - OW), (H - OH, 0), (H - OH, W - OW), ((H - OH) // 2, ((W - OW) // 2) | 1 if W > OW else 0)]
    inside = [(min(max(y, 0), H - OH), min(max(x, 0), W - OW)) for y, x in inside]
    hang = [(-1, 0), (0, -2), (H - OH + 3, 0), (0, W - OW + 4), (-4, -3), (H - OH + 1, W - OW + 2)]
    sets = []
    for variant in range(max(len(inside), len(hang))):
        rows_in = [inside[(variant + b) % len(inside)] + (OH, OW) for b in range(B)]
        rows_pad = [hang[(variant + b) % len(hang)] + (OH, OW) for b in range(B)]
        sets += [rows_in, rows_pad]
    return sets


# ---------------------------------------------------------------------------------------------------------- stats
def oracle_stats(v):
    """Per image, from the exact integer sums of the uint8 values ``v`` [B, ...]: (fp64 mean, fp64 adj)."""
    out = []
    for img in v:
        n = img.size
        S, Q = int(img.astype(np.int64).sum()), int((img.astype(np.int64) ** 2).sum())
        mean = S / n
        adj = max(np.sqrt(max(Q / n - mean * mean, 0.0)), 1.0 / np.sqrt(float(n)))
        out.append((mean, adj))
    return out


# --------------------------------------------------------------------------------------------------------- resize
def axis_scale(boxn, outn, mapping):
    if mapping == "align_corners":
        return np.float32(boxn - 1) / np.float32(outn - 1) if outn > 1 else np.float32(0.0)
    return np.float32(boxn) / np.float32(outn)


def oracle_resize(img, boxes, flips, OH, OW, mapping):
    """The definition in fp64 from the fp32 scales: ([B, OH, OW, C] fp64 values, the largest |in| per axis pair).
    A box of the output size takes the copy path (zeros outside the image)."""
    B, H, W, C = img.shape
    o = 0.5 if mapping == "half_pixel" else 0.0
    src = img.astype(np.float64)
    out = np.zeros((B, OH, OW, C))
    for b in range(B):
        y0, x0, bh, bw = (int(v) for v in boxes[b])
        if (bh, bw) == (OH, OW):
            out[b] = copy_values(img[b:b + 1], boxes[b:b + 1], flips[b:b + 1], OH, OW)[0]
            continue
        sy, sx = float(axis_scale(bh, OH, mapping)), float(axis_scale(bw, OW, mapping))
        for y in range(OH):
            iny = (y + o) * sy - o
            ylo, yhi, ty = max(int(np.floor(iny)), 0), min(int(np.ceil(iny)), bh - 1), iny - np.floor(iny)
            r0, r1 = min(max(y0 + ylo, 0), H - 1), min(max(y0 + yhi, 0), H - 1)
            for x in range(OW):
                xs = OW - 1 - x if flips[b] else x
                inx = (xs + o) * sx - o
                xlo, xhi, tx = max(int(np.floor(inx)), 0), min(int(np.ceil(inx)), bw - 1), inx - np.floor(inx)
                c0, c1 = min(max(x0 + xlo, 0), W - 1), min(max(x0 + xhi, 0), W - 1)
                top = src[b, r0, c0] + (src[b, r0, c1] - src[b, r0, c0]) * tx
                bot = src[b, r1, c0] + (src[b, r1, c1] - src[b, r1, c0]) * tx
                out[b, y, x] = top + (bot - top) * ty
    return out


def resize_tolerance(want, boxes, inv, bf16):
    """See test_resize_against_fp64 for the derivation.  ``want``: the oracle's scaled output; ``inv``: the largest
    |1 / std|."""
    n = float(max(max(int(b[2]), int(b[3])) for b in boxes) + 1)          # |in| and |in + o| stay below this
    d_in = U * (2.0 * n + 1.0)                                            # per axis
    tol = abs(inv) * (255.0 * 2.0 * d_in + 6.0 * 255.0 * U) + 2.0 * U * np.abs(want)
    if bf16:
        mag = np.maximum(np.abs(want), 2.0 ** -126)
        tol = tol + 2.0 ** (np.floor(np.log2(mag)) - 8.0)                 # half a bf16 ulp of the oracle value
    return tol


def checkerboard(B, H, W, C):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    board = (((y + x) & 1) * 255).astype(np.uint8)
    return np.broadcast_to(board[None, :, :, None], (B, H, W, C)).copy()


def random_images(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, C), generator=g, dtype=torch.uint8).numpy()


# ----------------------------------------------------------------------------------------------------- end to end
def fresh(device):
    """A new variable store on ``device`` (an indexed device on the GPU: the step counter is kept per device)."""
    from mdtf.train import step as S
    from mdtf.train import variables as V
    V.reset_default_graph()
    S.reset()
    store = V.get_store()
    store.device = torch.device("cuda", 0) if device == "cuda" else torch.device("cpu")
    store.compute_dtype = None
    return store


def lenet_step(device, hip_graph, batch=8):
    """LeNet over a uint8 [batch, 28, 28, 1] source, ``cifar_preprocess`` in the tower's ``pre_process_fn``; the
    program also returns a position-weighted checksum of the preprocessed input.  -> (op, loss, checksum, seen)."""
    import mdtf
    from mdtf.data.loaders import SyntheticImageLoader
    from mdtf.models import LeNet, SoftmaxCrossEntropyLoss
    from mdtf.runtime import Net, Tower
    store = fresh(device)
    if device == "cuda":
        store.compute_dtype = torch.bfloat16                 # the conv kernels take bf16 activations
    store.generator.manual_seed(3)
    loader = SyntheticImageLoader(stored_shape=(28, 28, 1), num_classes=10, seed=5)
    loader.batch_size = batch
    raw, gt = loader.load_train_batch()
    seen = []

    class Recording(LeNet):
        def inference(self, x):
            seen.append((x.dtype, tuple(x.shape), x.detach().float().mean((1, 2, 3)).abs().max()))
            return super(Recording, self).inference(x)

    weights = torch.linspace(-1.0, 1.0, 28 * 28).reshape(1, 28, 28, 1)
    holder = {}

    def pre(images, labels, args, kwargs):
        x = mdtf.image.cifar_preprocess(images)              # dtype: the store's compute dtype, fp32 on the CPU
        if "weights" not in holder:                          # uploaded by the building pass, before any capture
            holder["weights"] = weights.to(x.device)
        holder["sum"] = (x.float() * holder["weights"]).sum((1, 2, 3))
        return x, labels

    class Checked(Tower):
        def _forward(self, post_process_fn, args, kwargs):
            inner = Tower._forward(self, post_process_fn, args, kwargs)

            def fn(r, g):
                out = inner(r, g)
                out["checksum"] = holder["sum"]
                return out
            return fn

    base = mdtf.train.MomentumOptimizer(0.01, 0.9)
    tg = []
    tower = Checked(Net(Recording()), "tower_0/", tg, raw, gt, SoftmaxCrossEntropyLoss(), base, pre_process_fn=pre,
                    batch_size=batch)
    _, loss, _ = tower.process()
    opt = mdtf.train.SyncReplicasOptimizer(base, hip_graph=True) if hip_graph else base
    op = opt.apply_gradients(Tower.average_gradients(tg), global_step=mdtf.train.get_or_create_global_step())
    return op, loss, tower.program.output("checksum"), seen
