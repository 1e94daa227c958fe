"""Layer-wise adaptive updates (LAMB, LARS) with the per-layer trust ratios on the device.

The flat update kernels (:mod:`mdtf.ops.optim`) apply one ``[lr, lr_t, grad_scale]`` to a whole group; LAMB and
LARS scale every variable's ("layer's") step by a ratio of L2 norms over that variable.  ``csrc/layerwise.hip``
does it in three kinds of launches and no host read of a norm (the step stays hipGraph-capturable):

* :func:`lamb_moments_` / :func:`lars_norms_` — one launch per update target: the moments (LAMB) and one fp32
  partial pair per work item, ``(sum w^2, sum u^2)`` / ``(sum w^2, sum g^2)``;
* :func:`layer_finalize_` — one launch for all targets, one block per layer: partials summed in a fixed order in
  fp64 into ``sums[2 L]``, then ``ratio[L]`` (modes as :func:`mdtf.ops.gradnorm.clip_finalize_`: sharded replicas
  all-reduce ``sums`` between the halves);
* :func:`lamb_apply_` / :func:`lars_apply_` — one launch per target: the update with ``ratio[layer]`` looked up
  per work item, bf16 shadow refreshed.

Math (``g^ = grad_scale * g``; ``dyn`` = device ``[lr, lr_t, grad_scale]`` overrides the scalars)::

    LAMB   m = b1 m + (1 - b1) g^ ;  v = b2 v + (1 - b2) g^2 ;  u = m / (sqrt(v) + eps) + wd w
           r = |w| / |u| if |w| > 0 and |u| > 0 else 1 ;  w -= lr r u
    LARS   t = eeta |w| / (|g^| + wd |w| + eps) if |w| > 0 and |g^| > 0 else 1
           s = lr t (g^ + wd w) ;  acc = mom acc + s ;  w -= acc   (nesterov: s + mom acc)

Layers without weight decay (``decay`` false) have ratio 1 and ``wd = 0`` whatever ``weight_decay`` is passed.
A non-finite norm gives a NaN ratio: every weight of the layer turns NaN.  Zeros (alignment padding, bucket tails, pad rows) stay zero and add nothing to a norm, so
padding is counted with a neighbouring layer.

A :class:`LayerMap` holds the layers and, per update target, the pieces ``(target_offset, length, layer_id)`` and
the device table of work items (each inside one piece, at most one 16 KiB chunk; a layer's items contiguous).
GPU tensors run the HIP kernels; CPU tensors (and ``MDTF_KERNELS=torch``) the PyTorch reference below: the same
pieces and math, one fp64 partial pair per piece.
"""
import math

import torch

from . import _native

_native.register("mdtf_layerwise_chunk4", [], _native.I)
_native.register("mdtf_lamb_moments", [_native.P, _native.I, _native.I, _native.P, _native.P, _native.P, _native.P,
                                       _native.P, _native.F, _native.F, _native.F, _native.F, _native.F, _native.P,
                                       _native.P])
_native.register("mdtf_lamb_apply", [_native.P, _native.I, _native.P, _native.P, _native.P, _native.P, _native.P,
                                     _native.F, _native.F, _native.F, _native.P, _native.P])
_native.register("mdtf_lars_norms", [_native.P, _native.I, _native.I, _native.P, _native.P, _native.P, _native.P])
_native.register("mdtf_lars_apply", [_native.P, _native.I, _native.P, _native.P, _native.P, _native.P, _native.P,
                                     _native.F, _native.F, _native.F, _native.F, _native.I, _native.P, _native.P])
_native.register("mdtf_layer_finalize", [_native.P, _native.I, _native.P, _native.P, _native.P, _native.I, _native.F,
                                         _native.F, _native.F, _native.F, _native.P, _native.I, _native.P])

FULL, REDUCE, COEF = 0, 1, 2      # layer_finalize_ modes: both halves | partials -> sums | sums -> ratio
LAMB, LARS = 0, 1
CHUNK = 4096                      # elements per work item at most (16 KiB; csrc/layerwise.hip kChunk4 * 4)


def _native_ok(device):
    device = torch.device(device)
    if device.type != "cuda" or _native.mode() == "torch":
        return False
    _native.lib()                 # raise loudly if missing
    return True


class LayerMap(object):
    """Layers and, per update target, the pieces and work items of a layer-wise update.

    ``decay``: one flag per layer (the ratio applies; otherwise it is 1).  ``pieces``: one list per target of
    ``(target_offset, length, layer_id)``; offsets and lengths are multiples of 4 elements, pieces of one target do
    not overlap, and the pieces of one layer are adjacent in ONE target's list (a variable lives in one group, and
    in one bucket of it).  ``names`` (optional) label the layers.  Built once, outside any hipGraph capture."""

    def __init__(self, decay, pieces, device, names=None):
        self.device = torch.device(device)
        self.native = _native_ok(self.device)
        self.decay = [bool(d) for d in decay]
        self.names = list(names) if names is not None else ["layer_%d" % i for i in range(len(self.decay))]
        self.pieces = [[(int(o), int(n), int(l)) for o, n, l in ps] for ps in pieces]
        chunk = CHUNK
        if self.native:
            chunk = 4 * int(_native.fn("mdtf_layerwise_chunk4")())
        nl = len(self.decay)
        first, count = [0] * nl, [0] * nl
        self.items, self.pbase = [], []       # per target: [(off, len, layer)] and its first partial pair
        total, closed, last = 0, set(), None
        for ps in self.pieces:
            self.pbase.append(total)
            items = []
            for o, n, l in ps:
                if o % 4 or n % 4 or n < 0 or o < 0 or not 0 <= l < nl:
                    raise ValueError("layer piece (%d, %d, %d): offsets and lengths are multiples of 4 elements and "
                                     "the layer one of %d" % (o, n, l, nl))
                if n == 0:
                    continue
                if l != last:
                    if l in closed:
                        raise ValueError("the pieces of layer %d are not adjacent in one target" % l)
                    if last is not None:
                        closed.add(last)
                    first[l], last = total + len(items), l
                step = chunk if self.native else n
                for s in range(0, n, step):
                    items.append((o + s, min(step, n - s), l))
                count[l] = total + len(items) - first[l]
            if last is not None:              # a layer never continues in the next target
                closed.add(last)
                last = None
            spans = sorted((o, o + n) for o, n, _ in items)
            for (a0, a1), (b0, _) in zip(spans, spans[1:]):
                if b0 < a1:
                    raise ValueError("layer pieces of one target overlap at element %d" % b0)
            self.items.append(items)
            total += len(items)
        self.num_items = total
        self.num_layers = nl
        self.first, self.count = first, count
        self.extent = [max([o + n for o, n, _ in it] or [0]) for it in self.items]
        self.item_tables, self.layer_table = None, None
        if self.native:
            if any(e // 4 > 0x7fffffff for e in self.extent) or total > 0x7fffffff:
                raise ValueError("layer-wise update: a target of more than 2^33 elements")
            rows = [[[o // 4, n // 4, l, int(self.decay[l])] for o, n, l in it] or [[0, 0, 0, 0]] for it in self.items]
            self.item_tables = [torch.tensor(r, dtype=torch.int32).to(self.device) for r in rows]
            self.layer_table = torch.tensor([[first[i], count[i], int(self.decay[i]), 0] for i in range(nl)]
                                            or [[0, 0, 0, 0]], dtype=torch.int32).to(self.device)

    def bytes_per_call(self, streams):
        """Bytes one launch over every target moves: ``streams`` fp32 streams (+ nothing for the shadow)."""
        return 4 * streams * sum(n for it in self.items for _, n, _ in it)


def group_pieces(group, first_layer=0):
    """Pieces of a whole flat group (all-reduce mode): variable i owns its slot ``[offsets[i], offsets[i + 1])``,
    alignment and bucket padding (zeros) included.  Returns ``(pieces, names)``; layer ids count from
    ``first_layer`` in the group's variable order."""
    ends = list(group.offsets[1:]) + [group.numel]
    pieces = [(o, e - o, first_layer + i) for i, (o, e) in enumerate(zip(group.offsets, ends))]
    return pieces, [v.name for v in group.variables]


def shard_pieces(group, rank, first_layer=0):
    """Pieces of ``rank``'s shard buffer of a group (sharded mode): bucket ``b``'s range ``[b.start + rank *
    b.shard_len, + b.shard_len)`` lives at ``b.shard_offset`` of the shard buffer; a variable's piece is its slot
    cut to that range (none when the slot lies in other ranks' shards)."""
    full, names = group_pieces(group, first_layer)
    out = []
    for b in group.buckets:
        lo = b.start + rank * b.shard_len
        hi = lo + b.shard_len
        for o, n, l in full:
            s, e = max(o, lo), min(o + n, hi)
            if s < e:
                out.append((b.shard_offset + s - lo, e - s, l))
    return out, names


def map_for_targets(targets, reducer):
    """The :class:`LayerMap` of a train op's update targets (``GradReducer.update_targets``): one layer per
    variable, numbered over the groups in order."""
    decay, names, pieces = [], [], []
    for t in targets:
        g = t.group
        if t.key == "shard":
            ps, ns = shard_pieces(g, reducer.rank, len(decay))
        else:
            ps, ns = group_pieces(g, len(decay))
        pieces.append(ps)
        names += ns
        decay += [bool(g.decay)] * len(ns)
    return LayerMap(decay, pieces, targets[0].master.device, names)


class LayerBuffers(object):
    """Persistent buffers of one layer-wise train op: item partials (fp32 pairs on the GPU, one fp64 pair per piece
    on the reference path), ``sums`` (fp64[2 L], what sharded replicas all-reduce) and ``ratio`` (fp32[L]).
    Allocated once, outside any hipGraph capture."""

    def __init__(self, lmap):
        dev = lmap.device
        self.native = lmap.native
        self.partials = torch.zeros(2 * max(lmap.num_items, 1), dtype=torch.float32 if self.native else torch.float64,
                                    device=dev)
        self.sums = torch.zeros(2 * max(lmap.num_layers, 1), dtype=torch.float64, device=dev)
        self.ratio = torch.ones(max(lmap.num_layers, 1), dtype=torch.float32, device=dev)


def state_for(targets, reducer):
    """``(LayerMap, LayerBuffers)`` of a reducer's update targets, built by the first (eager) step and kept on the
    reducer; never allocated inside a hipGraph capture."""
    if reducer is None:
        raise ValueError("a layer-wise update needs the train op's reducer (rank, shard layout, where its buffers live)")
    st = getattr(reducer, "layer_state", None)
    if st is None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("layer-wise optimizer buffers must be allocated by an eager step before capture")
        lmap = map_for_targets(targets, reducer)
        st = reducer.layer_state = (lmap, LayerBuffers(lmap))
    return st


def _check(lmap, ti, *tensors):
    if not 0 <= ti < len(lmap.items):
        raise ValueError("target %d of a layer map over %d targets" % (ti, len(lmap.items)))
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < lmap.extent[ti]:
            raise ValueError("layer-wise update needs contiguous fp32 buffers of at least %d elements, got %s x %d"
                             % (lmap.extent[ti], t.dtype, t.numel()))
        if t.device.type != lmap.device.type:
            raise ValueError("layer map on %s, buffer on %s" % (lmap.device, t.device))


def _check_shadow(lmap, ti, shadow):
    if shadow is not None and (not shadow.is_contiguous() or shadow.numel() < lmap.extent[ti]
                               or (lmap.native and shadow.dtype != torch.bfloat16)):
        raise ValueError("layer-wise update: the shadow must be a contiguous bf16 buffer of the target's size")


def _dyn(dyn, lr, gs):
    """(lr, grad_scale) as fp32-rounded Python floats, from ``dyn`` when given (reference path)."""
    if dyn is not None:
        d = dyn.to(torch.float32).tolist()
        return d[0], d[2]
    return (float(torch.tensor(float(lr), dtype=torch.float32)),
            float(torch.tensor(float(gs), dtype=torch.float32)))


def _lamb_u(m, v, w, eps, wd):
    u = m / (v.sqrt() + eps)
    return u + wd * w if wd else u


def lamb_moments_(lmap, buf, ti, w, g, m, v, beta1, beta2, epsilon, grad_scale=1.0, weight_decay=0.0, dyn=None):
    """Target ``ti``: update ``m``, ``v`` in place and write the partial pairs ``(sum w^2, sum u^2)``."""
    _check(lmap, ti, w, g, m, v)
    if lmap.native:
        _native.check(_native.fn("mdtf_lamb_moments")(
            _native.ptr(lmap.item_tables[ti]), len(lmap.items[ti]), lmap.pbase[ti], _native.ptr(w), _native.ptr(g),
            _native.ptr(m), _native.ptr(v), _native.ptr(buf.partials), float(beta1), float(beta2), float(epsilon),
            float(grad_scale), float(weight_decay), _native.ptr(dyn), _native.stream_ptr()), "lamb_moments")
        return
    _, gs = _dyn(dyn, 0.0, grad_scale)
    for k, (o, n, l) in enumerate(lmap.items[ti]):
        gh = g[o:o + n] * gs
        mm, vv, ww = m[o:o + n], v[o:o + n], w[o:o + n]
        mm.mul_(beta1).add_(gh, alpha=1 - beta1)
        vv.mul_(beta2).addcmul_(gh, gh, value=1 - beta2)
        u = _lamb_u(mm, vv, ww, epsilon, weight_decay if lmap.decay[l] else 0.0)
        buf.partials[2 * (lmap.pbase[ti] + k)] = ww.double().pow(2).sum()
        buf.partials[2 * (lmap.pbase[ti] + k) + 1] = u.double().pow(2).sum()


def lars_norms_(lmap, buf, ti, w, g):
    """Target ``ti``: the partial pairs ``(sum w^2, sum g^2)`` (the raw gradient; the finalize applies the scale)."""
    _check(lmap, ti, w, g)
    if lmap.native:
        _native.check(_native.fn("mdtf_lars_norms")(
            _native.ptr(lmap.item_tables[ti]), len(lmap.items[ti]), lmap.pbase[ti], _native.ptr(w), _native.ptr(g),
            _native.ptr(buf.partials), _native.stream_ptr()), "lars_norms")
        return
    for k, (o, n, _) in enumerate(lmap.items[ti]):
        buf.partials[2 * (lmap.pbase[ti] + k)] = w[o:o + n].double().pow(2).sum()
        buf.partials[2 * (lmap.pbase[ti] + k) + 1] = g[o:o + n].double().pow(2).sum()


def layer_finalize_(lmap, buf, kind, eeta=1e-3, weight_decay=0.0, epsilon=0.0, grad_scale=1.0, dyn=None, mode=FULL):
    """``buf.partials`` -> ``buf.sums`` -> ``buf.ratio`` for every layer of every target (one launch).  ``kind``:
    :data:`LAMB` or :data:`LARS` (``eeta``, ``weight_decay``, ``epsilon``, ``grad_scale`` / ``dyn[2]`` are LARS's)."""
    if kind not in (LAMB, LARS) or mode not in (FULL, REDUCE, COEF):
        raise ValueError("layer_finalize_: kind %r, mode %r" % (kind, mode))
    if lmap.native:
        _native.check(_native.fn("mdtf_layer_finalize")(
            _native.ptr(lmap.layer_table), lmap.num_layers, _native.ptr(buf.partials), _native.ptr(buf.sums),
            _native.ptr(buf.ratio), int(kind), float(eeta), float(weight_decay), float(epsilon), float(grad_scale),
            _native.ptr(dyn), int(mode), _native.stream_ptr()), "layer_finalize")
        return
    nl = lmap.num_layers
    if mode != COEF:
        pairs = buf.partials.view(-1, 2)
        for l in range(nl):
            buf.sums[2 * l:2 * l + 2] = pairs[lmap.first[l]:lmap.first[l] + lmap.count[l]].sum(0)   # fixed order
        if mode == REDUCE:
            return
    _, gs = _dyn(dyn, 0.0, grad_scale)
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))      # noqa: E731 (the kernel's fp32 arguments)
    eeta, wd, eps = f32(eeta), f32(weight_decay), f32(epsilon)
    sums = buf.sums.tolist()
    out = []
    for l in range(nl):
        sa, sb = sums[2 * l], sums[2 * l + 1]
        r = 1.0
        if lmap.decay[l]:
            if not (math.isfinite(sa) and math.isfinite(sb)):
                r = float("nan")
            else:
                wn = math.sqrt(sa)
                if kind == LAMB:
                    un = math.sqrt(sb)
                    if wn > 0 and un > 0:
                        r = wn / un
                else:
                    gn = gs * math.sqrt(sb)
                    if not math.isfinite(gn):
                        r = float("nan")
                    elif wn > 0 and gn > 0:
                        r = eeta * wn / (gn + wd * wn + eps)
        out.append(r)
    if nl:
        buf.ratio[:nl] = torch.tensor(out, dtype=torch.float64).to(torch.float32)


def lamb_apply_(lmap, buf, ti, w, m, v, shadow, lr, epsilon, weight_decay=0.0, dyn=None):
    """Target ``ti``: ``w -= lr * ratio[layer] * u`` with ``u`` recomputed from the updated moments and the old
    ``w``; refresh ``shadow`` if given."""
    _check(lmap, ti, w, m, v)
    _check_shadow(lmap, ti, shadow)
    if lmap.native:
        _native.check(_native.fn("mdtf_lamb_apply")(
            _native.ptr(lmap.item_tables[ti]), len(lmap.items[ti]), _native.ptr(w), _native.ptr(m), _native.ptr(v),
            _native.ptr(shadow), _native.ptr(buf.ratio), float(lr), float(epsilon), float(weight_decay),
            _native.ptr(dyn), _native.stream_ptr()), "lamb_apply")
        return
    lr, _ = _dyn(dyn, lr, 1.0)
    lr = torch.tensor(lr, dtype=torch.float32)
    for o, n, l in lmap.items[ti]:
        ww = w[o:o + n]
        ww.sub_((lr * buf.ratio[l]) * _lamb_u(m[o:o + n], v[o:o + n], ww, epsilon,
                                              weight_decay if lmap.decay[l] else 0.0))
        if shadow is not None:
            shadow[o:o + n].copy_(ww)


def lars_apply_(lmap, buf, ti, w, g, acc, shadow, lr, momentum, grad_scale=1.0, weight_decay=0.0, nesterov=False,
                dyn=None):
    """Target ``ti``: ``s = lr * ratio[layer] * (g^ + wd w)``; ``acc = momentum * acc + s``; ``w -= acc``
    (nesterov: ``s + momentum * acc``); refresh ``shadow`` if given."""
    _check(lmap, ti, w, g, acc)
    _check_shadow(lmap, ti, shadow)
    if lmap.native:
        _native.check(_native.fn("mdtf_lars_apply")(
            _native.ptr(lmap.item_tables[ti]), len(lmap.items[ti]), _native.ptr(w), _native.ptr(g), _native.ptr(acc),
            _native.ptr(shadow), _native.ptr(buf.ratio), float(lr), float(momentum), float(grad_scale),
            float(weight_decay), int(bool(nesterov)), _native.ptr(dyn), _native.stream_ptr()), "lars_apply")
        return
    lr, gs = _dyn(dyn, lr, grad_scale)
    lr = torch.tensor(lr, dtype=torch.float32)
    for o, n, l in lmap.items[ti]:
        ww, aa = w[o:o + n], acc[o:o + n]
        gh = g[o:o + n] * gs
        if weight_decay and lmap.decay[l]:
            gh = gh + weight_decay * ww
        s = (lr * buf.ratio[l]) * gh
        aa.mul_(momentum).add_(s)
        ww.sub_(s + momentum * aa if nesterov else aa)
        if shadow is not None:
            shadow[o:o + n].copy_(ww)
