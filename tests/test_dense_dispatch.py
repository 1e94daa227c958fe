"""Dense-layer dispatch pinned launch for launch, on the CPU.

``mdtf.ops.gemm`` runs on CPU tensors that claim to be on the device (``_Dev``) when ``N.fn`` is the recorder
of ``test_conv_dispatch``: every native launch, every library product (``torch.mm`` / ``torch.addmm``), every
``torch.cat``, every column sum and every gradient-slot declaration a forward / backward of ``_Dense`` issues is
recorded, with pointers by the name of the scenario tensor they alias.  Buffers the code under test allocates
(``torch.empty`` / ``torch.empty_like``) and library results are named in order of creation (``e0``, ``mm1``, ...).
Each scenario also records which returned gradients are ``None``, markers or tensors, the state of the
activation-gradient sink and of ffn()'s link (``fused``).

The expected traces in ``tests/fixtures/dense_dispatch_trace.json`` were recorded with this module before
``_Dense`` was restructured; the tests assert exact equality, so the routing of a dense product cannot change
unnoticed.  ``MDTF_PP_FWD=act`` is the shipped default: every ``default/`` scenario runs under it.

Not pinned: the body of ``_wgrad_section`` past its guard (it needs real streams), the ``_fp32_out_ok``
``except`` branch of ``_accum_mm`` (which of its two arms runs depends on the torch build: every scenario starts
with the question open, and the trace shows the ``torch.addmm`` attempt and, where it is refused, the ``torch.mm``
after it), and the torch-version ``except`` in ``_TiedDecoder.backward``.

Regenerate (only when dispatch behaviour is meant to change)::

    python tests/test_dense_dispatch.py --regen
"""
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_conv_dispatch as D  # noqa: E402
from mdtf.ops import _native as N  # noqa: E402
from mdtf.ops import actsink  # noqa: E402
from mdtf.ops import conv as C  # noqa: E402
from mdtf.ops import gemm, kernels, mm, tunable  # noqa: E402
from mdtf.parallel.flat import FlatGroup  # noqa: E402
from mdtf.train import variables as V  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "dense_dispatch_trace.json")
BF16 = torch.bfloat16
DECLINED = -2            # MdtfStatus "unsupported configuration": the shape is not taken


class _Dev(torch.Tensor):
    """A CPU tensor that claims to be on the device (``_Dense`` tests ``x.is_cuda`` itself)."""
    is_cuda = property(lambda self: True)


class Recorder(D.Recorder):
    """The conv harness's recorder; the kernels named in ``decline`` return "shape not taken"."""

    def __init__(self):
        super().__init__()
        self.decline = ()
        self.made = 0

    def fn(self, name):
        call = super().fn(name)
        if name not in self.decline:
            return call

        def declined(*args):
            call(*args)
            self.calls[-1].append("-> %d" % DECLINED)
            return DECLINED
        return declined

    def where(self, t):
        if t is None:
            return "null"
        return self._resolve(t if isinstance(t, int) else t.data_ptr()) or "ptr"

    def made_by(self, kind, t):
        """Name a tensor the code under test made (kept alive: no later allocation takes its address)."""
        if t.numel() and self._resolve(t.data_ptr()) is None:
            self.name("%s%d" % (kind, self.made), t)
            self.made += 1
        return t


# the flags the environment sets at import, at their shipped defaults
DEFAULTS = (
    (gemm, dict(DENSE="pp", PP=True, PP_FWD="act", PP_DGRAD="fused", PP_FWD_SHAPES={"768x768"},
                PP_DGRAD_SHAPES={"768x768"}, PP_WGRAD="wg", DENSE_WGRAD_STREAM=False, FFN_FUSE=True,
                ACT_DGRAD_CORE=False, FWD_MODE="auto", HAND_FWD=True, FWD_TILES={}, HAND_WGRAD=True,
                HAND_DGRAD=False, FUSED_BIAS_GRAD=True, DGRAD_ACT_TILES={(3072, 768): (128, 256, 3, 3)},
                _fp32_out_ok=None)),
    (mm, dict(TILES={}, WG_SK=False, _WG_STAGES=None,
              WG_TILES={(768, 2304, 8192): (128, 2, 4), (768, 3072, 8192): (128, 2, 3),
                        (3072, 768, 8192): (128, 2, 3), (768, 768, 8192): (128, 2, 6),
                        (1024, 3072, 8192): (256, 3, 2), (1024, 4096, 8192): (256, 3, 2),
                        (4096, 1024, 8192): (256, 3, 2)})),
    (C, dict(_SLAB_MODE="dense", WGRAD_SLAB=False, DENSE_WGRAD_SLAB=True, WGRAD_INK=False, SLAB_SIDE=False)),
    (V, dict(STORE_FIRST=True, GRAD_EPOCH=[1])), (N, dict(_DETERMINISTIC=False)), (actsink, dict(ENABLED=True)))
MODULES = {"gemm": gemm, "mm": mm, "V": V, "N": N, "actsink": actsink, "C": C}


class Scenario(object):
    """One scenario's state: the recorder, the patches and the named tensors."""

    def __init__(self, mp, flags=None, decline=(), env=None):
        self.mp = mp
        self.rec = rec = Recorder()
        rec.decline = tuple(decline)
        self.out = {}
        self.links = []
        mp.setattr(N, "fn", rec.fn)
        mp.setattr(N, "stream_ptr", lambda device=None: N.P(0))
        mp.setattr(N, "use_native", lambda *tensors: True)
        mp.setattr(tunable, "ensure", lambda device: None)
        for mod, values in DEFAULTS:
            for flag, value in values.items():
                mp.setattr(mod, flag, value)
        for var in ("MDTF_WG_SQUARE", "MDTF_WEIGHT_CAT_CACHE", "MDTF_PP_FWD_TILE", "MDTF_WG_FFN_OUT"):
            mp.delenv(var, raising=False)
        for var, value in (env or {}).items():
            mp.setenv(var, value)
        mp.setattr(gemm, "_CATS", gemm._WeightCats())
        for flag, value in (flags or {}).items():
            mod, _, name = flag.rpartition(".")
            mp.setattr(MODULES[mod or "gemm"], name, value)

        def colsum_into(x2d, out):
            rec.note("kernels.colsum_into", list(x2d.shape), rec.where(x2d), rec.where(out))
            return out.add_(x2d.float().sum(0))

        def colsum(x2d):
            rec.note("kernels.colsum", list(x2d.shape), rec.where(x2d))
            return rec.made_by("colsum", x2d.float().sum(0))
        mp.setattr(kernels, "colsum_into", colsum_into)
        mp.setattr(kernels, "colsum", colsum)
        for name in ("mm", "addmm", "cat"):
            mp.setattr(torch, name, self._library(name, getattr(torch, name)))
        for name in ("empty", "empty_like"):
            mp.setattr(torch, name, self._allocator(getattr(torch, name)))
        real_arr = mm._arr

        def arr(ts):
            rec.note("mm._arr", [rec.where(t) for t in ts])
            return real_arr(ts)
        mp.setattr(mm, "_arr", arr)
        for name in ("claim_store", "note_accumulate", "unclaim_store"):
            mp.setattr(V, name, self._noted(name, getattr(V, name)))
        real_backward = gemm._Dense.backward      # autograd hands the reshaped output's gradient on as a plain tensor
        mp.setattr(gemm._Dense, "backward", staticmethod(lambda ctx, dy: real_backward(ctx, dy.as_subclass(_Dev))))
        real_link = gemm._ActLink

        def link():
            self.links.append(real_link())
            return self.links[-1]
        mp.setattr(gemm, "_ActLink", link)

    def _library(self, name, real):
        rec = self.rec

        def call(*args, **kwargs):
            ops = args[0] if name == "cat" else [a for a in args if isinstance(a, torch.Tensor)]
            extra = {k: (rec.where(v) if isinstance(v, torch.Tensor) else str(v)) for k, v in kwargs.items()}
            if name == "cat" and len(args) > 1:
                extra["dim"] = args[1]
            rec.note("torch." + name, *([list(t.shape), rec.where(t)] for t in ops), *([extra] if extra else []))
            return rec.made_by(name, real(*args, **kwargs))
        return call

    def _allocator(self, real):
        def call(*args, **kwargs):
            return self.rec.made_by("e", real(*args, **kwargs).as_subclass(_Dev))
        return call

    def _noted(self, name, real):
        def call(var):
            r = real(var)
            self.rec.note("V." + name, getattr(var, "name", None), *([bool(r)] if name == "claim_store" else []))
            return r
        return call

    def t(self, name, shape, dtype=BF16, grad=False):
        t = torch.zeros(tuple(shape), dtype=dtype).as_subclass(_Dev)
        if grad:
            t.requires_grad_(True)
        return self.rec.name(name, t)

    def params(self, specs, want_grad=True):
        """``specs``: (name, shape, in a slot?) or None -> the tensors the model computes with.  Those in a slot
        are the bf16 shadows of real Variables of one FlatGroup (their fp32 gradient slots named ``<name>.grad``);
        the others plain leaves (biases fp32, as a variable kept in fp32 reads)."""
        vs = {sp[0]: V.Variable(sp[0], torch.zeros(sp[1])) for sp in specs if sp is not None and sp[2]}
        self.group = FlatGroup(list(vs.values()), "cpu", BF16, False) if vs else None
        out = []
        for sp in specs:
            if sp is None:
                out.append(None)
                continue
            name, shape, slot = sp
            if slot:
                t = self.rec.name(name, vs[name].shadow.as_subclass(_Dev))
                t.requires_grad_(want_grad)
                t._mdtf_var = vs[name]
                self.rec.name(name + ".grad", vs[name].grad)
            else:
                t = self.t(name, shape, BF16 if len(shape) == 2 else torch.float32, grad=want_grad)
            out.append(t)
        return out

    def backward(self, y, inputs, names):
        self.rec.note("--backward")
        dy = self.t("dy", y.shape)
        keep = [(n, t) for n, t in zip(names, inputs) if t is not None and t.requires_grad]
        grads = torch.autograd.grad([y], [t for _, t in keep], [dy], allow_unused=True) if keep else ()
        self.out["grads"] = {n: (None if g is None else "marker" if V._is_marker(g)
                                 else [list(g.shape), str(g.dtype), self.rec.where(g)])
                             for (n, _), g in zip(keep, grads)}

    def result(self):
        self.out["calls"] = self.rec.finish()
        self.out["links"] = [[ln.fused, ln.pre is None, ln.act] for ln in self.links]
        return self.out


def _per_segment(v, nseg):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * nseg


def case(s, entry="dense", T=4096, K=128, n=128, act=None, nseg=1, wslot=True, bslot=True, bias=True, sink=None,
         x_grad=True, w_grad=True, raises=False):
    """Forward and backward of one entry point.  ``wslot`` / ``bslot``: which weights / biases have fp32
    gradient slots (one flag, or one per segment); ``sink``: None | "first" | "acc", the state the input's
    activation-gradient sink is in when this layer contributes."""
    trans = entry in ("trans", "apply_trans")
    nseg = 2 if entry == "ffn" else nseg
    wslot, bslot = _per_segment(wslot, nseg), _per_segment(bslot, nseg)
    wshape = (n, K) if trans else (K, n)
    specs = [("w%d" % j, (n, K) if entry == "ffn" and j == 1 else wshape, wslot[j]) for j in range(nseg)]
    specs += [("b%d" % j, (K if entry == "ffn" and j == 1 else n,), bslot[j]) if bias else None for j in range(nseg)]
    names = ["x"] + [sp[0] for sp in specs[:nseg]] + ["b%d" % j for j in range(nseg)]
    wb = s.params(specs, w_grad)
    ws, bs = wb[:nseg], wb[nseg:]
    x = s.t("x", (T, K), grad=x_grad)
    xs = actsink.attach(x) if sink else None
    try:
        if entry == "dense":
            y = gemm.dense(x, ws[0], bs[0], act)
        elif entry == "multi":
            y = gemm.dense_multi(x, ws, bs, act)
        elif entry == "trans":
            y = gemm.dense_transposed(x, ws[0], bs[0])
        elif entry == "ffn":
            y = gemm.ffn(x, ws[0], bs[0], ws[1], bs[1], act)
        else:           # dense_transposed() hands no sink on: the autograd function itself, with one
            y = gemm._Dense.apply(x, 0, True, 1, xs, tuple(x.shape), None, None, ws[0], bs[0])
        s.out["y"] = [list(y.shape), s.rec.where(y)]
        if xs is not None:
            xs.register()
            if sink == "acc":
                xs.register()
                xs.adopt_or_add(s.t("sink_buf", x.shape))
        s.backward(y, [x] + wb, names)
    except RuntimeError as e:
        if not raises:
            raise
        s.out["raised"] = str(e)
    if xs is not None:
        s.out["sink"] = [xs.count, s.rec.where(xs.buf)]


def cats_case(s, active=True):
    """q|k|v forwards of two "steps": the first registers the group with the weight-cat cache (one torch.cat),
    the second refreshes every registered group with one batched copy launch."""
    if not active:
        s.mp.setenv("MDTF_WEIGHT_CAT_CACHE", "0")
    s.mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    wb = s.params([("w%d" % j, (128, 128), True) for j in range(3)] + [("b%d" % j, (128,), True) for j in range(3)])
    s.mp.setattr(V.get_store(), "flat", types.SimpleNamespace(groups=[s.group]))
    x = s.t("x", (2048, 128))
    for step in (1, 2):
        s.rec.note("--step", step)
        gemm._CATS.step_begin()
        y = gemm.dense_multi(x, wb[:3], wb[3:])
        gemm._CATS.step_end()
    s.out["y"] = [list(y.shape), s.rec.where(y)]
    s.out["cats"] = [len(gemm._CATS.entries), gemm._CATS.desc is not None]


SCENARIOS = {}


def scenario(name, fn=case, flags=None, decline=(), env=None, **kwargs):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, dict(flags=flags, decline=decline, env=env), kwargs)


T2, SMALL = 2048, 256                      # below _wg_ok's floor / below every M threshold of the tile tables
ENTRIES = {
    "dense/none": dict(), "dense/relu": dict(act="relu"), "dense/gelu": dict(act="gelu"),
    "multi/none": dict(entry="multi", nseg=3), "multi/gelu": dict(entry="multi", nseg=3, act="gelu"),
    "trans": dict(entry="trans", n=192), "trans100": dict(entry="trans", n=100), "trans256": dict(entry="trans", n=256),
    "ffn/gelu": dict(entry="ffn", act="gelu"), "ffn/relu": dict(entry="ffn", act="relu"),
}
SLOTS = {"noslots": dict(wslot=False, bslot=False), "wslot_only": dict(bslot=False), "nobias": dict(bias=False),
         "noslots_nobias": dict(wslot=False, bias=False)}
SHAPES_ON = {"PP_FWD_SHAPES": {"128x128", "128x384"}, "PP_DGRAD_SHAPES": {"128x128", "384x128"}}
LEGACY = {"DENSE": "legacy", "PP": False}


def family(prefix, entries, flags=None, **kwargs):
    for e in entries:
        scenario("%s/%s" % (prefix, e), flags=flags, **dict(ENTRIES[e], **kwargs))


# ---- the shipped defaults: every entry point, both token counts, every gradient destination, every sink state
family("default", ENTRIES)
family("default/t2048", ENTRIES, T=T2)
family("default/t256", ["dense/none", "dense/gelu", "multi/none"], T=SMALL)
for _slots, _kw in SLOTS.items():
    family("default/" + _slots, ["dense/none", "dense/gelu", "multi/none", "multi/gelu", "trans", "ffn/gelu"], **_kw)
    family("default/t2048/" + _slots, ["dense/none", "dense/gelu", "multi/none", "multi/gelu"], T=T2, **_kw)
for _sink in ("first", "acc"):
    family("default/sink_" + _sink, ["dense/none", "dense/gelu", "multi/none", "multi/gelu", "ffn/gelu"], sink=_sink)
    scenario("default/sink_%s/apply_trans" % _sink, entry="apply_trans", n=192, sink=_sink)
family("default/x_no_grad", ["dense/none", "dense/gelu", "ffn/gelu"], x_grad=False)
family("default/w_no_grad", ["dense/none", "dense/gelu", "multi/none"], w_grad=False, wslot=False, bslot=False)
scenario("default/n100/dense", n=100)
scenario("default/n100/multi", entry="multi", nseg=3, n=100)
scenario("default/n100/multi/gelu", entry="multi", nseg=3, n=100, act="gelu")
scenario("default/mixed_slots/multi", entry="multi", nseg=3, T=T2, wslot=(True, False, True))
scenario("default/mixed_slots/multi/gelu", entry="multi", nseg=3, T=T2, act="gelu", wslot=(True, False, True),
         bslot=(True, False, True))
scenario("default/wgrad_tile_table", T=4096, flags={"PP_WGRAD": "none",
                                                    "DENSE_WGRAD_TILES": {(128, 128): (64, 128, 4, True)}})
scenario("default/wg_square_off", env={"MDTF_WG_SQUARE": "0"})
scenario("default/shapes_on/dense/none", flags=SHAPES_ON)
scenario("default/shapes_on/multi/none", flags=SHAPES_ON, entry="multi", nseg=3)
for _sink in ("first", "acc"):
    family("default/shapes_on/sink_" + _sink, ["dense/none", "dense/gelu", "multi/none"], flags=SHAPES_ON, sink=_sink)

# ---- each flag alone on top of the defaults -------------------------------------------------------------------
family("legacy", ENTRIES, flags=LEGACY)
family("legacy/t2048", ["dense/none", "multi/none", "ffn/gelu"], flags=LEGACY, T=T2)
for _sink in ("first", "acc"):
    family("legacy/sink_" + _sink, ["dense/none", "multi/none"], flags=LEGACY, sink=_sink)
    scenario("legacy/sink_%s/apply_trans" % _sink, flags=LEGACY, entry="apply_trans", n=192, sink=_sink)
for _slots in ("noslots", "wslot_only", "nobias"):
    family("legacy/" + _slots, ["dense/none", "multi/gelu", "trans"], flags=LEGACY, **SLOTS[_slots])
for _v in ("all", "fused", "none"):
    family("pp_fwd=" + _v, ENTRIES, flags={"PP_FWD": _v})
    family("pp_fwd=%s/noslots" % _v, ["dense/gelu", "multi/none", "trans"], flags={"PP_FWD": _v}, **SLOTS["noslots"])
    family("pp_fwd=%s/nobias" % _v, ["dense/none", "multi/none", "trans"], flags={"PP_FWD": _v}, **SLOTS["nobias"])
family("pp_fwd=act", ["dense/none", "dense/gelu"], flags={"PP_FWD": "act"})
for _sink in ("first", "acc"):
    scenario("pp_fwd=all/sink_%s/apply_trans" % _sink, flags={"PP_FWD": "all"}, entry="apply_trans", n=192,
             sink=_sink)
    scenario("pp_fwd=all/sink_%s/apply_trans100" % _sink, flags={"PP_FWD": "all"}, entry="apply_trans", n=100,
             sink=_sink)
for _v in ("all", "none"):
    family("pp_dgrad=" + _v, ["dense/gelu", "multi/gelu", "ffn/gelu"], flags={"PP_DGRAD": _v})
    family("pp_dgrad=%s/pp_fwd=all" % _v, ["dense/none", "ffn/gelu"], flags={"PP_DGRAD": _v, "PP_FWD": "all"})
    for _sink in ("first", "acc"):
        family("pp_dgrad=%s/sink_%s" % (_v, _sink), ["dense/gelu", "multi/gelu"], flags={"PP_DGRAD": _v},
               sink=_sink)
family("pp_dgrad=fused", ["dense/gelu", "multi/gelu"], flags={"PP_DGRAD": "fused"})
for _v in ("all", "none"):
    family("pp_wgrad=" + _v, ["dense/none", "dense/gelu", "multi/gelu", "ffn/gelu"], flags={"PP_WGRAD": _v})
    family("pp_wgrad=%s/pp_fwd=all" % _v, ["trans", "trans100", "trans256", "multi/none"],
           flags={"PP_WGRAD": _v, "PP_FWD": "all"})
    family("pp_wgrad=%s/pp_fwd=all/nobias" % _v, ["trans256", "dense/none"], flags={"PP_WGRAD": _v, "PP_FWD": "all"},
           bias=False)
    family("pp_wgrad=%s/wslot_only" % _v, ["dense/gelu", "multi/gelu"], flags={"PP_WGRAD": _v}, bslot=False)
    family("pp_wgrad=%s/noslots" % _v, ["dense/gelu", "multi/gelu"], flags={"PP_WGRAD": _v}, **SLOTS["noslots"])
family("pp_wgrad=wg", ["dense/none", "dense/gelu"], flags={"PP_WGRAD": "wg"})
HAND_HIT = {"HAND_DGRAD": True, "DGRAD_TILES": {(128, 128): (128, 128, 2, 2), (128, 384): (128, 256, 2, 3)}}
family("hand_dgrad/hit", ["dense/none", "multi/none", "trans", "ffn/gelu"], flags=HAND_HIT)
family("hand_dgrad/hit/t256", ["dense/none"], flags=HAND_HIT, T=SMALL)
family("hand_dgrad/hit/legacy", ["dense/none", "dense/gelu", "multi/none"], flags=dict(HAND_HIT, **LEGACY))
family("hand_dgrad/miss", ["dense/none", "multi/none"], flags={"HAND_DGRAD": True})
for _sink in ("first", "acc"):
    family("hand_dgrad/hit/sink_" + _sink, ["dense/none"], flags=HAND_HIT, sink=_sink)
    family("hand_dgrad/miss/sink_" + _sink, ["dense/none"], flags={"HAND_DGRAD": True}, sink=_sink)
for _mode, _hand in (("mdtf", True), ("hipblaslt", False)):
    _f = dict(LEGACY, FWD_MODE=_mode, HAND_FWD=_hand)
    family("legacy/fwd=" + _mode, ["dense/none", "dense/relu", "dense/gelu", "multi/none", "trans", "ffn/gelu"],
           flags=_f)
    family("legacy/fwd=%s/t256" % _mode, ["dense/gelu", "multi/none"], flags=_f, T=SMALL)
    family("legacy/fwd=%s/nobias" % _mode, ["dense/none"], flags=_f, bias=False)
    scenario("legacy/fwd=%s/n192" % _mode, flags=_f, n=192)
    scenario("legacy/fwd=%s/n192/t256" % _mode, flags=_f, n=192, T=SMALL)
    scenario("legacy/fwd=%s/n100" % _mode, flags=_f, n=100)
    family("fwd=" + _mode, ["dense/none", "multi/none"], flags={"FWD_MODE": _mode, "HAND_FWD": _hand})
FWD_TABLE = {"FWD_TILES": {(128, 128, 1): (128, 128, 3, 2), (128, 128, 3): (128, 256, 2, 3)}}
family("fwd_tiles", ["dense/none", "dense/gelu", "multi/none"], flags=FWD_TABLE)
family("fwd_tiles/t256", ["dense/none"], flags=FWD_TABLE, T=SMALL)
family("fwd_tiles/legacy", ["dense/gelu", "multi/none"], flags=dict(FWD_TABLE, **LEGACY))
family("act_dgrad_core", ["ffn/gelu", "ffn/relu"], flags={"ACT_DGRAD_CORE": True})
family("act_dgrad_core/legacy", ["ffn/gelu"], flags=dict(LEGACY, ACT_DGRAD_CORE=True))
family("ffn_fuse_off", ["ffn/gelu", "ffn/relu"], flags={"FFN_FUSE": False})
family("ffn_fuse_off/legacy", ["ffn/gelu"], flags=dict(LEGACY, FFN_FUSE=False))
DET = {"N._DETERMINISTIC": True}
family("deterministic", ["dense/none", "dense/gelu", "multi/none", "multi/gelu", "trans"], flags=DET)
family("deterministic/t2048", ["dense/none", "multi/gelu"], flags=DET, T=T2)
family("deterministic/nobias", ["dense/none", "multi/gelu"], flags=DET, bias=False)
NOFUSE = {"FUSED_BIAS_GRAD": False}
family("fused_bias_grad_off", ["dense/none", "dense/gelu", "multi/none", "multi/gelu"], flags=NOFUSE)
family("fused_bias_grad_off/t2048", ["dense/none", "dense/gelu", "multi/none", "multi/gelu", "ffn/gelu"], flags=NOFUSE,
       T=T2)
scenario("fused_bias_grad_off/t2048/mixed_slots/multi", flags=NOFUSE, entry="multi", nseg=3, T=T2,
         bslot=(True, False, True))
family("hand_wgrad_off/t2048", ["dense/none", "multi/gelu"], flags={"HAND_WGRAD": False}, T=T2)
family("store_first_off", ["dense/none", "dense/gelu", "multi/gelu", "trans"], flags={"V.STORE_FIRST": False})
family("wgrad_stream", ["dense/none", "dense/gelu"], flags={"DENSE_WGRAD_STREAM": True}, wslot=False, bslot=False)
family("wgrad_stream/wslot_only", ["dense/none"], flags={"DENSE_WGRAD_STREAM": True}, bslot=False)
family("act_sinks_off", ["dense/none"], flags={"actsink.ENABLED": False}, sink="first")
scenario("weight_cats/active", cats_case)
scenario("weight_cats/inactive", cats_case, active=False)

# ---- a kernel declines ("shape not taken"), one at a time, where it would otherwise run --------------------
family("decline/gemm_pp", ["dense/gelu", "multi/gelu", "ffn/gelu"], decline=["mdtf_gemm_pp"])
family("decline/gemm_pp/pp_fwd=all", ["dense/none", "trans", "ffn/gelu"], decline=["mdtf_gemm_pp"],
       flags={"PP_FWD": "all"})
family("decline/gemm_pp/pp_dgrad=all", ["dense/gelu"], decline=["mdtf_gemm_pp"], flags={"PP_DGRAD": "all"})
for _sink in ("first", "acc"):
    family("decline/gemm_pp/pp_dgrad=all/sink_" + _sink, ["dense/gelu", "multi/gelu"], decline=["mdtf_gemm_pp"],
           flags={"PP_DGRAD": "all"}, sink=_sink)
family("decline/gemm_pp/pp_wgrad=all", ["dense/gelu", "multi/gelu"], decline=["mdtf_gemm_pp"],
       flags={"PP_WGRAD": "all"})
family("decline/gemm_pp/pp_wgrad=all/pp_fwd=all", ["trans"], decline=["mdtf_gemm_pp"],
       flags={"PP_WGRAD": "all", "PP_FWD": "all"})
family("decline/gemm_pp/act_dgrad_core", ["ffn/gelu"], decline=["mdtf_gemm_pp"], flags={"ACT_DGRAD_CORE": True})
family("decline/gemm_wg", ["dense/none", "dense/gelu", "multi/none", "multi/gelu"], decline=["mdtf_gemm_wg"])
family("decline/gemm_wg/store_first_off", ["dense/none", "dense/gelu"], decline=["mdtf_gemm_wg"],
       flags={"V.STORE_FIRST": False})
family("decline/gemm_wg/nobias", ["dense/none"], decline=["mdtf_gemm_wg"], bias=False)
family("decline/gemm_fwd/legacy/fwd=mdtf", ["dense/gelu", "multi/none"], decline=["mdtf_gemm_fwd"],
       flags=dict(LEGACY, FWD_MODE="mdtf"))
family("decline/gemm_dgrad_act", ["ffn/gelu", "ffn/relu"], decline=["mdtf_gemm_dgrad_act"])
family("decline/gemm_dgrad_act/legacy", ["ffn/gelu"], decline=["mdtf_gemm_dgrad_act"], flags=LEGACY)
family("decline/gemm_wgrad/t2048", ["dense/none", "dense/gelu", "multi/none", "multi/gelu"],
       decline=["mdtf_gemm_wgrad"], T=T2)
family("decline/gemm_wgrad+gemm_wg", ["dense/none", "multi/gelu"], decline=["mdtf_gemm_wgrad", "mdtf_gemm_wg"])
family("decline/conv_dgrad_v2/hand_dgrad", ["dense/none"], decline=["mdtf_conv_dgrad_v2"], flags=HAND_HIT,
       raises=True)


def run_scenario(name):
    fn, setup, kwargs = SCENARIOS[name]
    with pytest.MonkeyPatch.context() as mp:
        s = Scenario(mp, **setup)
        fn(s, **kwargs)
        return json.loads(json.dumps(s.result()))


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_dispatch_trace(name, expected):
    assert run_scenario(name) == expected["scenarios"][name]


def test_fixture_has_no_stale_scenarios(expected):
    assert sorted(expected["scenarios"]) == sorted(SCENARIOS)


def regen():
    body = ",\n".join("%s: %s" % (json.dumps(n), json.dumps(run_scenario(n), separators=(",", ":"), sort_keys=True))
                      for n in sorted(SCENARIOS))
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write("{\n\"scenarios\": {\n" + body + "\n}\n}\n")
    print("wrote %s: %d scenarios, %d bytes" % (FIXTURE, len(SCENARIOS), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    if "--regen" in sys.argv:
        regen()
    else:
        sys.exit("usage: python tests/test_dense_dispatch.py --regen")
