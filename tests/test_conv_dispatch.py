"""Conv dispatch pinned launch for launch, on the CPU.

``mdtf.ops.conv`` runs on CPU tensors when ``N.fn`` is a recorder: every native launch a forward / backward of
the conv autograd function would issue is recorded as ``[kernel, arg, ...]`` with integers by value and
pointers by the name of the scenario tensor they alias (``null`` / ``ptr`` otherwise).  The expected traces in
``tests/fixtures/conv_dispatch_trace.json`` were recorded with this module before the dispatch was
restructured; the tests assert exact equality, so the Python wiring between ``choose()`` and the kernels
cannot change unnoticed.

Regenerate (only when dispatch behaviour is meant to change)::

    python tests/test_conv_dispatch.py --regen
"""
import ctypes
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mdtf.ops import _native as N  # noqa: E402
from mdtf.ops import actsink  # noqa: E402
from mdtf.ops import bn  # noqa: E402
from mdtf.ops import conv as C  # noqa: E402
from mdtf.train import variables as V  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "conv_dispatch_trace.json")
BF16 = torch.bfloat16


class Recorder(object):
    """The fake native layer: ``fn(name)`` returns a callable that records its arguments and returns 0."""

    def __init__(self):
        self.calls = []
        self.named = []          # (name, tensor): kept alive, so no later allocation can take their address

    def name(self, name, t, since=None):
        """Name ``t``; ``since``: also in the calls recorded from that index on, which saw it as an unknown
        pointer (a buffer the launch under test allocated itself)."""
        self.named.append((name, t))
        for call in self.calls[since:] if since is not None else ():
            for i, a in enumerate(call):
                if isinstance(a, tuple) and self._resolve(a[1]) is not None:
                    call[i] = self._resolve(a[1])
        return t

    def _resolve(self, addr):
        for name, t in self.named:
            base = t.data_ptr()
            if t.numel() and base <= addr < base + t.numel() * t.element_size():
                return name if addr == base else "%s+%d" % (name, addr - base)
        return None

    def _arg(self, a):
        if a is None:
            return "null"
        if isinstance(a, (ctypes.c_int, ctypes.c_longlong)):
            return a.value
        if isinstance(a, int):
            return int(a)
        if isinstance(a, ctypes.c_void_p):
            if not a.value:
                return "null"
            return self._resolve(a.value) or ("?", a.value)      # unknown: named later (name(since=)) or "ptr"
        return "ptr"

    def fn(self, name):
        def call(*args):
            self.calls.append([name] + [self._arg(a) for a in args])
            return 0
        return call

    def note(self, *what):
        self.calls.append(list(what))

    def finish(self):
        for call in self.calls:
            for i, a in enumerate(call):
                if isinstance(a, tuple):
                    call[i] = "ptr"
        return self.calls


class Scenario(object):
    """One scenario's state: the recorder, the patches, the named tensors and a few drivers."""

    def __init__(self, mp):
        self.mp = mp
        self.rec = Recorder()
        self.out = {}
        mp.setattr(N, "fn", self.rec.fn)
        mp.setattr(N, "stream_ptr", lambda device=None: ctypes.c_void_p(0))
        mp.setattr(C, "_STATS", {})
        mp.setattr(C, "_BSTATS", {})
        mp.setattr(V, "GRAD_EPOCH", [1])
        # the flags the environment sets at import, at their shipped defaults
        for mod, flags in ((C, dict(_SLAB_MODE="dense", WGRAD_SLAB=False, DENSE_WGRAD_SLAB=True, WGRAD_INK=False,
                                    WGRAD_STREAM=False, SLAB_SIDE=False, BWD_STATS=True, CONV_ROWS=True,
                                    DUAL_DGRAD=True, DUAL_TILE=(2, 8, 1), STEM="mdtf", STEM_KERNEL="rows",
                                    _STEM_PACK_W=True, STEM_WG_BLOCKS=768, MAX_STAT_SLOTS=128, _TABLE=None,
                                    TABLE_PATH=os.path.join(ROOT, "mdtf", "ops", "conv_table.json"))),
                           (V, dict(STORE_FIRST=True)), (N, dict(_DETERMINISTIC=False)),
                           (actsink, dict(ENABLED=True))):
            for flag, value in flags.items():
                mp.setattr(mod, flag, value)
        mp.delenv("MDTF_CONV", raising=False)
        mp.delenv("MDTF_WINOGRAD", raising=False)
        mp.delenv("TF_ENABLE_WINOGRAD_NONFUSED", raising=False)
        real_claim, real_note = V.claim_store, V.note_accumulate

        def claim(var):
            r = real_claim(var)
            self.rec.note("V.claim_store", bool(r))
            return r

        def note(var):
            self.rec.note("V.note_accumulate")
            return real_note(var)
        mp.setattr(V, "claim_store", claim)
        mp.setattr(V, "note_accumulate", note)
        real_slab, real_acquire = C.wgrad_slab, C.bwd_stats_acquire

        def slab(*a, **k):
            t, cap = real_slab(*a, **k)
            if t is not None:
                self.rec.name("slab", t)
            return t, cap

        def acquire(*a, **k):
            return self.rec.name("bstats", real_acquire(*a, **k))
        mp.setattr(C, "wgrad_slab", slab)
        mp.setattr(C, "bwd_stats_acquire", acquire)
        self.counters = (C.DUAL_FUSED[0], actsink.FOLDED[0], bn.ON_CONSUMER_USED[0])

    def t(self, name, shape, dtype=BF16, grad=False):
        t = torch.zeros(tuple(shape), dtype=dtype)
        if grad:
            t.requires_grad_(True)
        return self.rec.name(name, t)

    def deterministic(self, flag=True):
        self.mp.setattr(N, "_DETERMINISTIC", N.deterministic())      # restored with the other patches
        N.set_deterministic(flag)

    def table(self, entries):
        """A conv table of its own; keys are written for the tuned batch (the batch-agnostic lookup)."""
        self.mp.setattr(C, "_TABLE", dict(entries))

    def forward(self, x, w, stride, pads, dil, want):
        if want is None:
            return C.conv2d_nhwc(x, w, stride, pads, dil)
        since = len(self.rec.calls)
        y, st = C.conv2d_stats_nhwc(x, w, stride, pads, dil, private=(want == "private"))
        self.rec.note("stats", None if st is None else st[2])
        if st is not None:       # allocated by this forward before any of its temporaries was freed
            self.rec.name("stats_sum", st[0], since)
            self.rec.name("stats_sq", st[1], since)
        return y

    def backward(self, y, inputs, tag="grads"):
        self.rec.note("--backward")
        dy = self.t("dy" if tag == "grads" else "dy2", y.shape)
        inputs = [t for t in inputs if t.requires_grad]
        grads = torch.autograd.grad([y], inputs, [dy], allow_unused=True) if inputs else ()
        self.out[tag] = [g is None for g in grads]

    def sink_state(self, xs):
        self.out["sink"] = [xs.count, xs.buf is not None, xs.stats is not None, xs.early is not None,
                            xs.pend is None, xs.pconv is None]

    def result(self):
        self.out["calls"] = self.rec.finish()
        now = (C.DUAL_FUSED[0], actsink.FOLDED[0], bn.ON_CONSUMER_USED[0])
        self.out["counters"] = [b - a for a, b in zip(self.counters, now)]
        return self.out


def prepare_sink(s, xs, x, others=0, pre=None, req=0):
    """Put the activation-gradient sink of ``x`` into the state a contributor finds: ``others`` further
    registered consumers, an earlier contribution (``buf``: written, ``masked``: pending), and the producing
    BatchNorm's statistics request of length ``req``."""
    for _ in range(others):
        xs.register()
    if pre == "buf":
        xs.adopt_or_add(s.t("sink_buf", x.shape))
    elif pre == "masked":
        xs.defer_masked(s.t("pend_g", x.shape), s.t("pend_mask", x.shape, torch.uint8))
    if req:
        cx = x.shape[3]
        request = [s.t("bn_x", x.shape), s.t("bn_mask", x.shape, torch.uint8)]
        if req == 3:
            request.append(lambda sbuf: ("early", sbuf))
        if req == 4:
            request += [None, (s.t("bn_g", (cx,), torch.float32), s.t("bn_mean", (cx,), torch.float32),
                               s.t("bn_invstd", (cx,), torch.float32), x.numel() // cx, cx)]
        xs.stat_req = tuple(request)


def conv_case(s, xs_, ws_, stride=1, pad=0, want=None, sink=None, wsink=False, pend=False, dx=True, dw=True,
              before_backward=None):
    """Forward and backward of one conv; ``sink``: keyword arguments of :func:`prepare_sink`."""
    stride, pads, dil = (stride, stride), (pad,) * 4, (1, 1)
    x = s.t("x", xs_, grad=dx)
    w = s.t("w", ws_, grad=dw)
    if wsink:
        w._mdtf_var = types.SimpleNamespace(grad=s.t("w_grad", ws_, torch.float32))
    xs = actsink.attach(x) if sink is not None else None
    if pend:
        ent = (x, s.t("pend_x", xs_), s.t("pend_ss", (2 * xs_[3],), torch.float32),
               s.t("pend_mask", xs_, torch.uint8))
        s.mp.setattr(bn, "take_pending", lambda y: ent if y is x else None)
    y = s.forward(x, w, stride, pads, dil, want)
    if xs is not None:
        prepare_sink(s, xs, x, **sink)
    if before_backward is not None:
        before_backward(s)
    s.backward(y, [x, w])
    if xs is not None:
        s.sink_state(xs)


def projection_case(s, c1, req=0, pp=False, dual=True):
    """A block input feeding a strided 1x1 projection and a 1x1 / stride-1 conv with ``c1`` outputs: the
    projection's backward runs first (deferred), then the other conv's (fused when ``dual_ok``, else the
    deferred closure runs).  ``pp``: the projection's data gradient is a ping-pong choice; ``pp_ok`` does not
    take a strided data gradient, so that branch is reached only with the predicate replaced."""
    s.mp.setattr(C, "DUAL_DGRAD", dual)
    xshape, pshape, bshape = (2, 56, 56, 256), (1, 1, 256, 512), (1, 1, 256, c1)
    if pp:
        s.table({"dgrad:256,56,56,256:1,1,512:2,2:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 3}})
        s.mp.setattr(C, "pp_ok", lambda *a, **k: True)
    x = s.t("x", xshape, grad=True)
    xs = actsink.attach(x)
    w2 = s.t("w2", pshape, grad=True)
    w = s.t("w", bshape, grad=True)
    y2 = s.forward(x, w2, (2, 2), (0, 0, 0, 0), (1, 1), None)
    y = s.forward(x, w, (1, 1), (0, 0, 0, 0), (1, 1), None)
    prepare_sink(s, xs, x, req=req)
    s.backward(y2, [x, w2], tag="grads2")
    s.out["sink_deferred"] = [xs.count, xs.pconv is None]
    s.backward(y, [x, w])
    s.sink_state(xs)


def stem_case(s, want=None, packed=True, wsink=False, deterministic_bwd=False):
    if not packed:
        s.mp.setattr(C, "STEM", "miopen")        # the forward leaves no packed image ...

    def before_backward(s):
        if not packed:
            s.mp.setattr(C, "STEM", "mdtf")      # ... for the stem weight gradient chosen in the backward
        if deterministic_bwd:
            s.deterministic()
    conv_case(s, (2, 64, 64, 3), (7, 7, 3, 64), stride=2, pad=3, want=want, dx=False, wsink=wsink,
              before_backward=before_backward)


def convt_case(s, forced=None):
    if forced:
        s.mp.setenv("MDTF_CONV", forced)
    x = s.t("x", (2, 8, 8, 64), grad=True)
    w = s.t("w", (3, 3, 64, 64), grad=True)
    y = C.conv2d_dgrad_nhwc(x, w, (2, 16, 16, 64), (2, 2), (1, 1, 1, 1))
    s.backward(y, [x, w])


# the geometries (ResNet-50 layers at batch 2; the batch-agnostic lookup gives them the shipped table's choices)
V1 = dict(xs_=(4, 8, 8, 16), ws_=(3, 3, 16, 24), pad=1)                 # C % 64 != 0: v1 kernels
V2 = dict(xs_=(2, 28, 28, 128), ws_=(3, 3, 128, 128), pad=1)            # fwd v2, dgrad v2, wgrad v3 (slab 1)
V3 = dict(xs_=(2, 14, 14, 256), ws_=(3, 3, 256, 256), pad=1)            # fwd v3 (stages 32), dgrad v3
WS = dict(xs_=(2, 56, 56, 64), ws_=(1, 1, 64, 64))                      # ws streamed, dgrad tile tp = 4
WS_BNA = dict(xs_=(2, 56, 56, 64), ws_=(1, 1, 64, 256))                 # ws streamed, bna_ok; wgrad slab 0
WS_ROWS = dict(xs_=(2, 56, 56, 64), ws_=(3, 3, 64, 64), pad=1)          # ws row-staged
PP = dict(xs_=(2, 56, 56, 256), ws_=(1, 1, 256, 128))                   # with PP_TABLE: ping-pong fwd and dgrad
STRIDED = dict(xs_=(2, 56, 56, 256), ws_=(1, 1, 256, 512), stride=2)    # the stage-2 projection
PP_TABLE = {
    "fwd:256,56,56,256:1,1,128:1,1:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 3},
    "dgrad:256,56,56,256:1,1,128:1,1:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 1},
}
# ping-pong entries whose shape pp_ok refuses (Cin 64 is no multiple of tile 0's 256 columns; 192 gathered
# channels are no power of two): the previous entry, or the defaults
PP_PREV_TABLE = {
    "dgrad:256,56,56,64:1,1,64:1,1:0,0,0,0:1,1": {
        "backend": "mdtf", "ver": 5, "tile": 0,
        "prev": {"backend": "mdtf", "bm": 128, "bn": 64, "splits": 0, "ver": 2, "stages": 3}},
    "fwd:256,56,56,64:1,1,64:1,1:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 0},     # fwd takes it
}
PP_NOPREV_TABLE = {
    "dgrad:256,56,56,64:1,1,64:1,1:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 0},
    "fwd:256,28,28,192:1,1,64:1,1:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 3},
    "dgrad:256,28,28,192:1,1,64:1,1:0,0,0,0:1,1": {"backend": "mdtf", "ver": 5, "tile": 3,
                                                  "prev": {"backend": "miopen"}},
}
MIOPEN_TABLE = {k % "256,28,28,128:3,3,128:1,1:1,1,1,1:1,1": {"backend": "miopen"}
                for k in ("fwd:%s", "dgrad:%s", "wgrad:%s")}

SCENARIOS = {}


def scenario(name, fn, *args, **kwargs):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = lambda s: fn(s, *args, **kwargs)


def _with(setup, fn, **kwargs):
    def run(s):
        setup(s)
        fn(s, **kwargs)
    return run


# ---- every backend: forward, backward without a sink, statistics False / True / 2 -------------------------
for _name, _geo_, _setup in (
        ("v1", V1, None), ("v2", V2, None), ("v3", V3, None), ("ws", WS, None), ("ws_bna_shape", WS_BNA, None),
        ("ws_rows", WS_ROWS, None), ("ws_rows_off", WS_ROWS, lambda s: s.mp.setattr(C, "CONV_ROWS", False)),
        ("strided", STRIDED, None),
        ("pp", PP, lambda s: s.table(PP_TABLE)),
        ("pp_prev", WS, lambda s: s.table(PP_PREV_TABLE)),
        ("pp_noprev", WS, lambda s: s.table(PP_NOPREV_TABLE)),
        ("pp_prev_lib", dict(xs_=(2, 28, 28, 192), ws_=(1, 1, 192, 64)), lambda s: s.table(PP_NOPREV_TABLE)),
        ("winograd", dict(xs_=(2, 8, 8, 64), ws_=(3, 3, 64, 64), pad=1),
         lambda s: s.mp.setenv("MDTF_WINOGRAD", "1")),
        ("miopen_env", V2, lambda s: s.mp.setenv("MDTF_CONV", "miopen")),
        ("miopen_table", V2, lambda s: s.table(MIOPEN_TABLE)),
        ("miopen_channels", dict(xs_=(2, 8, 8, 12), ws_=(3, 3, 12, 20), pad=1), None),
        ("mdtf_env", V2, lambda s: s.mp.setenv("MDTF_CONV", "mdtf")),
        ("mdtf2_env", V2, lambda s: s.mp.setenv("MDTF_CONV", "mdtf2")),
        ("det_ws", WS, lambda s: s.deterministic()),               # ver-4 entry in deterministic mode: v2
        ("det_v3", V3, lambda s: s.deterministic()),
        ("det_v1", V1, lambda s: s.deterministic())):
    for _want in (None, "shared", "private"):
        for _wsink in (False, True):
            if _wsink and _want is not None:
                continue
            _n = "plain/%s/%s%s" % (_name, _want or "nostats", "/wsink" if _wsink else "")
            _kw = dict(_geo_, want=_want, wsink=_wsink)
            scenario(_n, _with(_setup, conv_case, **_kw) if _setup else conv_case, **({} if _setup else _kw))

scenario("plain/v2/dx_only", conv_case, dw=False, **V2)
scenario("plain/v2/dw_only", conv_case, dx=False, wsink=True, **V2)
scenario("plain/v2/no_grads", conv_case, dx=False, dw=False, **V2)

# ---- a pending BatchNorm apply on the operand ---------------------------------------------------------------
scenario("pend/bna", conv_case, pend=True, want="shared", **WS_BNA)
scenario("pend/bna_private", conv_case, pend=True, want="private", **WS_BNA)
scenario("pend/no_stats", conv_case, pend=True, **WS_BNA)                       # not want_stats: applied
scenario("pend/not_bna_shape", conv_case, pend=True, want="shared", **WS_ROWS)  # 3x3: applied
scenario("pend/not_ws", conv_case, pend=True, want="shared", **V2)

# ---- the stem -------------------------------------------------------------------------------------------------
for _want in (None, "shared", "private"):
    scenario("stem/%s" % (_want or "nostats"), stem_case, want=_want)
scenario("stem/wsink", stem_case, wsink=True)
scenario("stem/no_packed_image", stem_case, packed=False)
scenario("stem/no_packed_image/wsink", stem_case, packed=False, wsink=True)
scenario("stem/deterministic_backward", stem_case, deterministic_bwd=True)
scenario("stem/deterministic", _with(lambda s: s.deterministic(), stem_case, want="shared"))

# ---- backward into an activation-gradient sink -----------------------------------------------------------
SINK_STATES = {
    "first": dict(others=1),
    "accumulate": dict(others=2, pre="buf"),
    "folded": dict(others=2, pre="masked"),
    "complete": dict(req=2),
    "complete_accumulate": dict(others=1, pre="buf", req=2),
    "complete_folded": dict(others=1, pre="masked", req=2),
    "complete_early": dict(req=3),
    "complete_wgrad_fin": dict(req=4),
    "request_not_completing": dict(others=1, req=2),
}
for _name, _geo_, _setup in (
        ("ws", WS, None), ("ws_rows", WS_ROWS, None), ("pp", PP, lambda s: s.table(PP_TABLE)), ("v2", V2, None),
        ("v3", V3, None), ("det_ws", WS, lambda s: s.deterministic()),
        ("det_pp", PP, lambda s: (s.table(PP_TABLE), s.deterministic())),
        ("det_v2", V2, lambda s: s.deterministic())):
    for _state, _sink in SINK_STATES.items():
        _kw = dict(_geo_, sink=_sink, wsink=True)
        scenario("sink/%s/%s" % (_name, _state),
                 _with(_setup, conv_case, **_kw) if _setup else conv_case, **({} if _setup else _kw))
        if _state.startswith("complete") and not _name.startswith("det"):
            scenario("sink/%s/%s/bwd_stats_off" % (_name, _state),
                     _with(lambda s, _setup=_setup: (_setup and _setup(s), s.mp.setattr(C, "BWD_STATS", False)),
                           conv_case, **_kw))
scenario("sink/v2/complete_wgrad_fin/no_wsink", conv_case, sink=dict(req=4), **V2)
scenario("sink/v2/complete/dx_only", conv_case, sink=dict(req=2), dw=False, **V2)
for _state in ("first", "accumulate", "folded", "complete"):
    scenario("sink/v1/%s" % _state, conv_case, sink=SINK_STATES[_state], **V1)          # adopt_or_add
    scenario("sink/miopen/%s" % _state, _with(lambda s: s.mp.setenv("MDTF_CONV", "miopen"), conv_case,
                                              sink=SINK_STATES[_state], **V2))
    scenario("sink/winograd/%s" % _state, _with(lambda s: s.mp.setenv("MDTF_WINOGRAD", "1"), conv_case,
                                                sink=SINK_STATES[_state], **V2))

# ---- the strided projection: deferred, fused, or run by its closure ----------------------------------------
scenario("proj/first_deferred", conv_case, sink=dict(others=1), **STRIDED)
scenario("proj/first_completing", conv_case, sink=dict(), **STRIDED)                 # completing: not deferred
scenario("proj/not_first", conv_case, sink=dict(others=2, pre="buf"), **STRIDED)
scenario("proj/dual_off", _with(lambda s: s.mp.setattr(C, "DUAL_DGRAD", False), conv_case, sink=dict(others=1),
                                **STRIDED))
scenario("proj/v1_not_deferred", _with(lambda s: s.mp.setenv("MDTF_CONV", "mdtf"), conv_case,
                                       sink=dict(others=1), **STRIDED))
for _req in (0, 2, 3, 4):
    scenario("proj/dual/req%d" % _req, projection_case, 128, req=_req)
    scenario("proj/closure_v2/req%d" % _req, projection_case, 64, req=_req)
    scenario("proj/closure_pp/req%d" % _req, projection_case, 64, req=_req, pp=True)
scenario("proj/dual_pp", projection_case, 128, req=2, pp=True)
scenario("proj/dual/deterministic", _with(lambda s: s.deterministic(), projection_case, c1=128, req=2))
scenario("proj/dual/bwd_stats_off", _with(lambda s: s.mp.setattr(C, "BWD_STATS", False), projection_case, c1=128,
                                          req=2))
scenario("proj/dual_disabled", projection_case, 128, req=2, dual=False)

# ---- weight-gradient slabs: the three MDTF_WGRAD_SLAB modes x the table's "slab" field both ways ----------
for _mode, _on in (("dense", False), ("1", True), ("0", False)):
    for _name, _geo_ in (("table_slab1", V2), ("table_slab0", WS_BNA), ("table_silent", STRIDED), ("v1", V1)):
        for _wsink in (False, True):
            scenario("slab/%s/%s%s" % (_mode, _name, "/wsink" if _wsink else ""),
                     _with(lambda s, _mode=_mode, _on=_on: (s.mp.setattr(C, "_SLAB_MODE", _mode),
                                                            s.mp.setattr(C, "WGRAD_SLAB", _on)),
                           conv_case, dx=False, wsink=_wsink, **_geo_))
scenario("slab/deterministic", _with(lambda s: s.deterministic(), conv_case, dx=False, wsink=True, **V2))
scenario("slab/second_writer", _with(
    lambda s: s.mp.setattr(V, "claim_store", lambda var: (s.rec.note("V.claim_store", False), False)[1]),
    conv_case, dx=False, wsink=True, **V2))

# ---- conv2d_transpose ------------------------------------------------------------------------------------------
scenario("convt/mdtf", convt_case)
scenario("convt/v1", convt_case, forced="mdtf")
scenario("convt/library", convt_case, forced="miopen")


def run_scenario(name):
    with pytest.MonkeyPatch.context() as mp:
        s = Scenario(mp)
        SCENARIOS[name](s)
        return json.loads(json.dumps(s.result()))


def choose_all():
    """``choose()`` for every key of the shipped table under each ``MDTF_CONV`` and both deterministic modes."""
    with open(os.path.join(ROOT, "mdtf", "ops", "conv_table.json")) as f:
        keys = sorted(json.load(f))
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(C, "_TABLE", None)
        mp.setattr(C, "TABLE_PATH", os.path.join(ROOT, "mdtf", "ops", "conv_table.json"))
        mp.setattr(N, "_DETERMINISTIC", N.deterministic())
        mp.delenv("MDTF_WINOGRAD", raising=False)
        mp.delenv("TF_ENABLE_WINOGRAD_NONFUSED", raising=False)
        for forced in ("auto", "mdtf", "mdtf2", "miopen"):
            mp.setenv("MDTF_CONV", forced)
            for det in (False, True):
                N.set_deterministic(det)
                for key in keys:
                    pass_, xs_, ws_, st, pads, dil = key.split(":")
                    n, h, w, c = (int(v) for v in xs_.split(","))
                    kh, kw, co = (int(v) for v in ws_.split(","))
                    ch = C.choose(pass_, (n, h, w, c), (kh, kw, c, co), tuple(int(v) for v in st.split(",")),
                                  tuple(int(v) for v in pads.split(",")), tuple(int(v) for v in dil.split(",")))
                    out["%s|det%d|%s" % (forced, det, key)] = json.loads(json.dumps(ch))
    return out


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def expected():
    return _fixture()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_dispatch_trace(name, expected):
    assert run_scenario(name) == expected["scenarios"][name]


def test_fixture_has_no_stale_scenarios(expected):
    assert sorted(expected["scenarios"]) == sorted(SCENARIOS)


def test_choose_shipped_table(expected):
    got = choose_all()
    assert sorted(got) == sorted(expected["choose"])
    wrong = {k: (v, expected["choose"][k]) for k, v in got.items() if v != expected["choose"][k]}
    assert not wrong, wrong


def regen():
    lines = []
    for section, items in (("scenarios", {n: run_scenario(n) for n in sorted(SCENARIOS)}), ("choose", choose_all())):
        body = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                          for k, v in sorted(items.items()))
        lines.append("%s: {\n%s\n}" % (json.dumps(section), body))
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print("wrote %s: %d scenarios, %d choices, %d bytes" % (FIXTURE, len(SCENARIOS), len(choose_all()),
                                                          os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    if "--regen" in sys.argv:
        regen()
    else:
        sys.exit("usage: python tests/test_conv_dispatch.py --regen")
