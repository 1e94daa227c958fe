"""The fused optimizer updates (``mdtf.ops.optim`` / ``csrc/optim.hip``: sgd, momentum, Adam and the batched
``apply_multi_``) against an independent fp64 reference, element by element.

Every test takes a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.optim`` (the bound of
``optim_helpers`` must hold for it too: that is what validates the scale and the rounding counts), ``cuda`` the HIP
kernels.  Tensors are slices [4 : 4 + n] of sentinel-filled buffers; after every call the sentinels and the whole
gradient buffer must be bitwise unchanged, and the bf16 shadow bitwise ``w.bfloat16()``.
"""
import os
import subprocess
import sys

import pytest
import torch

from mdtf.ops import optim as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_helpers as OH  # noqa: E402
import optim_variant_child as VC  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]

# 4: one float4, one thread | 64: one wave of float4s is not filled | 4*511, 4*512, 4*513: Adam's chunk of
# 2 x 256 float4s per block short by one float4 (the ``i < n4`` guard of the second half), exactly full, and one
# float4 into a second block (its first guard passes for one thread, ``break`` for the second half) |
# 4*(2*512 + 257): two full Adam chunks and a third whose second half has one float4; 6 blocks (the last ragged) for
# the grid-stride kernels | 4*(2048*256 + 37): the smallest size class at which sgd, momentum and apply_multi (2048
# blocks at most) take a second trip of the grid-stride loop, for 37 threads only; 1025 Adam chunks
SIZES = [4, 64, 4 * 511, 4 * 512, 4 * 513, 4 * (2 * 512 + 257), 4 * (2048 * 256 + 37)]
N = 4 * (2 * 512 + 257)           # the size of the hyper-parameter grids
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=3, gs=0.5, wd=1e-2, decoupled=True, bias_correction=True)
MOMENTUM = dict(lr=0.1, mom=0.9, gs=0.5, wd=1e-2, nesterov=False)
SGD = dict(lr=0.1, gs=0.5, wd=1e-2)
HP = {"sgd": SGD, "momentum": MOMENTUM, "adam": ADAM}


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from mdtf.ops import _native
        _native.lib()
        assert _native.mode() != "torch"
    return device


def _k_single(kind, hp):
    if kind == "sgd":
        return OH.K_SGD
    if kind == "momentum":
        return OH.K_NESTEROV if hp["nesterov"] else OH.K_MOMENTUM
    return OH.K_ADAM


class Bufs(object):
    """The guarded device buffers of one parameter group."""

    def __init__(self, kind, device, inp, shadow=True):
        n = inp["w"].numel()
        self.kind, self.n = kind, n
        self.w = OH.Guarded(inp["w"], device)
        self.g = [OH.Guarded(g, device) for g in inp["g"]]
        self.s1 = OH.Guarded(inp["acc" if kind == "momentum" else "m"], device) if kind != "sgd" else None
        self.s2 = OH.Guarded(inp["v"], device) if kind == "adam" else None
        self.shadow = OH.Guarded(None, device, torch.bfloat16, n) if shadow else None

    def t(self, x):
        return x.t if x is not None else None

    def state_names(self):
        return {"sgd": [], "momentum": [("acc", self.s1)], "adam": [("m", self.s1), ("v", self.s2)]}[self.kind]

    def assert_contained(self, what):
        for name, b in [("w", self.w), ("s1", self.s1), ("s2", self.s2), ("shadow", self.shadow)]:
            assert b is None or b.guards_intact(), "%s: wrote outside %s[0:n]" % (what, name)
        for i, g in enumerate(self.g):
            assert g.unchanged(), "%s: gradient %d modified" % (what, i)

    def outputs(self):
        out = {"w": self.w.t.clone()}
        for name, b in self.state_names():
            out[name] = b.t.clone()
        if self.shadow is not None:
            out["shadow"] = self.shadow.t.clone()
        return out


def _call(b, g, hp, dyn=None):
    w, s1, s2, sh = b.w.t, b.t(b.s1), b.t(b.s2), b.t(b.shadow)
    if b.kind == "sgd":
        O.sgd_(w, g, sh, hp["lr"], hp["gs"], hp["wd"], dyn=dyn)
    elif b.kind == "momentum":
        O.momentum_(w, g, s1, sh, hp["lr"], hp["mom"], hp["gs"], hp["wd"], hp["nesterov"], dyn=dyn)
    else:
        O.adam_(w, g, s1, s2, sh, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["step"], hp["gs"], hp["wd"],
                hp["decoupled"], hp["bias_correction"], dyn=dyn)


def _ref_start(kind, inp):
    if kind == "sgd":
        return OH.start(w=inp["w"])
    if kind == "momentum":
        return OH.start(w=inp["w"], acc=inp["acc"])
    return OH.start(w=inp["w"], m=inp["m"], v=inp["v"])


def _ref_step(kind, st, g, hp, lr=None, lr_t=None):
    lr = hp["lr"] if lr is None else lr
    if kind == "sgd":
        OH.sgd_step(st, g, lr, hp["gs"], hp["wd"])
    elif kind == "momentum":
        OH.momentum_step(st, g, lr, hp["mom"], hp["gs"], hp["wd"], hp["nesterov"])
    else:
        if lr_t is None:
            lr_t = OH.adam_lr_t(lr, hp["b1"], hp["b2"], hp["step"], hp["bias_correction"])
        OH.adam_step(st, g, lr, lr_t, hp["b1"], hp["b2"], hp["eps"], hp["gs"], hp["wd"], hp["decoupled"])


def _compare(b, st, ks, what):
    """w and every state buffer against fp64; the shadow bitwise against round-to-nearest-even of the fp32 w."""
    b.assert_contained(what)
    OH.check(b.w.t, st, "w", ks["w"], what)
    for name, buf in b.state_names():
        OH.check(buf.t, st, name, ks[name], what)
    if b.shadow is not None:
        # a NaN stays a NaN (its payload is not part of the rounding); everything else, infinities included, bitwise
        nan = torch.isnan(b.w.t)
        assert torch.equal(torch.isnan(b.shadow.t), nan), "%s: shadow NaN positions" % what
        assert OH.bits_equal(b.shadow.t.masked_fill(nan, 0), b.w.t.masked_fill(nan, 0).bfloat16()), \
            "%s: shadow != bf16(w)" % what


def _one_update(kind, device, n, hp, seed, zero_state=False):
    device = _device(device)
    inp = OH.make_inputs(n, seed, zero_state=zero_state)
    b = Bufs(kind, device, inp)
    _call(b, b.g[0].t, hp)
    st = _ref_start(kind, inp)
    _ref_step(kind, st, inp["g"][0], hp)
    _compare(b, st, _k_single(kind, hp), "%s/%s n=%d" % (device, kind, n))
    return b, inp


# ------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
@pytest.mark.parametrize("device", DEVICES)
def test_every_size(device, kind, n):
    hp = dict(HP[kind], nesterov=True) if kind == "momentum" else HP[kind]
    b, inp = _one_update(kind, device, n, hp, seed=n % 1000 + 1)
    assert not torch.equal(b.w.t.cpu(), inp["w"])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["momentum", "adam"])
@pytest.mark.parametrize("device", DEVICES)
def test_apply_multi_every_size(device, kind, n):
    _apply_multi(device, kind, 3, torch.bfloat16, True, n)


# -------------------------------------------------------------------------------------------- hyper-parameters
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("device", DEVICES)
def test_sgd_grid(device, wd, gs):
    _one_update("sgd", device, N, dict(SGD, wd=wd, gs=gs), seed=21)


@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("device", DEVICES)
def test_momentum_grid(device, nesterov, wd, mom):
    _one_update("momentum", device, N, dict(MOMENTUM, nesterov=nesterov, wd=wd, mom=mom), seed=22)


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("step", [1, 3, 100000])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("device", DEVICES)
def test_adam_grid(device, decoupled, wd, step, bias_correction):
    for eps in (1e-8, 1e-6):                           # TF's default | BERT's
        for gs in (1.0, 0.5):
            hp = dict(ADAM, decoupled=decoupled, wd=wd, step=step, bias_correction=bias_correction, eps=eps, gs=gs)
            _one_update("adam", device, N, hp, seed=23, zero_state=step == 1)


@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov", "adam_l2", "adam_decoupled"])
@pytest.mark.parametrize("device", DEVICES)
def test_lr_zero_keeps_w_updates_state_refreshes_shadow(device, kind):
    kind, hp = _variant(kind)
    b, inp = _one_update(kind, device, N, dict(hp, lr=0.0), seed=24)
    assert OH.bits_equal(b.w.t.cpu(), inp["w"])
    for name, buf in b.state_names():
        assert not torch.equal(buf.t.cpu(), inp[name]), name
    assert OH.bits_equal(b.shadow.t.cpu(), inp["w"].bfloat16())


def _variant(name):
    return {"sgd": ("sgd", SGD), "momentum": ("momentum", MOMENTUM),
            "nesterov": ("momentum", dict(MOMENTUM, nesterov=True)),
            "adam_l2": ("adam", dict(ADAM, decoupled=False)), "adam_decoupled": ("adam", ADAM)}[name]


# -------------------------------------------------------------------------------------------- five steps in a row
@pytest.mark.parametrize("kind", ["momentum", "nesterov", "adam_l2", "adam_decoupled"])
@pytest.mark.parametrize("device", DEVICES)
def test_five_steps_carry_state(device, kind):
    """The state one launch writes is what the next reads: five updates with fresh gradients, compared once."""
    device = _device(device)
    kind, hp = _variant(kind)
    steps = 5
    inp = OH.make_inputs(N, 25, k=steps, zero_state=kind == "adam")
    b = Bufs(kind, device, inp)
    st = _ref_start(kind, inp)
    for i in range(steps):
        hp_i = dict(hp, step=i + 1) if kind == "adam" else hp
        _call(b, b.g[i].t, hp_i)
        _ref_step(kind, st, inp["g"][i], hp_i)
    k = steps * _k_single(kind, hp)["w"]
    _compare(b, st, dict(w=k, acc=k, m=k, v=k), "%s/%s x5" % (device, kind))


# ------------------------------------------------------------------------------------------------------------ dyn
@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov", "adam_decoupled"])
@pytest.mark.parametrize("device", DEVICES)
def test_dyn_overrides_scalars(device, kind):
    """dyn = [lr, lr_t, grad_scale] on the device replaces the scalar arguments: wrong scalars + dyn is bitwise the
    call with the right scalars.  Adam: lr != lr_t (bias correction at step 3) and decoupled decay, which uses lr,
    so reading one slot for both shows.  lr = 2^-10 is exact in fp32 (the PyTorch branch forms lr*wd on the host)."""
    device = _device(device)
    kind, hp = _variant(kind)
    hp = dict(hp, lr=2.0 ** -10, gs=0.5)
    inp = OH.make_inputs(N, 26)
    want = Bufs(kind, device, inp)
    _call(want, want.g[0].t, hp)
    lr_t = OH.adam_lr_t(hp["lr"], ADAM["b1"], ADAM["b2"], ADAM["step"]) if kind == "adam" else 123.0
    assert OH.f32(lr_t) != OH.f32(hp["lr"])
    dyn = torch.tensor([hp["lr"], lr_t, hp["gs"]], dtype=torch.float32, device=device)
    got = Bufs(kind, device, inp)
    _call(got, got.g[0].t, dict(hp, lr=99.0, gs=7.0, step=1), dyn=dyn)
    got.assert_contained("dyn")
    assert dyn.tolist() == [OH.f32(hp["lr"]), OH.f32(lr_t), 0.5]
    a, e = got.outputs(), want.outputs()
    for name in e:
        assert OH.bits_equal(a[name], e[name]), name
    # and the scalars alone do matter
    off = Bufs(kind, device, inp)
    _call(off, off.g[0].t, dict(hp, lr=99.0, gs=7.0, step=1))
    assert not torch.equal(off.w.t, want.w.t)


# ---------------------------------------------------------------------------------------------------- apply_multi
def _multi_lrs(k):
    return [0.1 / (1 + i) for i in range(k)], [0.013 / (1 + 0.5 * i) for i in range(k)]


def _multi_hp(kind, flag):
    if kind == "sgd":
        return dict(SGD)
    if kind == "momentum":
        return dict(MOMENTUM, nesterov=flag)
    return dict(ADAM, decoupled=flag)


def _multi_call(kind, b, grads, lrs, lrts, hp, flag):
    O.apply_multi_(kind, b.w.t, grads, b.t(b.s1), b.t(b.s2), b.t(b.shadow), lrs, lrts, momentum=hp.get("mom", 0.0),
                   beta1=hp.get("b1", 0.9), beta2=hp.get("b2", 0.999), epsilon=hp.get("eps", 1e-8),
                   grad_scale=hp["gs"], weight_decay=hp["wd"], flag=flag)


def _apply_multi(device, kind, k, g_dtype, flag, n=N, mixed=False):
    device = _device(device)
    hp = _multi_hp(kind, flag)
    lrs, lrts = _multi_lrs(k)
    if kind == "adam":
        lrs = [lr * 0.01 for lr in lrs]
    inp = OH.make_inputs(n, 27 + k, k=k, g_dtype=g_dtype)
    if mixed:
        inp["g"][1] = inp["g"][1].float() if g_dtype == torch.bfloat16 else inp["g"][1].bfloat16()
    b = Bufs(kind, device, inp)
    _multi_call(kind, b, [g.t for g in b.g], lrs, lrts, hp, flag)
    st = _ref_start(kind, inp)
    for g, lr, lr_t in zip(inp["g"], lrs, lrts):
        _ref_step(kind, st, g, hp, lr=lr, lr_t=lr_t)
    ks = _k_single(kind, hp)
    if k > 1:
        ks = {name: k * ks["w"] for name in ks}
    _compare(b, st, ks, "%s/multi-%s k=%d %s flag=%d n=%d" % (device, kind, k, str(g_dtype)[6:], flag, n))
    return b, inp, hp, lrs, lrts


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("g_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
@pytest.mark.parametrize("device", DEVICES)
def test_apply_multi(device, kind, k, g_dtype, flag):
    b, inp, hp, lrs, lrts = _apply_multi(device, kind, k, g_dtype, flag)
    if k == 1 and g_dtype == torch.float32 and kind != "adam":
        # the same arithmetic in the same order as the single-update kernel: bitwise
        one = Bufs(kind, device, inp)
        _call(one, one.g[0].t, dict(hp, lr=lrs[0]))
        a, e = b.outputs(), one.outputs()
        for name in e:
            assert OH.bits_equal(a[name], e[name]), name


@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
@pytest.mark.parametrize("device", DEVICES)
def test_apply_multi_mixed_dtypes_fall_back(device, kind):
    _apply_multi(device, kind, 3, torch.bfloat16, True, mixed=True)


@pytest.mark.parametrize("device", DEVICES)
def test_apply_multi_refuses_nine(device):
    device = _device(device)
    inp = OH.make_inputs(64, 30, k=9)
    b = Bufs("sgd", device, inp)
    before = b.w.buf.clone()
    with pytest.raises((AssertionError, RuntimeError)):
        O.apply_multi_("sgd", b.w.t, [g.t for g in b.g], None, None, b.shadow.t, [0.1] * 9, [0.1] * 9)
    assert torch.equal(b.w.buf, before)


# ------------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov", "adam_l2", "adam_decoupled", "multi_nesterov",
                                  "multi_adam_l2"])
@pytest.mark.parametrize("device", DEVICES)
def test_inf_and_nan_stay_in_their_elements(device, kind):
    """One inf and one NaN gradient, in different float4s: w, state and shadow are non-finite exactly where the fp64
    reference is (``check`` asserts the positions), the other lanes of those float4s within the bound."""
    device = _device(device)
    n, bad = 64, {5: float("inf"), 18: float("nan")}
    multi = kind.startswith("multi_")
    kind, hp = _variant(kind[6:] if multi else kind)
    inp = OH.make_inputs(n, 31, k=2 if multi else 1)
    for i, x in bad.items():
        inp["g"][-1][i] = x
    b = Bufs(kind, device, inp)
    st = _ref_start(kind, inp)
    if multi:
        lrs, lrts = _multi_lrs(2)
        _multi_call(kind, b, [g.t for g in b.g], lrs, lrts, hp, hp.get("decoupled", hp.get("nesterov", False)))
        for g, lr, lr_t in zip(inp["g"], lrs, lrts):
            _ref_step(kind, st, g, hp, lr=lr, lr_t=lr_t)
        ks = {name: 2 * _k_single(kind, hp)["w"] for name in ("w", "acc", "m", "v")}
    else:
        _call(b, b.g[0].t, hp)
        _ref_step(kind, st, inp["g"][0], hp)
        ks = _k_single(kind, hp)
    _compare(b, st, ks, "%s/%s special" % (device, kind))
    nonfinite = (~torch.isfinite(b.w.t)).nonzero().flatten().tolist()
    assert nonfinite == sorted(bad), nonfinite
    assert (~torch.isfinite(b.shadow.t.float())).nonzero().flatten().tolist() == sorted(bad)


# -------------------------------------------------------------------------------- argument rejection (no launch)
def _entry_points(w, g, s1, s2, shadow, gb=None):
    return {
        "sgd": lambda: O.sgd_(w, g, shadow, 0.1, 0.5, 1e-2),
        "momentum": lambda: O.momentum_(w, g, s1, shadow, 0.1, 0.9, 0.5, 1e-2, False),
        "adam": lambda: O.adam_(w, g, s1, s2, shadow, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5, 1e-2, True),
        "apply_multi": lambda: O.apply_multi_("adam", w, [gb if gb is not None else g], s1, s2, shadow, [0.1], [0.1]),
    }


@pytest.mark.parametrize("entry", ["sgd", "momentum", "adam", "apply_multi"])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_rejects_n_not_multiple_of_4(device, entry):
    """The kernels drop n & 3 trailing elements; only the host check stands between a 6-element slice and a
    silently partial update."""
    device = _device(device)
    inp = OH.make_inputs(6, 32)
    bufs = [OH.Guarded(inp[k] if k != "g" else inp["g"][0], device) for k in ("w", "g", "m", "v")]
    shadow = OH.Guarded(None, device, torch.bfloat16, 6)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _entry_points(*[b.t for b in bufs], shadow.t)[entry]()
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in bufs) and shadow.unchanged()


_USES = {"sgd": "w g shadow", "momentum": "w g s1 shadow", "adam": "w g s1 s2 shadow",
         "apply_multi": "w g s1 s2 shadow bf16_grad"}


@pytest.mark.parametrize("entry,which", [(e, w) for e, ws in _USES.items() for w in ws.split()])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_rejects_misaligned_pointers(device, entry, which):
    """fp32 buffers move as float4 (16 bytes), shadow and bf16 gradients as 4 x bf16 (8 bytes)."""
    device = _device(device)
    n = 8
    f = {k: torch.full((n + 8,), 0.5, device=device) for k in ("w", "g", "s1", "s2")}
    h = {k: torch.full((n + 8,), 0.5, device=device, dtype=torch.bfloat16) for k in ("shadow", "bf16_grad")}
    before = {k: t.clone() for k, t in list(f.items()) + list(h.items())}
    # 4 bytes past a 16-byte boundary for fp32, 4 bytes past an 8-byte boundary for bf16
    view = {k: t[5:5 + n] if k == which else t[4:4 + n] for k, t in f.items()}
    view.update({k: t[6:6 + n] if k == which else t[4:4 + n] for k, t in h.items()})
    assert view[which].data_ptr() % (8 if which in h else 16) == 4
    with pytest.raises(RuntimeError, match="invalid argument"):
        _entry_points(view["w"], view["g"], view["s1"], view["s2"], view["shadow"],
                      view["bf16_grad"] if which == "bf16_grad" else None)[entry]()
    torch.cuda.synchronize()
    for k, t in list(f.items()) + list(h.items()):
        assert torch.equal(t, before[k]), k


# ------------------------------------------------------------------------------------------------ kernel variants
@pytest.mark.parametrize("device", GPU_ONLY)
def test_kernel_variants_bitwise_equal(device, tmp_path):
    """MDTF_NT_OPT=0 (cached instead of nontemporal loads / stores) and MDTF_ADAM_CHUNK=0 (grid-stride Adam) are
    read once per process, so each combination runs in a fresh child; the arithmetic per element is the same, so
    every output equals the default build's bitwise."""
    _device(device)
    assert os.environ.get("MDTF_NT_OPT", "1") != "0" and os.environ.get("MDTF_ADAM_CHUNK", "1") != "0"
    want = VC.compute()
    for i, extra in enumerate([{"MDTF_NT_OPT": "0", "MDTF_ADAM_CHUNK": "0"}, {"MDTF_ADAM_CHUNK": "0"},
                               {"MDTF_NT_OPT": "0"}]):
        env = {k: v for k, v in os.environ.items() if k not in ("MDTF_NT_OPT", "MDTF_ADAM_CHUNK")}
        env.update(extra)
        out = str(tmp_path / ("variant%d.pt" % i))
        r = subprocess.run([sys.executable, os.path.abspath(VC.__file__), out], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, "child %r exited %d:\n%s" % (extra, r.returncode, r.stdout[-4000:])
        got = torch.load(out)
        assert sorted(got) == sorted(want) and len(want) >= 20
        for name in want:
            assert OH.bits_equal(got[name], want[name]), (extra, name)
