"""Store-first gradient slots (train/variables.py claim_store / note_accumulate / unclaimed_skips and
parallel/flat.py zero_grad(skip_stored)): CPU bookkeeping checks; the kernel side is in test_kernels_gpu.py
(test_grad_store_first_matches_zero_and_accumulate, test_fill_ranges_zero)."""
import torch

from mdtf.parallel.flat import FlatGroup
from mdtf.train import variables as V


def _group():
    vs = [V.Variable("a", torch.ones(5, 3)), V.Variable("b", torch.ones(7)), V.Variable("c", torch.ones(130))]
    return FlatGroup(vs, "cpu", None, False), vs


def test_zero_grad_skips_only_store_written_slots():
    g, (a, b, c) = _group()
    g.grad.fill_(1.0)
    b.store_first = True
    g.zero_grad(skip_stored=True)
    assert a.grad.abs().sum() == 0 and c.grad.abs().sum() == 0
    assert torch.equal(b.grad, torch.ones(7)) and b.skip_zero
    assert g.grad.sum() == 7                      # alignment gaps zeroed too
    g.grad.fill_(1.0)
    g.zero_grad()                                 # the full fill (backup replicas, async PS) ignores the flags
    assert g.grad.abs().sum() == 0 and not b.skip_zero


def test_claim_store_first_write_only(monkeypatch):
    monkeypatch.setattr(V, "STORE_FIRST", True)
    g, (a, b, c) = _group()
    V.begin_grad_epoch()
    assert V.claim_store(a)                       # the step's first (full-slot) write: overwrite
    assert not V.claim_store(a)                   # a second write the same step accumulates
    V.note_accumulate(b)                          # b's first write accumulates ...
    assert not V.claim_store(b)                   # ... so a later full-slot writer must too
    assert a.store_first and not b.store_first
    # next step: a's slot is skipped by the fill; an accumulating first write zeroes it before adding
    g.grad.fill_(3.0)
    g.zero_grad(skip_stored=True)
    V.begin_grad_epoch()
    assert a.skip_zero and a.grad.sum() == 45
    V.note_accumulate(a)
    assert a.grad.abs().sum() == 0 and not a.store_first
    # a skipped slot nobody writes in a step is zeroed at the end of backward
    a.store_first = True
    g.grad.fill_(2.0)
    g.zero_grad(skip_stored=True)
    V.begin_grad_epoch()
    V.unclaimed_skips([a, b, c])
    assert a.grad.abs().sum() == 0


def test_claim_store_disabled(monkeypatch):
    monkeypatch.setattr(V, "STORE_FIRST", False)
    _, (a, _, _) = _group()
    V.begin_grad_epoch()
    a.uses = 1
    assert not V.claim_store(a)


# ---- every in-place writer goes through V.accumulate_slot / V.store_slot -------------------------------------
# A "step" is what train/step.py does around a backward.  Each scenario runs with store-first on and off; the slots
# after the last step must be equal bit for bit (on the CPU both runs are the same arithmetic), and the slot under
# test must have been skipped by the fill of the last step in the store-first run (else the test shows nothing).
import pytest  # noqa: E402

import test_conv_dispatch as D  # noqa: E402
from mdtf.ops import conv as C, gemm, kernels  # noqa: E402

STALE = 1000.0


def _step(g, vs, run):
    V.begin_grad_epoch()
    g.zero_grad(skip_stored=True)
    for v in vs:
        v.uses = 0
    skipped = [v.skip_zero for v in vs]
    run()
    V.unclaimed_skips(vs)
    return skipped


def _stored_step(g, vs, stored):
    """Step 1: a store kernel's write of ``stored``, emulated."""
    def run():
        for v in stored:
            V.claim_store(v)
            v.grad.fill_(STALE)
            v.uses = 0
    _step(g, vs, run)


def _on_off(monkeypatch, scenario):
    """``scenario()`` -> (slots, skipped flags of the last step) with store-first on and off."""
    monkeypatch.setattr(kernels, "colsum_into", lambda x2d, out: out.add_(x2d.float().sum(0)))   # (a HIP kernel)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(V, "STORE_FIRST", on)
        out[on] = scenario()
    (g_on, skipped), (g_off, _) = out[True], out[False]
    assert all(skipped), skipped                       # not vacuous: the fill left the stored slots out
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)
    return g_on


def _dense_scenario(shapes, nstored, forward):
    gen = torch.Generator().manual_seed(3)
    vs = [V.Variable("v%d" % i, torch.randn(s, generator=gen)) for i, s in enumerate(shapes)]
    g = FlatGroup(vs, "cpu", torch.bfloat16, False)
    x = torch.randn(16, 32, generator=gen).to(torch.bfloat16)
    _stored_step(g, vs, vs[:nstored])

    def run():
        y = forward(x, [v.read(torch.bfloat16) for v in vs])
        y.backward(torch.randn(y.shape, generator=gen).to(y.dtype))
    skipped = _step(g, vs, run)
    return [v.grad.clone() for v in vs], skipped[:nstored]


@pytest.mark.parametrize("name,shapes,nstored,forward", [
    ("dense", [(32, 48), (48,)], 1, lambda x, r: gemm.dense(x, r[0], r[1])),
    ("dense_multi", [(32, 48), (32, 48), (48,), (48,)], 2, lambda x, r: gemm.dense_multi(x, r[:2], r[2:])),
    ("dense_transposed", [(48, 32), (48,)], 1, lambda x, r: gemm.dense_transposed(x, r[0], r[1])),
])
def test_dense_fallback_after_a_stored_step(monkeypatch, name, shapes, nstored, forward):
    grads = _on_off(monkeypatch, lambda: _dense_scenario(shapes, nstored, forward))
    for gr in grads[:nstored]:
        assert 0 < gr.abs().max() < STALE / 2                # no trace of the stale constant


class _StoredSink(D.Scenario):
    """The dispatch recorder with the filter's sink a real Variable whose slot a store kernel wrote the step
    before; random operands, for the paths that compute on the CPU."""

    def t(self, name, shape, dtype=D.BF16, grad=False):
        t = super().t(name, shape, dtype, False)
        if name in ("x", "w", "dy"):
            t.copy_(torch.randn(tuple(shape), generator=torch.Generator().manual_seed(len(name))))
        return t.requires_grad_(True) if grad else t

    def forward(self, x, w, *args):
        self.var = V.Variable("w", torch.zeros(w.shape))
        self.group = FlatGroup([self.var], "cpu", None, False)
        self.rec.name("w_slot", self.var.grad)
        w._mdtf_var = self.var
        _stored_step(self.group, [self.var], [self.var])
        V.begin_grad_epoch()
        self.group.zero_grad(skip_stored=True)
        self.skipped = self.var.skip_zero
        return super().forward(x, w, *args)


def _conv_scenario(case, on, env=None, **kwargs):
    with pytest.MonkeyPatch.context() as mp:
        s = _StoredSink(mp)
        if env:
            mp.setenv("MDTF_CONV", env)
        mp.setattr(V, "STORE_FIRST", on)
        mp.setattr(V, "GRAD_EPOCH", [1])
        case(s, wsink=True, **kwargs)
        declared = s.var.written_epoch == V.GRAD_EPOCH[0]
        return s.var.grad.clone(), s.skipped, declared, s.result()["calls"]


def test_conv_miopen_wgrad_after_a_stored_step():
    (g_on, skipped, declared, _), (g_off, _, _, _) = [_conv_scenario(D.conv_case, on, env="miopen", **D.V2)
                                                      for on in (True, False)]
    assert skipped and declared
    assert torch.equal(g_on, g_off)
    assert g_on.abs().sum() > 0


@pytest.mark.parametrize("packed", [True, False])
def test_stem_wgrad_after_a_stored_step(packed):
    (grad, skipped, declared, calls), (g_off, _, _, _) = [_conv_scenario(D.stem_case, on, packed=packed)
                                                          for on in (True, False)]
    assert skipped and declared                      # the write was declared ...
    assert torch.equal(grad, g_off)                  # ... so the stale sum was zeroed
    if packed:                                       # (the recorder computes nothing; unpacked: the library path)
        assert grad.abs().sum() == 0
        launch = [c for c in calls if c[0] == "mdtf_stem_wgrad"]
        assert len(launch) == 1 and "w_slot" in launch[0]
        assert calls.index(["V.note_accumulate"]) < calls.index(launch[0])


class _InPlace(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, declare):
        ctx.sink, ctx.like, ctx.declare = V.grad_sink(w), w, declare
        return w.sum()

    @staticmethod
    def backward(ctx, dy):
        slot = V.accumulate_slot(ctx.sink) if ctx.declare else ctx.sink.master     # (any tensor: undeclared)
        slot.add_(0)
        return V.grad_marker(ctx.like), None


def test_undeclared_in_place_write_is_refused():
    g, (a, b, c) = _group()
    V.begin_grad_epoch()
    _InPlace.apply(a.read(), True).backward()
    V.begin_grad_epoch()
    with pytest.raises(RuntimeError, match="a.*accumulate_slot / store_slot"):
        _InPlace.apply(a.read(), False).backward()


def test_accessor_semantics(monkeypatch):
    monkeypatch.setattr(V, "STORE_FIRST", True)
    a = V.Variable("a", torch.ones(5, 3))
    a.pad_rows = 3
    g = FlatGroup([a], "cpu", None, False)
    V.begin_grad_epoch()
    slot, store = V.store_slot(a)
    assert store and slot is a.grad and a.store_first
    assert V.store_slot(a) == (a.grad, False)                        # once per epoch
    # the next step's fill skips the slot: accumulate_slot zeroes it, once
    g.grad.fill_(3.0)
    g.zero_grad(skip_stored=True)
    V.begin_grad_epoch()
    assert a.skip_zero and a.grad.sum() == 45
    assert V.accumulate_slot(a) is a.grad and a.grad.abs().sum() == 0 and not a.store_first
    a.grad.fill_(1.0)
    assert V.accumulate_slot(a).sum() == 15                           # the second writer adds onto the first
    assert V.accumulate_slot(a, padded=True) is a.grad_padded and a.grad_padded.shape == (8, 3)
    assert V.store_slot(a, padded=True)[0] is a.grad_padded
    assert V.accumulate_slot(None) is None
    # store-first off: never a store; the slot is declared and (were it skipped) zeroed
    monkeypatch.setattr(V, "STORE_FIRST", False)
    a.grad.fill_(2.0)
    V.begin_grad_epoch()
    slot, store = V.store_slot(a)
    assert not store and slot is a.grad and a.written_epoch == V.GRAD_EPOCH[0] and a.grad.abs().sum() == 0
