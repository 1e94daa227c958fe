"""The row kernels of ``csrc/transformer.hip`` (LayerNorm with fused dropout and residual and its two backward forms,
the masked scaled softmax, the embedding gather / scatter-add, the fused BERT embedding) against the independent fp64
oracles of ``transformer_helpers``, element by element, at the smallest shapes that reach each template and code path.

Every test takes a device: ``cpu`` runs the PyTorch branch of ``mdtf.ops.transformer`` on fp32 tensors holding
bf16-representable values (this validates the oracle and the bounds without a GPU); ``cuda`` runs the HIP kernels
twice, through the autograd wrappers and through the registered entry points with every buffer (``mean``, ``rstd``,
the gradient slots and the workspaces included) inside sentinel guard bands: guards intact, inputs bitwise unchanged,
every output element stored.

The bounds are those of ``transformer_helpers`` (derivations and the measured CPU constant in its docstring); the
operation count k of every ``gamma(k)`` stands next to its use there.  The env-selected forms (``MDTF_LN_BWD``,
``MDTF_LN_BWD_RPB``, ``MDTF_LN_ATOMICS``, ``MDTF_LN_NT``, ``MDTF_EMBED_SMALL_2PASS``) run in fresh child processes
(``transformer_variant_child.py``) and are checked against the same oracle and bounds, never against the default
form's outputs.  The ``test_check_fails_*`` tests perturb copies of CPU outputs and require the checks to raise.
"""
import os
import subprocess
import sys

import pytest
import torch

from mdtf.ops import _native
from mdtf.ops import transformer as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transformer_helpers as TH  # noqa: E402
import transformer_variant_child as VC  # noqa: E402
from transformer_helpers import U, gamma  # noqa: E402

DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
CPU_ONLY = [pytest.param("cpu")]
MDTF_EINVAL, MDTF_EUNSUPPORTED = -1, -2


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        _native.lib()
        assert _native.mode() != "torch" and not _native.deterministic()
    return device


def _blocks(device, rows, H):
    return int(VC.call_ws("mdtf_ln_bwd_ws", rows, H)) // (2 * H) if device == "cuda" else 0


# ================================================================================================== LayerNorm
class _Var(object):                     # what variables.grad_sink looks for: an fp32 gradient slot
    def __init__(self, grad):
        self.grad = grad


def _ln_run(device, x, res, g, b, dy, p=0.0, seed=0, slots=None):
    """Through ``layer_norm`` (with dropout: ``_LayerNorm.apply``, which takes the seed).  ``slots``: the
    (dgamma, dbeta) gradient slots, attached the way a Variable's are."""
    xd = TH.put(x, device).requires_grad_(True)
    rd = TH.put(res, device).requires_grad_(True) if res is not None else None
    gd, bd = g.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    if slots is not None:
        if device == "cuda":
            gd._mdtf_var, bd._mdtf_var = _Var(slots[0]), _Var(slots[1])
        else:
            gd.grad, bd.grad = slots
    if p:
        y = T._LayerNorm.apply(xd, rd, gd, bd, TH.EPS, float(p), seed)
    else:
        y = T.layer_norm(xd, gd, bd, TH.EPS, residual=rd)
    y.backward(TH.put(dy, device))
    if device == "cuda":
        torch.cuda.synchronize()
    on_slot = slots is not None and device == "cuda"
    return dict(y=y.detach(), dx=xd.grad, dres=rd.grad if rd is not None else None,
                dgamma=slots[0] if on_slot else gd.grad, dbeta=slots[1] if on_slot else bd.grad)


def _check_ln_fwd(what, device, fref, g, b, y, s=None, mean=None, rstd=None, aten=None):
    aten = (device == "cpu") if aten is None else aten
    fb = TH.ln_fwd_bounds(fref, g, b, device, aten=aten)
    if mean is not None:
        TH.check(mean, fref["mean"], fb["mean"], what + " mean")
        TH.check(rstd, fref["rstd"], fb["rstd"], what + " rstd")
    if s is not None:
        TH.check(s, fref["s"], fb["s"], what + " s")
    TH.check(y, fref["y"], fb["y"], what + " y")
    return fb


def _check_ln_bwd_raw(what, c, r, p, seed, device="cuda"):
    """The raw backward's outputs ``r`` against the oracle at the same s, mean, rstd."""
    rows, H = c["s"].shape
    keep = TH.hash_keep(seed, rows * H, p).view(rows, H) if p else None
    ref = TH.ln_bwd_ref(c["dy"], c["s"], c["mean"], c["rstd"], c["g"], keep, p, r["dg0"], r["db0"])
    bb = TH.ln_bwd_raw_bounds(ref, int(r["blocks"]), device)
    TH.check(r["dx"], ref["dx"], bb["dx"], what + " dx")
    if p:
        TH.check(r["dxb"], ref["dxb"], bb["dxb"], what + " dx_branch")
    TH.check(r["dgamma"], ref["dgamma"], bb["dgamma"], what + " dgamma")
    TH.check(r["dbeta"], ref["dbeta"], bb["dbeta"], what + " dbeta")


def _check_ln_autograd(what, device, x, res, g, b, dy, out, keep=None, p=0.0, dg0=None, db0=None):
    """Forward y and the wrapper's gradients against fp64 autograd of the true function."""
    rows, H = x.shape
    aten = device == "cpu"
    fref = TH.ln_fwd_ref(x, res, g, b, keep, p)
    fb = _check_ln_fwd(what, device, fref, g, b, out["y"])
    ar = TH.ln_autograd_ref(x, res, g, b, dy, keep, p, dg0, db0)
    blocks = _blocks(device, rows, H)
    bb = TH.ln_bwd_autograd_bounds(fref, fb, g, dy, blocks, device, aten, dg0, db0)
    b0 = TH.ln_bwd_autograd_bounds(fref, fb, g, dy, blocks, device, aten, dg0, db0, saved_term=False)
    ds = bb["ref"]["dx"]                                    # d loss / d s, analytic: must be autograd's
    want = ar["dres"] if res is not None else (ar["dx"] if keep is None else None)
    if want is not None:
        assert float((ds - want).abs().max()) <= 1e-10 * float(bb["ref"]["T"].max().clamp(min=1e-30)), what
    share = float(((bb["dx"] - b0["dx"]) / bb["dx"]).mean())
    print("TRF_SAVED %-60s the bf16-saved s: %.0f %% of the dx bound on average" % (what, 100 * share))
    if res is not None:
        TH.check(out["dres"], ds, bb["dx"], what + " dres")
    if keep is None:
        TH.check(out["dx"], ds, bb["dx"], what + " dx")
    else:
        # k = 3: 1 - p, the reciprocal, the product; a dropped element is exactly 0
        kp = keep.double() / (1.0 - TH.f32(p))
        e = kp * (bb["e_dx"] * (1.0 + gamma(3)) + gamma(3) * ds.abs())
        TH.check(out["dx"], ar["dx"], TH.out_bound(ar["dx"], e, device == "cuda"), what + " dx_branch")
    TH.check(out["dgamma"], ar["dgamma"], bb["dgamma"], what + " dgamma")
    TH.check(out["dbeta"], ar["dbeta"], bb["dbeta"], what + " dbeta")
    return fref, fb


def _cpu_rstd_units(what, x, res, g, b, fref):
    """The measured constant of ``transformer_helpers``, asserted where it was measured: fp32 native_layer_norm's
    rstd over the rows whose mean lies within 4 standard deviations of 0 (beyond that ATen's merge of chunk moments
    sets the error, not the reciprocal square root; the bound's ``aten`` term covers it)."""
    s = x if res is None else x + res
    _, mean, rstd = torch.native_layer_norm(s, (s.shape[1],), g, b, TH.EPS)
    fb = TH.ln_fwd_bounds(fref, g, b, "cpu", aten=True)
    TH.check(mean.reshape(-1), fref["mean"], fb["mean"], what + " mean")
    TH.check(rstd.reshape(-1), fref["rstd"], fb["rstd"], what + " rstd")
    sel = fref["mean"].abs() * fref["rstd"] <= 4.0
    if sel.any():
        units = float(((rstd.reshape(-1).double() - fref["rstd"]).abs() / (U * fref["rstd"]))[sel].max())
        print("TRF_CPU %-62s rstd %.3f units" % (what, units))
        assert units <= TH.RSTD_UNITS_CPU, (what, units)


def _ln_case(device, rows, H, with_res, seed):
    what = "%s/ln %dx%d res=%d" % (device, rows, H, with_res)
    x, res, g, b, dy = TH.ln_inputs(rows, H, seed, with_res)
    out = _ln_run(device, x, res, g, b, dy)
    fref, _ = _check_ln_autograd(what, device, x, res, g, b, dy, out)
    if device == "cpu":
        _cpu_rstd_units(what, x, res, g, b, fref)
        return
    f = VC.ln_fwd_raw(what + " raw fwd", x, res, g, b)
    _check_ln_fwd(what + " raw", device, fref, g, b, f["y"], f["s"], f["mean"], f["rstd"])
    assert TH.bits_equal(f["y"], out["y"]), what + ": the entry point and the wrapper differ"
    c = VC.ln_raw_inputs(rows, H, seed)
    _check_ln_bwd_raw(what + " raw bwd", c, VC.ln_bwd_raw(what + " raw bwd", c), 0.0, 0)


def _ln_row_counts(H):
    return (1, 3, 9) if H == 8192 else (1, 3, 37)


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("H", VC.LN_H)
@pytest.mark.parametrize("device", DEVICES)
def test_layernorm(device, H, with_res):
    """One H per instantiated template (``VC.LN_H``); rows 1, 3 and 37: partial blocks, idle slices, a half-filled
    wave for the 32-lane templates (9 rows at H = 8192)."""
    device = _device(device)
    for rows in _ln_row_counts(H):
        _ln_case(device, rows, H, with_res, 100 + H + rows)


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("device", DEVICES)
def test_layernorm_second_row_loop_trip(device, H):
    """8197 rows: ln_bwd_geometry gives 17 rows per block, so at H = 64 (4 slices of 4 rows in flight) the row loop
    takes a second trip that holds a single row; at H = 256 (8 half-wave slices) the last rows in flight are idle."""
    device = _device(device)
    if device == "cuda":
        assert VC.call_ws("mdtf_ln_bwd_ws", 8197, H) == 483 * 2 * H
    for with_res in (False, True):
        _ln_case(device, 8197, H, with_res, 300 + H)


@pytest.mark.parametrize("H", [520, 768])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_layernorm_dropout(device, H):
    """p = 0.1 on the branch input: the keep bits are the counter hash with the seed ``effective_seed`` gives
    (the CPU branch draws its mask from PyTorch's generator, so there is nothing to compare on ``cpu``)."""
    device = _device(device)
    rows, p, seed = 37, 0.1, 123457
    what = "%s/ln dropout %dx%d" % (device, rows, H)
    x, res, g, b, dy = TH.ln_inputs(rows, H, 400 + H, True)
    keep = TH.hash_keep(T.effective_seed(seed, torch.device("cuda", torch.cuda.current_device())), rows * H,
                        p).view(rows, H)
    assert 0.8 < float(keep.float().mean()) < 0.97
    out = _ln_run(device, x, res, g, b, dy, p, seed)
    fref, _ = _check_ln_autograd(what, device, x, res, g, b, dy, out, keep, p)
    assert bool((out["dx"].cpu()[~keep] == 0).all())
    # the entry points take the seed as it is (no step counter)
    keep = TH.hash_keep(seed, rows * H, p).view(rows, H)
    fref = TH.ln_fwd_ref(x, res, g, b, keep, p)
    f = VC.ln_fwd_raw(what + " raw fwd", x, res, g, b, p, seed)
    _check_ln_fwd(what + " raw", device, fref, g, b, f["y"], f["s"], f["mean"], f["rstd"])
    c = VC.ln_raw_inputs(rows, H, 400 + H)
    _check_ln_bwd_raw(what + " raw bwd", c, VC.ln_bwd_raw(what + " raw bwd", c, p, seed), p, seed)


@pytest.mark.parametrize("H", [72, 768, 2056])
@pytest.mark.parametrize("device", DEVICES)
def test_layernorm_value_edges(device, H):
    """Rows of ``ln_edge_inputs``.  Constant rows (all 2.0, all 0): every partial sum is exact, so mean is the value,
    rstd is eps^-1/2 = 1e6 to the intrinsic's accuracy, y is beta exactly and dx is the centred g times 1e6.  The row
    1000 +- {0, 4, 8}: a one-pass variance would lose it; the bounds of the two-pass form hold."""
    device = _device(device)
    what = "%s/ln edges H=%d" % (device, H)
    x, res, g, b, dy = TH.ln_edge_inputs(H, 500 + H)
    out = _ln_run(device, x, res, g, b, dy)
    fref = TH.ln_fwd_ref(x, res, g, b)
    assert abs(float(fref["rstd"][0]) - 1e6) < 1.0 and float(fref["rstd"][1]) < 1.0
    y = out["y"].float().cpu()
    assert torch.equal(y[0], b) and torch.equal(y[2], b), what + ": y of a constant row is not beta"
    if device == "cuda":
        f = VC.ln_fwd_raw(what + " raw fwd", x, res, g, b)
        mean, rstd, sv = f["mean"].cpu(), f["rstd"].cpu(), f["s"]
        assert TH.bits_equal(sv.cpu(), x.bfloat16()), what + ": s is not x"
        assert TH.bits_equal(f["y"], out["y"])
    else:
        _, mean, rstd = torch.native_layer_norm(x, (H,), g, b, TH.EPS)
        mean, rstd = mean.reshape(-1), rstd.reshape(-1)
    assert float(mean[0]) == 2.0 and float(mean[2]) == 0.0, what
    units = TH.RSTD_UNITS_CPU * (TH.INTRINSIC_FACTOR if device == "cuda" else 1.0)
    for r in (0, 2):                                            # var is exactly 0: only the add of eps and the rsqrt
        assert abs(float(rstd[r]) - float(fref["rstd"][r])) <= (units + 1) * U * 1e6, (what, r, float(rstd[r]))
    # rows 1 and 3 under the general bounds (the constant rows' bounds cannot know that their sums are exact)
    sel = [1, 3]
    fsel = TH.ln_fwd_ref(x[sel], None, g, b)
    _check_ln_fwd(what + " rows 1,3", device, fsel, g, b, out["y"][sel], None, mean[sel], rstd[sel])
    # backward: the kernel reads the statistics it saved; with var = 0 exactly the constant rows are raw cases
    ar = TH.ln_autograd_ref(x, res, g, b, dy)
    fb = TH.ln_fwd_bounds(fsel, g, b, device, aten=device == "cpu")
    bb = TH.ln_bwd_autograd_bounds(fsel, fb, g, dy[sel], _blocks(device, 4, H), device, device == "cpu")
    TH.check(out["dx"][sel], ar["dx"][sel], bb["dx"], what + " dx rows 1,3")
    for r in (0, 2):
        c = dict(dy=dy[r:r + 1], s=x[r:r + 1], g=g, mean=mean[r:r + 1].float(), rstd=rstd[r:r + 1].float())
        ref = TH.ln_bwd_ref(c["dy"], c["s"], c["mean"], c["rstd"], g)
        assert float(ref["dx"].abs().max()) > 1e5, what
        e = TH.ln_bwd_raw_bounds(ref, 0, device, device == "cuda")
        if device == "cpu":
            # ATen: a dy gamma + b s + c with b s + c = rstd^3 mean (...) cancelling: relative to the uncentred terms
            m, rs, gg = c["mean"].double(), c["rstd"].double(), ref["gg"]
            B = rs ** 3 * (m.abs() * gg.abs().mean() + (gg * x[r].double()).abs().mean())
            e["dx"] = e["dx"] + gamma(H + 12) * (B * (x[r].double().abs() + m.abs()) + rs * gg.abs().mean())
        TH.check(out["dx"][r:r + 1], ref["dx"], e["dx"], what + " dx constant row %d" % r)
    if device == "cuda":
        # the raw backward over all four rows at the kernel's own statistics
        c = dict(dy=dy, s=x, g=g, mean=mean.float(), rstd=rstd.float())
        _check_ln_bwd_raw(what + " raw bwd", c, VC.ln_bwd_raw(what + " raw bwd", c), 0.0, 0)


@pytest.mark.parametrize("slots", VC.SLOTS)
@pytest.mark.parametrize("device", DEVICES)
def test_layernorm_grad_slots(device, slots):
    """dgamma / dbeta into separate zero buffers, one flat buffer [dgamma | dbeta] (one [blocks, 2H] reduction),
    [dbeta | dgamma] (``beta_first``: the partial rows swapped) and slots that already hold values (+=); through
    the autograd wrapper with the slots attached as a Variable's are, and through the entry point."""
    device = _device(device)
    for H, rows in ((768, 37), (520, 37), (64, 3)):
        what = "%s/ln slots %s %dx%d" % (device, slots, rows, H)
        x, res, g, b, dy = TH.ln_inputs(rows, H, 600 + H, True)
        hold, dg, db, dg0, db0 = VC.make_slots(slots, H, device)
        if slots == "separate":
            dg0 = db0 = None
        if device == "cuda" and slots == "gamma_beta":
            assert db.data_ptr() == dg.data_ptr() + 4 * H
        if device == "cuda" and slots == "beta_gamma":
            assert dg.data_ptr() == db.data_ptr() + 4 * H
        out = _ln_run(device, x, res, g, b, dy, slots=(dg, db))
        _check_ln_autograd(what, device, x, res, g, b, dy, out, dg0=dg0, db0=db0)
        if device == "cuda":
            assert all(h.guards_intact() for h in hold), what
            c = VC.ln_raw_inputs(rows, H, 600 + H)
            _check_ln_bwd_raw(what + " raw", c, VC.ln_bwd_raw(what + " raw", c, slots=slots), 0.0, 0)


# ==================================================================================================== softmax
SOFTMAX_COLS = [8, 40, 128, 512, 520, 1024, 2056]


def _softmax_run(device, x, mask, scale, dy):
    xd = TH.put(x, device).requires_grad_(True)
    y = T.masked_softmax(xd, mask.to(device) if mask is not None else None, scale)
    y.backward(TH.put(dy, device))
    return y.detach(), xd.grad


def _check_softmax(what, device, x, mask, scale, dy, y, dx, saved=None):
    p = TH.softmax_ref(x, mask, scale)
    TH.check_nb(y, p, what + " y")
    saved = y if saved is None else saved
    ref, bound = TH.softmax_bwd_bounds(saved.float().cpu(), dy, scale, device, False)
    TH.check(dx, ref, bound, what + " dx at the saved y")
    ref, bound = TH.softmax_bwd_bounds(p, dy, scale, device, True)
    TH.check(dx, ref, bound, what + " dx true")


@pytest.mark.parametrize("mask_kind", ["none", "sparse", "full"])
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
@pytest.mark.parametrize("device", DEVICES)
def test_softmax(device, cols, mask_kind):
    """cols 8 .. 512: NV = 1 | 520: NV = 2, one lane in the second vector | 1024 | 2056: NV = 8, one lane in the
    fifth vector.  B = 3 with 15 rows per batch: a 4-row block straddles two batches.  scale 0.125 and 1."""
    device = _device(device)
    B, heads, sq = 3, 3, 5
    x, mask, dy = TH.softmax_inputs(B, heads, sq, cols, 700 + cols, mask_kind)
    for scale in (0.125, 1.0):
        what = "%s/softmax cols=%d mask=%s scale=%g" % (device, cols, mask_kind, scale)
        y, dx = _softmax_run(device, x, mask, scale, dy)
        _check_softmax(what, device, x, mask, scale, dy, y, dx)
        if device == "cuda":
            rows = B * heads * sq
            gx, gdy = TH.Guarded(x.bfloat16(), device), TH.Guarded(dy.bfloat16(), device)
            gm = TH.Guarded(mask, device) if mask is not None else None
            gy, gdx = (TH.Guarded(None, device, torch.bfloat16, x.shape) for _ in range(2))
            assert VC.call("mdtf_softmax_fwd", VC._p(gx), VC._p(gm), VC._p(gy), rows, cols, scale, heads * sq) == 0
            gyi = TH.Guarded(gy.t, device)
            assert VC.call("mdtf_softmax_bwd", VC._p(gdy), VC._p(gyi), VC._p(gdx), rows, cols, scale) == 0
            TH.assert_contained(what + " raw", [gx, gdy, gyi] + ([gm] if gm else []), [gy, gdx])
            _check_softmax(what + " raw", device, x, mask, scale, dy, gy.t, gdx.t)
            assert TH.bits_equal(gy.t, y) and TH.bits_equal(gdx.t, dx)


# ================================================================================================== embedding
def _embed_run(device, table, ids, dy, slot=None):
    td = TH.put(table, device).requires_grad_(True)
    if slot is not None:
        if device == "cuda":
            td._mdtf_var = _Var(slot)
        else:
            td.grad = slot
    out = T.embedding_lookup(td, ids.to(device))
    out.backward(TH.put(dy, device))
    return out.detach(), (slot if (slot is not None and device == "cuda") else td.grad)


@pytest.mark.parametrize("H", [8, 64, 768])
@pytest.mark.parametrize("vocab", [100, 2, 3, 4])
@pytest.mark.parametrize("device", DEVICES)
def test_embedding(device, vocab, H):
    """vocab 100: the general scatter; 2, 3, 4: the small-table kernels (two-pass through the wrapper, one-pass
    through ``mdtf_embed_bwd``).  n = 165: ten 16-token blocks and a ragged tail of 5 (two 64-token blocks and a tail
    of 37 for the one-pass form), and n = 1.  40 % of the tokens select one row; on the GPU two ids are out of range
    (``F.embedding`` raises on them on the CPU)."""
    device = _device(device)
    gpu = device == "cuda"
    for n in (165, 1):
        what = "%s/embed vocab=%d n=%d H=%d" % (device, vocab, n, H)
        table, ids, dy = TH.embed_inputs(vocab, n, H, 800 + vocab + H, gpu)
        out, dt = _embed_run(device, table, ids, dy)
        want = TH.embed_fwd_ref(table, ids)
        assert TH.bits_equal(out.cpu(), want.bfloat16() if gpu else want), what + ": the gather is not bitwise"
        TH.check_embed_bwd(dt, dy, ids, vocab, what + " dtable", bf16_out=gpu)
        slot0 = TH.randn((vocab, H), 31, 3.0)
        _, dt2 = _embed_run(device, table, ids, dy, slot=slot0.to(device).clone())
        TH.check_embed_bwd(dt2, dy, ids, vocab, what + " dtable slot", slot0=slot0)
        if not gpu:
            continue
        gt, gi = TH.Guarded(table.bfloat16(), device), TH.Guarded(ids, device)
        go = TH.Guarded(None, device, torch.bfloat16, (n, H))
        assert VC.call("mdtf_embed_fwd", VC._p(gt), VC._p(gi), VC._p(go), n, H, vocab) == 0
        TH.assert_contained(what + " raw fwd", [gt, gi], [go])
        assert TH.bits_equal(go.t, out)
        gdy = TH.Guarded(dy.bfloat16(), device)
        gd = TH.Guarded(slot0, device)
        assert VC.call("mdtf_embed_bwd", VC._p(gdy), VC._p(gi), VC._p(gd), n, H, vocab) == 0
        assert gd.guards_intact() and gdy.unchanged() and gi.unchanged(), what
        TH.check_embed_bwd(gd.t, dy, ids, vocab, what + " raw dtable", slot0=slot0)
        nws = int(VC.call_ws("mdtf_embed_bwd_ws_floats", n, H, vocab))
        assert nws == (-(-n // 16) * vocab * H if vocab <= 4 else 0), (what, nws)
        if nws:
            gd2, gws = TH.Guarded(slot0, device), TH.Guarded(None, device, torch.float32, (nws,))
            assert VC.call("mdtf_embed_bwd_ws", VC._p(gdy), VC._p(gi), VC._p(gd2), n, H, vocab, VC._p(gws)) == 0
            assert gd2.guards_intact() and gdy.unchanged() and gi.unchanged(), what
            TH.assert_contained(what + " raw ws", [], [gws])
            TH.check_embed_bwd(gd2.t, dy, ids, vocab, what + " raw dtable two-pass", slot0=slot0)


def _bert_run(device, word, pos, typ, ids, types, dy, slots=None):
    ts = [TH.put(t, device).requires_grad_(True) for t in (word, pos, typ)]
    if slots is not None:
        for t, s in zip(ts, slots):
            if device == "cuda":
                t._mdtf_var = _Var(s)
            else:
                t.grad = s
    if device == "cuda":
        out = T._BertEmbed.apply(ts[0], ts[1], ts[2], ids.to(device), types.to(device))     # the fused kernels
    else:
        out = T.bert_embeddings(ts[0], ts[1], ts[2], ids, types)
    out.backward(TH.put(dy, device))
    return out.detach(), [s if (slots is not None and device == "cuda") else t.grad
                          for t, s in zip(ts, slots or [None] * 3)]


def _check_bert(what, device, word, pos, typ, ids, types, dy, out, grads, slots0, bf16_grads):
    B, S = ids.shape
    npos, ntypes = pos.shape[0], typ.shape[0]
    ref, ab = TH.bert_fwd_ref(word, pos, typ, ids, types)
    # k = 2: the two adds of the three-term sum, rounded once
    TH.check(out, ref, TH.out_bound(ref, gamma(2) * ab, device == "cuda"), what + " out")
    s0 = slots0 or [None] * 3
    TH.check_embed_bwd(grads[0], dy, ids, word.shape[0], what + " dword", s0[0], bf16_grads)
    pos_ids = torch.arange(S)[None].expand(B, S)
    TH.check_embed_bwd(grads[1], dy, pos_ids, npos, what + " dpos", s0[1], bf16_grads)
    TH.check_embed_bwd(grads[2], dy, types, ntypes, what + " dtyp", s0[2], bf16_grads)
    prior = s0[1].double() if s0[1] is not None else torch.zeros(pos.shape, dtype=torch.float64)
    assert torch.equal(grads[1].detach().cpu().double()[S:], prior[S:]), what + ": position rows S.. changed"


@pytest.mark.parametrize("ntypes", [2, 4])
@pytest.mark.parametrize("B", [1, 8, 12])
@pytest.mark.parametrize("device", DEVICES)
def test_bert_embedding(device, B, ntypes):
    """word[ids] + pos[0..S) + typ[types], S = 24 of npos = 40; B = 1, 8 (one full batch block) and 12 (a second,
    half-filled one).  On the GPU a word id and two type ids are out of range (zero rows, nothing added back)."""
    device = _device(device)
    gpu = device == "cuda"
    S, npos, H, vocab = 24, 40, 72, 50
    what = "%s/bert_embed B=%d ntypes=%d" % (device, B, ntypes)
    word, pos, typ, ids, types, dy = TH.bert_inputs(B, S, H, vocab, npos, ntypes, 850 + B, gpu)
    out, grads = _bert_run(device, word, pos, typ, ids, types, dy)
    _check_bert(what, device, word, pos, typ, ids, types, dy, out, grads, None, gpu)
    slots0 = [TH.randn(t.shape, 41 + i, 3.0) for i, t in enumerate((word, pos, typ))]
    _, grads = _bert_run(device, word, pos, typ, ids, types, dy, [s.to(device).clone() for s in slots0])
    _check_bert(what + " slots", device, word, pos, typ, ids, types, dy, out, grads, slots0, False)
    if gpu:
        gin = [TH.Guarded(t.bfloat16(), device) for t in (word, pos, typ)] + [TH.Guarded(ids, device),
                                                                              TH.Guarded(types, device)]
        go = TH.Guarded(None, device, torch.bfloat16, (B, S, H))
        assert VC.call("mdtf_bert_embed_fwd", *([VC._p(t) for t in gin] + [VC._p(go), B * S, S, H, vocab, npos,
                                                                       ntypes])) == 0
        TH.assert_contained(what + " raw fwd", gin, [go])
        assert TH.bits_equal(go.t, out)
        gdy = TH.Guarded(dy.bfloat16(), device)
        gs = [TH.Guarded(s, device) for s in slots0]
        assert VC.call("mdtf_bert_embed_bwd", VC._p(gdy), VC._p(gin[3]), VC._p(gin[4]), VC._p(gs[0]), VC._p(gs[1]),
                       VC._p(gs[2]), B, S, H, vocab, ntypes) == 0
        assert all(g.guards_intact() for g in gs) and gdy.unchanged() and gin[3].unchanged() and gin[4].unchanged()
        _check_bert(what + " raw", device, word, pos, typ, ids, types, dy, go.t, [g.t for g in gs], slots0, False)


# ============================================================================================ codes and rows = 0
@pytest.mark.parametrize("device", GPU_ONLY)
def test_return_codes(device):
    """Shapes the kernels do not take are refused on the host, before any launch; the wrappers raise."""
    device = _device(device)
    z = torch.zeros(4 * 8200, dtype=torch.float32, device=device)
    p, null = VC._p(z), VC._p(None)
    ln_f = lambda H: VC.call("mdtf_ln_fwd", p, null, p, p, p, p, p, p, 1, H, 1e-12, 0.0, 0, null)      # noqa: E731
    ln_b = lambda H: VC.call("mdtf_ln_bwd", p, p, p, p, p, p, null, p, p, p, 1, H, 0.0, 0, null)      # noqa: E731
    assert ln_f(12) == MDTF_EINVAL and ln_b(12) == MDTF_EINVAL
    assert ln_f(8200) == MDTF_EUNSUPPORTED and ln_b(8200) == MDTF_EUNSUPPORTED
    assert VC.call("mdtf_softmax_fwd", p, null, p, 1, 12, 1.0, 1) == MDTF_EINVAL
    assert VC.call("mdtf_softmax_bwd", p, p, p, 1, 12, 1.0) == MDTF_EINVAL
    assert VC.call("mdtf_softmax_fwd", p, null, p, 1, 8200, 1.0, 1) == MDTF_EUNSUPPORTED
    assert VC.call("mdtf_softmax_bwd", p, p, p, 1, 8200, 1.0) == MDTF_EUNSUPPORTED
    assert VC.call("mdtf_embed_fwd", p, p, p, 1, 12, 4) == MDTF_EINVAL
    assert VC.call("mdtf_embed_bwd_ws", p, p, p, 1, 8, 5, p) == MDTF_EINVAL
    fwd = lambda S, H, npos, nt: VC.call("mdtf_bert_embed_fwd", p, p, p, p, p, p, S, S, H, 4, npos, nt)  # noqa: E731
    assert fwd(8, 8, 8, 5) != 0 and fwd(9, 8, 8, 2) != 0 and fwd(8, 12, 8, 2) != 0
    assert VC.call("mdtf_bert_embed_bwd", p, p, p, p, p, p, 1, 8, 8, 4, 5) != 0
    assert bool((z == 0).all())
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=device)                              # noqa: E731
    f32 = lambda *s: torch.ones(s, device=device)                                                    # noqa: E731
    with pytest.raises(RuntimeError, match="invalid argument"):
        T.layer_norm(bf(2, 12), f32(12), f32(12))
    with pytest.raises(RuntimeError, match="unsupported"):
        T.layer_norm(bf(2, 8200), f32(8200), f32(8200))
    with pytest.raises(TypeError):
        T.layer_norm(f32(2, 16), f32(16), f32(16))
    with pytest.raises(RuntimeError, match="invalid argument"):
        T.masked_softmax(bf(1, 1, 2, 12))
    with pytest.raises(RuntimeError, match="unsupported"):
        T.masked_softmax(bf(1, 1, 2, 8200))
    with pytest.raises(RuntimeError, match="invalid argument"):
        T.embedding_lookup(bf(4, 12), torch.zeros(3, dtype=torch.int64, device=device))
    ids = torch.zeros((2, 8), dtype=torch.int64, device=device)
    with pytest.raises(RuntimeError, match="unsupported"):
        T._BertEmbed.apply(bf(4, 8), bf(8, 8), bf(5, 8), ids, ids)
    with pytest.raises(RuntimeError, match="unsupported"):
        T._BertEmbed.apply(bf(4, 8), bf(6, 8), bf(2, 8), ids, ids)
    torch.cuda.synchronize()


@pytest.mark.parametrize("device", GPU_ONLY)
def test_rows_zero(device):
    """rows = 0: every entry point returns 0 without a launch (a grid of 0 blocks is a launch error) and leaves the
    guarded buffers as they were."""
    device = _device(device)
    H = 64
    e = torch.zeros((0, H))
    g, b = torch.ones(H), torch.zeros(H)
    VC.ln_fwd_raw("rows=0 ln_fwd", e, e, g, b)
    c = dict(dy=e, s=e, g=g, mean=torch.zeros(0), rstd=torch.zeros(0))
    VC.ln_bwd_raw("rows=0 ln_bwd", c, slots="prefilled")
    gx, gy = TH.Guarded(torch.zeros(8, dtype=torch.bfloat16), device), TH.Guarded(None, device, torch.bfloat16, (8,))
    assert VC.call("mdtf_softmax_fwd", VC._p(gx), VC._p(None), VC._p(gy), 0, 8, 1.0, 1) == 0
    assert VC.call("mdtf_softmax_bwd", VC._p(gx), VC._p(gx), VC._p(gy), 0, 8, 1.0) == 0
    assert gx.unchanged() and gy.unchanged()
    # the wrappers on an empty batch: empty outputs, zero parameter gradients (the workspace of no rows is empty)
    xd = torch.zeros((0, H), dtype=torch.bfloat16, device=device, requires_grad=True)
    gd, bd = g.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    y = T.layer_norm(xd, gd, bd, TH.EPS, residual=torch.zeros_like(xd))
    y.backward(torch.zeros_like(y))
    assert y.shape == (0, H) and xd.grad.shape == (0, H) and not bool(gd.grad.any()) and not bool(bd.grad.any())
    sd = torch.zeros((2, 1, 0, 8), dtype=torch.bfloat16, device=device, requires_grad=True)
    p = T.masked_softmax(sd, torch.zeros((2, 8), device=device), 0.5)
    p.backward(torch.zeros_like(p))
    assert p.shape == sd.shape and sd.grad.shape == sd.shape
    torch.cuda.synchronize()


@pytest.mark.parametrize("device", CPU_ONLY)
def test_ln_bwd_workspace_sizes(device):
    """``mdtf_ln_bwd_ws`` is host code: blocks * 2H floats; no rows: no workspace (this divided by zero)."""
    if not _native.available():
        pytest.skip("the kernel library is not built")
    assert VC.call_ws("mdtf_ln_bwd_ws", 0, 64) == 0
    if not any(k in os.environ for k in _ENV_KEYS):
        assert [VC.call_ws("mdtf_ln_bwd_ws", r, 64) // 128 for r in (1, 16, 17, 8192, 8197)] == [1, 1, 2, 512, 483]


# ========================================================================================= env-selected forms
SETTINGS = [{"MDTF_LN_BWD": "2", "MDTF_LN_NT": "1", "MDTF_EMBED_SMALL_2PASS": "0"},
            {"MDTF_LN_BWD": "3"},
            {"MDTF_LN_ATOMICS": "1", "MDTF_LN_BWD_RPB": "5"},
            {"MDTF_LN_BWD": "3", "MDTF_LN_ATOMICS": "1", "MDTF_LN_BWD_RPB": "40"}]
_ENV_KEYS = ("MDTF_LN_BWD", "MDTF_LN_BWD_RPB", "MDTF_LN_ATOMICS", "MDTF_LN_NT", "MDTF_EMBED_SMALL_2PASS")
_child_failed = []


def _check_compute(tag, got, default=None):
    """Every output of ``VC.compute()`` against the oracle; ``default``: the default form's outputs, for the two
    bitwise statements only."""
    assert len(got) >= len(VC.LN_H) * (1 + 5 * len(VC.SLOTS)) + len(VC.SMALL_EMBED)
    for H in VC.LN_H:
        rows = VC.ln_rows(H)
        c = VC.ln_raw_inputs(rows, H, 900 + H)
        keep = TH.hash_keep(VC.SEED, rows * H, VC.P_DROP).view(rows, H)
        fref = TH.ln_fwd_ref(c["x"], c["res"], c["g"], c["b"], keep, VC.P_DROP)
        fb = TH.ln_fwd_bounds(fref, c["g"], c["b"], "cuda")
        TH.check(got["fwd/%d/s" % H], fref["s"], fb["s"], "%s/ln_fwd H=%d s" % (tag, H))
        if default is not None:
            assert TH.bits_equal(got["fwd/%d/s" % H], default["fwd/%d/s" % H]), (tag, H)
        for slots in VC.SLOTS:
            k = "bwd/%d/%s/" % (H, slots)
            _, _, _, dg0, db0 = VC.make_slots(slots, H, "cpu")
            r = dict(dx=got[k + "dx"], dxb=got[k + "dxb"], dgamma=got[k + "dgamma"], dbeta=got[k + "dbeta"],
                     dg0=dg0 if slots == "prefilled" else None, db0=db0 if slots == "prefilled" else None,
                     blocks=int(got[k + "blocks"]))
            _check_ln_bwd_raw("%s/ln_bwd H=%d %s" % (tag, H, slots), c, r, VC.P_DROP, VC.SEED)
            if default is not None and H > 2048:
                # past four vectors per lane every MDTF_LN_BWD runs ln_bwd_kernel, whose dx does not depend on the
                # block geometry
                assert TH.bits_equal(got[k + "dx"], default[k + "dx"]), (tag, H, slots)
    for vocab, n, H in VC.SMALL_EMBED:
        _, ids, dy = TH.embed_inputs(vocab, n, H, 950 + vocab, True)
        TH.check_embed_bwd(got["embed/%d/%d/%d" % (vocab, n, H)], dy, ids, vocab,
                           "%s/embed_small vocab=%d n=%d H=%d" % (tag, vocab, n, H), bf16_out=True)


_default = {}


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=["lean_nt_1pass", "lean_pf", "atomics_rpb5",
                                                               "lean_pf_atomics_rpb40"])
@pytest.mark.parametrize("device", GPU_ONLY)
def test_env_selected_forms(device, setting, tmp_path):
    """The switches are read once per process, so each setting runs ``transformer_variant_child.py`` in a fresh child
    (one at a time, under a time limit); after a child that does not exit 0 the remaining settings are skipped."""
    _device(device)
    if _child_failed:
        pytest.skip("an earlier child failed: %r" % (_child_failed[0],))
    assert not any(k in os.environ for k in _ENV_KEYS), "the parent must run the default forms"
    if not _default:
        _default.update(VC.compute())
        _check_compute("default", _default)
    env = dict(os.environ)
    env.update(SETTINGS[setting])
    out = str(tmp_path / "variant.pt")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(VC.__file__), out], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _child_failed.append(SETTINGS[setting])
        raise
    if r.returncode != 0:
        _child_failed.append(SETTINGS[setting])
    assert r.returncode == 0, "child %r exited %d:\n%s" % (SETTINGS[setting], r.returncode, r.stdout[-4000:])
    tag = "+".join("%s=%s" % (k[5:], v) for k, v in sorted(SETTINGS[setting].items()))
    _check_compute(tag, torch.load(out), _default)


# ============================================================================ the checks must be able to fail
def _ulps(t, n):
    """A bf16 tensor's first element moved by n bf16 steps away from zero."""
    t = t.clone()
    t.view(torch.int16).view(-1)[0] += n
    return t


@pytest.mark.parametrize("device", CPU_ONLY)
def test_check_fails_on_ln_forward_faults(device):
    """Two bf16 steps on one element, the last 8-column vector of a row zeroed, one row's mean off by 1e-3 |mean|."""
    rows, H = 5, 72
    x, res, g, b, dy = TH.ln_inputs(rows, H, 11, True)
    fref = TH.ln_fwd_ref(x, res, g, b)
    fb = TH.ln_fwd_bounds(fref, g, b, "cuda")
    y = TH.round_bf16(fref["y"]).bfloat16()
    s = TH.round_bf16(fref["s"]).bfloat16()
    mean = fref["mean"].float()
    TH.check(y, fref["y"], fb["y"], "perturb/y intact")
    TH.check(s, fref["s"], fb["s"], "perturb/s intact")
    TH.check(mean, fref["mean"], fb["mean"], "perturb/mean intact")
    with pytest.raises(AssertionError):
        TH.check(_ulps(y, 2), fref["y"], fb["y"], "perturb/y two ulps")
    with pytest.raises(AssertionError):
        TH.check(_ulps(s, 2), fref["s"], fb["s"], "perturb/s two ulps")
    y2 = y.clone()
    y2[3, -8:] = 0.0
    with pytest.raises(AssertionError):
        TH.check(y2, fref["y"], fb["y"], "perturb/y last vector")
    m2 = mean.clone()
    m2[2] += 1e-3 * m2[2].abs()
    with pytest.raises(AssertionError):
        TH.check(m2, fref["mean"], fb["mean"], "perturb/mean")


@pytest.mark.parametrize("device", CPU_ONLY)
def test_check_fails_on_ln_backward_faults(device):
    """dgamma without one row's contribution; [dgamma | dbeta] swapped; dx two bf16 steps off, last vector zeroed."""
    rows, H = 37, 72
    c = VC.ln_raw_inputs(rows, H, 12)
    ref = TH.ln_bwd_ref(c["dy"], c["s"], c["mean"], c["rstd"], c["g"])
    r = dict(dx=TH.round_bf16(ref["dx"]).bfloat16(), dxb=None, dgamma=ref["dgamma"].float(),
             dbeta=ref["dbeta"].float(), dg0=None, db0=None, blocks=3)
    _check_ln_bwd_raw("perturb/ln_bwd intact", c, r, 0.0, 0)
    one = (c["dy"][5].double() * ref["xh"][5]).float()
    for name, bad in (("dgamma row", dict(r, dgamma=r["dgamma"] - one)),
                      ("swapped", dict(r, dgamma=r["dbeta"], dbeta=r["dgamma"])),
                      ("dx two ulps", dict(r, dx=_ulps(r["dx"], 2)))):
        with pytest.raises(AssertionError):
            _check_ln_bwd_raw("perturb/ln_bwd " + name, c, bad, 0.0, 0)
    dx2 = r["dx"].clone()
    dx2[36, -8:] = 0.0
    with pytest.raises(AssertionError):
        _check_ln_bwd_raw("perturb/ln_bwd last vector", c, dict(r, dx=dx2), 0.0, 0)


@pytest.mark.parametrize("device", CPU_ONLY)
def test_check_fails_on_softmax_and_embedding_faults(device):
    """A softmax row normalised over cols - 8 keys; one unselected table row non-zero; a gather off by two steps."""
    cols = 40
    x, mask, dy = TH.softmax_inputs(3, 3, 5, cols, 13, "sparse")
    y, dx = _softmax_run("cpu", x, mask, 0.125, dy)
    _check_softmax("perturb/softmax intact", "cpu", x, mask, 0.125, dy, y, dx)
    y2 = y.clone()
    z = x[1, 1, 1] * 0.125 + mask[1]
    y2[1, 1, 1] = torch.exp(z - z.max()) / torch.exp(z - z.max())[:cols - 8].sum()
    with pytest.raises(AssertionError):
        _check_softmax("perturb/softmax short row", "cpu", x, mask, 0.125, dy, y2, dx)
    with pytest.raises(AssertionError):
        _check_softmax("perturb/softmax dx", "cpu", x, mask, 0.125, dy, y, _ulps(dx.bfloat16(), 2).float(), saved=y)
    table, ids, dyt = TH.embed_inputs(100, 165, 8, 14, False)
    assert not bool((ids == 3).any())
    _, dt = _embed_run("cpu", table, ids, dyt)
    TH.check_embed_bwd(dt, dyt, ids, 100, "perturb/embed intact")
    dt2 = dt.clone()
    dt2[3, 5] = 1e-30
    with pytest.raises(AssertionError):
        TH.check_embed_bwd(dt2, dyt, ids, 100, "perturb/embed idle row")
    dt3 = dt.clone()
    hot = int(ids[torch.nonzero(ids == 1)[0]]) if bool((ids == 1).any()) else int(ids[0])
    dt3[hot] -= dyt[int(torch.nonzero(ids == hot)[0])]
    with pytest.raises(AssertionError):
        TH.check_embed_bwd(dt3, dyt, ids, 100, "perturb/embed missing addend")
