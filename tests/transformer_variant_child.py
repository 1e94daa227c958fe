"""Body of ``test_transformer_kernels.py::test_env_selected_forms`` (not collected as a test), and the raw-entry-point
runners that file shares with it.

``compute()`` runs the cases whose code path depends on ``MDTF_LN_BWD``, ``MDTF_LN_BWD_RPB``, ``MDTF_LN_ATOMICS``,
``MDTF_LN_NT`` (read once per process by the kernel library) and ``MDTF_EMBED_SMALL_2PASS`` (read when
``mdtf.ops.transformer`` is imported) on the GPU and returns every output on the CPU: the LayerNorm forward's saved
``s``, the raw LayerNorm backward at every H of ``LN_H`` with dropout in each gradient-slot arrangement, and the
small-table embedding backward.  Run as a script it saves them to ``argv[1]``; the test starts it as a fresh process
per setting and checks the outputs against the same oracle and bounds as the default form's.
"""
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# one H per template LN_DISPATCH instantiates: <1,64> one live lane, nine lanes | <1,32> | <1,64> full | <2,64> one
# lane in the second vector | <3,32> | <4,64> a half-filled third vector and an empty fourth, full | <8,64> (past
# the lean form's limit) | <16,64>
LN_H = [8, 72, 256, 512, 520, 768, 1280, 2048, 2056, 8192]
SLOTS = ["separate", "gamma_beta", "beta_gamma", "prefilled"]
P_DROP, SEED = 0.1, 0x5EED5
SMALL_EMBED = [(2, 165, 64), (3, 165, 768), (4, 165, 8), (4, 1, 64)]        # (vocab, n, H)


def ln_rows(H):
    return 9 if H == 8192 else 37


def ln_raw_inputs(rows, H, seed):
    """What the raw backward reads: s (bf16-representable), mean and rstd (the fp32 roundings of the fp64 statistics
    of that s), gamma, dy; and x, res, beta for the forward."""
    import transformer_helpers as TH
    x, res, g, b, dy = TH.ln_inputs(rows, H, seed, True)
    s = TH.bf16_exact(x + res)
    ref = TH.ln_fwd_ref(s, None, g, b)
    return dict(x=x, res=res, g=g, b=b, dy=dy, s=s, mean=ref["mean"].float(), rstd=ref["rstd"].float())


def _p(g):
    from mdtf.ops import _native
    return _native.ptr(g.t if hasattr(g, "guards_intact") else g)


def call(name, *args):
    """A registered entry point called the way ``ops/transformer.py`` calls it; returns its code."""
    from mdtf.ops import _native
    from mdtf.ops import transformer  # noqa: F401  (registers the signatures)
    rc = _native.fn(name)(*args, _native.stream_ptr())
    torch.cuda.synchronize()
    return rc


def ln_fwd_raw(what, x, res, g, b, p=0.0, seed=0, eps=None):
    """mdtf_ln_fwd on guarded buffers: y, s (bf16), mean, rstd (fp32)."""
    import transformer_helpers as TH
    rows, H = x.shape
    gx = TH.Guarded(x.bfloat16(), "cuda")
    gr = TH.Guarded(res.bfloat16(), "cuda") if res is not None else None
    gg, gb = TH.Guarded(g, "cuda"), TH.Guarded(b, "cuda")
    gy, gs = (TH.Guarded(None, "cuda", torch.bfloat16, (rows, H)) for _ in range(2))
    gm, grs = (TH.Guarded(None, "cuda", torch.float32, (rows,)) for _ in range(2))
    rc = call("mdtf_ln_fwd", _p(gx), _p(gr), _p(gg), _p(gb), _p(gy), _p(gs), _p(gm), _p(grs), rows, H,
              TH.EPS if eps is None else eps, float(p), seed, _p(None))
    assert rc == 0, (what, rc)
    TH.assert_contained(what, [gx, gg, gb] + ([gr] if gr else []), [gy, gs, gm, grs] if rows else [])
    if not rows:
        assert all(o.unchanged() for o in (gy, gs, gm, grs)), what + ": rows = 0 wrote something"
    return dict(y=gy.t, s=gs.t, mean=gm.t, rstd=grs.t)


def make_slots(kind, H, device="cuda"):
    """(holder, dgamma view, dbeta view, prior dgamma, prior dbeta) of a gradient-slot arrangement; the holder is a
    list of Guarded buffers on the device, of plain tensors on the CPU."""
    import transformer_helpers as TH
    pre = TH.randn((2 * H,), 77, 3.0) if kind == "prefilled" else torch.zeros(2 * H)
    if device == "cpu":
        flat = pre.clone()
        a, b = (flat[H:], flat[:H]) if kind == "beta_gamma" else (flat[:H], flat[H:])
        swap = kind == "beta_gamma"
        return [flat], a, b, (pre[H:] if swap else pre[:H]), (pre[:H] if swap else pre[H:])
    if kind in ("gamma_beta", "beta_gamma"):
        flat = TH.Guarded(pre, device)
        a, b = (flat.t[H:], flat.t[:H]) if kind == "beta_gamma" else (flat.t[:H], flat.t[H:])
        return [flat], a, b, torch.zeros(H), torch.zeros(H)
    ga, gb = TH.Guarded(pre[:H], device), TH.Guarded(pre[H:], device)
    assert ga.t.data_ptr() + 4 * H != gb.t.data_ptr() and gb.t.data_ptr() + 4 * H != ga.t.data_ptr()
    return [ga, gb], ga.t, gb.t, pre[:H], pre[H:]


def ln_bwd_raw(what, c, p=0.0, seed=0, slots="separate", ws_written=True):
    """mdtf_ln_bwd on guarded buffers from the inputs ``c`` of ``ln_raw_inputs``: dx, dx_branch (with p), dgamma,
    dbeta, and the number of blocks the workspace was sized for."""
    import transformer_helpers as TH
    rows, H = c["s"].shape
    gdy, gs = TH.Guarded(c["dy"].bfloat16(), "cuda"), TH.Guarded(c["s"].bfloat16(), "cuda")
    gg, gm, grs = TH.Guarded(c["g"], "cuda"), TH.Guarded(c["mean"], "cuda"), TH.Guarded(c["rstd"], "cuda")
    gdx = TH.Guarded(None, "cuda", torch.bfloat16, (rows, H))
    gdxb = TH.Guarded(None, "cuda", torch.bfloat16, (rows, H)) if p else None
    holders, dg, db, dg0, db0 = make_slots(slots, H)
    nws = int(call_ws("mdtf_ln_bwd_ws", rows, H))
    assert nws % (2 * H) == 0 and nws >= (2 * H if rows else 0), (what, nws)
    gws = TH.Guarded(None, "cuda", torch.float32, (max(nws, 4),))
    rc = call("mdtf_ln_bwd", _p(gdy), _p(gs), _p(gg), _p(gm), _p(grs), _p(gdx), _p(gdxb), _p(dg), _p(db), _p(gws),
              rows, H, float(p), seed, _p(None))
    assert rc == 0, (what, rc)
    outs = [gdx] + ([gdxb] if gdxb else [])
    TH.assert_contained(what, [gdy, gs, gg, gm, grs], outs if rows else [])
    assert gws.guards_intact() and all(h.guards_intact() for h in holders), what + ": wrote outside a slot or ws"
    if rows and ws_written:
        assert gws.all_written(), what + ": a workspace element no block stored"
    if not rows:
        assert all(o.unchanged() for o in outs + holders + [gws]), what + ": rows = 0 wrote something"
    return dict(dx=gdx.t, dxb=gdxb.t if gdxb else None, dgamma=dg, dbeta=db, dg0=dg0, db0=db0,
                blocks=nws // (2 * H))


def call_ws(name, *args):
    from mdtf.ops import _native
    from mdtf.ops import transformer  # noqa: F401
    return _native.fn(name)(*args)


def embed_small_bwd(vocab, n, H, seed):
    """The table gradient of ``embedding_lookup`` for a small table through the autograd wrapper (bf16)."""
    import transformer_helpers as TH
    from mdtf.ops import transformer as T
    table, ids, dy = TH.embed_inputs(vocab, n, H, seed, True)
    td = table.cuda().bfloat16().requires_grad_(True)
    T.embedding_lookup(td, ids.cuda()).backward(dy.cuda().bfloat16())
    return td.grad


def atomics():
    return os.environ.get("MDTF_LN_ATOMICS", "0")[:1] == "1"


def compute():
    from mdtf.ops import _native
    _native.lib()
    assert _native.mode() != "torch" and not _native.deterministic()
    out = {}
    for H in LN_H:
        c = ln_raw_inputs(ln_rows(H), H, 900 + H)
        f = ln_fwd_raw("child fwd H=%d" % H, c["x"], c["res"], c["g"], c["b"], P_DROP, SEED)
        out["fwd/%d/s" % H] = f["s"].cpu()
        for slots in SLOTS:
            r = ln_bwd_raw("child bwd H=%d %s" % (H, slots), c, P_DROP, SEED, slots, ws_written=not atomics())
            for k in ("dx", "dxb", "dgamma", "dbeta"):
                out["bwd/%d/%s/%s" % (H, slots, k)] = r[k].cpu().clone()
            out["bwd/%d/%s/blocks" % (H, slots)] = torch.tensor(r["blocks"])
    for vocab, n, H in SMALL_EMBED:
        out["embed/%d/%d/%d" % (vocab, n, H)] = embed_small_bwd(vocab, n, H, 950 + vocab).cpu()
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    torch.save(compute(), sys.argv[1])
