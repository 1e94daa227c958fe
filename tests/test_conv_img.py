"""csrc/conv_img.hip: the image-resident 3x3 / stride 1 / pad 1 kernel for 28x28x128 and 14x14x256, elementwise
against the same conv in fp64 on the CPU (from the bf16-rounded operands).

The kernel is chosen inside ``mdtf_conv_fwd_v2`` / ``mdtf_conv_dgrad_v2``; the tests force every (shape, pass)
on with the process-wide mask and check the routing, so they exercise it whatever the default mask is.

Bounds (derived, not tuned), with u = 2^-24 (fp32 unit roundoff), K = 9 C products per output and
S = the same conv of |x| and |w| (>= |any partial sum|):

* Output.  The fp32 accumulation of K exact bf16 x bf16 products, in any order, is within K u S of the exact
  sum (first order); one bf16 rounding adds 2^-9 |ref| (half an ulp of 8 significand bits is 2^-9 relative).
  Factor 2 covers the higher-order terms and the rounding acting on the perturbed value:
  ``|out - ref| <= 2 (2^-9 |ref| + K u S)``, every element.
* Sums over the R = N H W rows of a channel.  Each summand carries the accumulation error <= K u S; adding R
  fp32 numbers in any order (lane partials, DPP, LDS and global atomics) adds <= R u sum|y| <= R u sum S.  So
  ``|sum - ref| <= 2 (K + R) u sum S``.
* Squared / product sums.  y^2 - ref^2 = (y - ref)(y + ref): <= 2 max|y| K u S per row; y x likewise with
  max|x|; the product's own rounding and the R additions add (R + 1) u max|.| sum S.  (2 K + R + 1) <= 2 (K + R)
  for R >= 1, so the limit is the same with S max|.|: ``2 (K + R) u max|.| sum S``.
  The BN-backward sums are taken from the gradient as stored (bf16); its rounding errors (2^-9 relative, of
  either sign) are not in the limit.  The inputs are drawn (plain normal, fixed seeds) so that today's
  conv_fd_v2 on the same tensors meets every limit too, and the tests assert that.
"""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
# (H = W, C) -> the conv_fd_v2 tile the training step runs these convs with: (bm, bn, stages, ver) forward, data
# gradient (conv_fd_v2<128,128,0,true,2,4> / <64,128,1,false,2,4>, <256,256,0,true,32,8> / <256,256,1,false,2,8>)
SHAPES = {(28, 128): ((128, 128, 2, 2), (64, 128, 2, 2)), (14, 256): ((256, 256, 32, 3), (256, 256, 2, 3))}
PADS = (1, 1, 1, 1)
CASES = [(n, hw, c) for (hw, c) in SHAPES for n in (1, 3)]


@pytest.fixture(autouse=True)
def _img_mask():
    from mdtf.ops import conv as C
    C.set_conv_img_mask(15)
    yield
    C.set_conv_img_mask(-1)


def _conv64(x, w):
    """NHWC x, HWIO w (float64) -> NHWC y, 3x3 / stride 1 / pad 1."""
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)


def _dgrad_filter(w):
    """The data gradient is the conv with the flipped filter, channels transposed."""
    return w.flip(0, 1).permute(0, 1, 3, 2)


@functools.lru_cache(maxsize=None)
def _case(n, hw, c):
    """Operands (bf16, CPU) and the fp64 references of one shape, computed once and left unchanged."""
    g = torch.Generator().manual_seed(1000 * n + hw + c)
    x = torch.randn(n, hw, hw, c, generator=g).bfloat16()
    dy = torch.randn(n, hw, hw, c, generator=g).bfloat16()
    bx = torch.randn(n, hw, hw, c, generator=g).bfloat16()
    w = (torch.randn(3, 3, c, c, generator=g) / (9 * c) ** 0.5).bfloat16()
    mbits = torch.rand(n * hw * hw * c, generator=g) > 0.4
    packed = (mbits.view(-1, 8).to(torch.int32) << torch.arange(8)).sum(1).to(torch.uint8)
    x64, dy64, w64 = x.double(), dy.double(), w.double()
    return {
        "x": x, "dy": dy, "bx": bx, "w": w, "mbits": mbits.view(n, hw, hw, c), "packed": packed,
        "y": _conv64(x64, w64), "ys": _conv64(x64.abs(), w64.abs()),
        "dx": _conv64(dy64, _dgrad_filter(w64)), "dxs": _conv64(dy64.abs(), _dgrad_filter(w64.abs())),
    }


def _check_out(out, ref, s, k, what):
    err = (out.double().cpu() - ref).abs()
    lim = 2 * (2.0 ** -9 * ref.abs() + k * U24 * s)
    worst = (err / lim).max().item()
    print("%s: max |out - ref| / limit = %.3f" % (what, worst))
    assert worst <= 1.0, what


def _check_sums(psum, psq, ref1, ref2, s, mx, k, what):
    """psum / psq [slots][C] partial rows; ref1 / ref2 [R][C] fp64 summands; s [R][C]; mx: max|.| of the second
    factor per channel (or a scalar)."""
    r = ref1.shape[0]
    lim1 = 2 * (k + r) * U24 * s.sum(0)
    lim2 = lim1 * mx
    e1 = ((psum.double().sum(0).cpu() - ref1.sum(0)).abs() / lim1).max().item()
    e2 = ((psq.double().sum(0).cpu() - ref2.sum(0)).abs() / lim2).max().item()
    print("%s: sum error / limit = %.3f, second sum error / limit = %.3f" % (what, e1, e2))
    assert e1 <= 1.0 and e2 <= 1.0, what


def _fwd(t, hw, c, stats):
    from mdtf.ops import conv as C
    bm, bn, stages, ver = SHAPES[(hw, c)][0]
    return C.mdtf_fwd(t["x"].to(DEV), t["w"].to(DEV), (hw, hw), (1, 1), PADS, (1, 1), bm, bn, stats=stats, ver=ver,
                      stages=stages)


def _dgrad(t, hw, c, **kw):
    from mdtf.ops import conv as C
    bm, bn, stages, ver = SHAPES[(hw, c)][1]
    return C.mdtf_dgrad(t["dy"].to(DEV), t["w"].to(DEV), tuple(t["dy"].shape), (1, 1), PADS, (1, 1), bm, bn, ver=ver,
                        stages=stages, **kw)


def _both_paths(run):
    """run() on the new kernel, then on conv_fd_v2 (mask 0): the reference path must meet the same limits."""
    from mdtf.ops import conv as C
    for mask, name in ((15, "conv3_img"), (0, "conv_fd_v2")):
        C.set_conv_img_mask(mask)
        run(name)
    C.set_conv_img_mask(15)


@pytest.mark.parametrize("n,hw,c", CASES)
def test_forward(n, hw, c):
    """Plain store and the forward BN-statistics epilogue (statistics rows at any slot: 5 slots, odd grid)."""
    from mdtf.ops import conv as C
    assert C.conv_img_routed(hw, hw, c, False)
    t = _case(n, hw, c)
    k = 9 * c

    def run(name):
        _check_out(_fwd(t, hw, c, None), t["y"], t["ys"], k, "%s fwd plain" % name)
        sbuf = torch.zeros(2, 5, c, device=DEV)
        y = _fwd(t, hw, c, (sbuf[0], sbuf[1]))
        _check_out(y, t["y"], t["ys"], k, "%s fwd stats" % name)
        yr = t["y"].reshape(-1, c)
        _check_sums(sbuf[0], sbuf[1], yr, yr * yr, t["ys"].reshape(-1, c), yr.abs().max(0).values, k,
                    "%s fwd stats" % name)

    _both_paths(run)


@pytest.mark.parametrize("n,hw,c", CASES)
def test_dgrad(n, hw, c):
    """Plain store and the BN-backward statistics (sum g m, sum g m x) with and without a ReLU mask."""
    from mdtf.ops import conv as C
    assert C.conv_img_routed(hw, hw, c, True)
    t = _case(n, hw, c)
    k = 9 * c

    def run(name):
        _check_out(_dgrad(t, hw, c), t["dx"], t["dxs"], k, "%s dgrad plain" % name)
        for masked in (True, False):
            bsum = torch.zeros(2, 4, c, device=DEV)
            dx = _dgrad(t, hw, c, bn_stats=(t["bx"].to(DEV), t["packed"].to(DEV) if masked else None, bsum[0],
                                            bsum[1], 4))
            _check_out(dx, t["dx"], t["dxs"], k, "%s dgrad bstat" % name)
            m = t["mbits"].double() if masked else torch.ones_like(t["dx"])
            gm = (t["dx"] * m).reshape(-1, c)
            bx = t["bx"].double().reshape(-1, c)
            _check_sums(bsum[0], bsum[1], gm, gm * bx, (t["dxs"] * m).reshape(-1, c), bx.abs().max(0).values, k,
                        "%s dgrad bstat mask=%s" % (name, masked))

    _both_paths(run)


def test_fallbacks():
    """Requests outside the kernel stay on conv_fd_v2 and stay correct: accumulate, a 15-wide image, mask 0."""
    from mdtf.ops import conv as C
    n, hw, c = 1, 14, 256
    t = _case(n, hw, c)
    k = 9 * c
    # accumulate = 1: out += dgrad (one more bf16 rounding of the sum: compare the difference in fp64)
    base = torch.randn(n, hw, hw, c, generator=torch.Generator().manual_seed(7)).bfloat16()
    out = base.to(DEV).clone()
    _dgrad(t, hw, c, out=out, accumulate=True)
    ref = t["dx"] + base.double()
    err = (out.double().cpu() - ref).abs()
    lim = 2 * (2.0 ** -9 * (ref.abs() + t["dx"].abs()) + k * U24 * t["dxs"])   # + the rounding of dgrad itself
    assert (err <= lim).all()
    # 15 x 15: not an instance
    assert not C.conv_img_routed(15, 15, c, False)
    g = torch.Generator().manual_seed(15)
    x = torch.randn(1, 15, 15, c, generator=g).bfloat16()
    y = C.mdtf_fwd(x.to(DEV), t["w"].to(DEV), (15, 15), (1, 1), PADS, (1, 1), 256, 256, ver=3, stages=2)
    _check_out(y, _conv64(x.double(), t["w"].double()), _conv64(x.double().abs(), t["w"].double().abs()), k, "15 wide")
    # mask 0 (MDTF_CONV_IMG=0)
    C.set_conv_img_mask(0)
    assert not C.conv_img_routed(hw, hw, c, False) and not C.conv_img_routed(28, 28, 128, True)
    _check_out(_fwd(t, hw, c, None), t["y"], t["ys"], k, "mask 0 fwd")
    _check_out(_dgrad(t, hw, c), t["dx"], t["dxs"], k, "mask 0 dgrad")


@pytest.mark.parametrize("hw,c", list(SHAPES))
def test_deterministic_and_graph_replay(hw, c):
    """Two launches give bitwise-equal outputs (the statistics may differ by atomics order); a captured and
    replayed launch equals an eager one."""
    t = _case(3, hw, c)
    sbuf = torch.zeros(2, 5, c, device=DEV)
    y0, y1 = _fwd(t, hw, c, (sbuf[0], sbuf[1])), _fwd(t, hw, c, (sbuf[0], sbuf[1]))
    d0, d1 = _dgrad(t, hw, c), _dgrad(t, hw, c)
    assert torch.equal(y0, y1) and torch.equal(d0, d1)
    x, w, dy = t["x"].to(DEV), t["w"].to(DEV), t["dy"].to(DEV)
    from mdtf.ops import conv as C
    (fbm, fbn, fst, fver), (dbm, dbn, dst, dver) = SHAPES[(hw, c)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg = C.mdtf_fwd(x, w, (hw, hw), (1, 1), PADS, (1, 1), fbm, fbn, ver=fver, stages=fst)
        dg = C.mdtf_dgrad(dy, w, tuple(dy.shape), (1, 1), PADS, (1, 1), dbm, dbn, ver=dver, stages=dst)
    yg.zero_()
    dg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y0) and torch.equal(dg, d0)


@pytest.mark.parametrize("hw,c", list(SHAPES))
def test_routing_is_observed(hw, c):
    """The entry points really launch conv3_img for these geometries: its block b adds its statistics into row
    b % slots, and block 0 owns the first 14 output rows of image 0.  So with at least as many rows as blocks, row 0
    holds the sums over exactly those 14 W pixels and the rows past the grid stay zero; conv_fd_v2's row 0 holds
    its first M tile (128 or 256 pixels) instead, which the same limit rejects."""
    from mdtf.ops import conv as C
    n, k, slots = 3, 9 * c, 8
    t = _case(n, hw, c)
    blocks = n * hw // 14
    mine = slice(0, 14)                                      # image 0, output rows 0 .. 13

    def row0_err(psum, ref, s):
        r = ref[0, mine].reshape(-1, c)
        lim = 2 * (k + r.shape[0]) * U24 * s[0, mine].reshape(-1, c).sum(0)
        return ((psum[0].double().cpu() - r.sum(0)).abs() / lim).max().item()

    for dgrad in (False, True):
        errs = {}
        for mask in (15, 0):
            C.set_conv_img_mask(mask)
            buf = torch.zeros(2, slots, c, device=DEV)
            if dgrad:
                _dgrad(t, hw, c, bn_stats=(t["bx"].to(DEV), None, buf[0], buf[1], slots))
                errs[mask] = row0_err(buf[0], t["dx"], t["dxs"])
            else:
                _fwd(t, hw, c, (buf[0], buf[1]))
                errs[mask] = row0_err(buf[0], t["y"], t["ys"])
            if mask == 15:
                used = (buf[0] != 0).any(1).cpu().tolist()
                assert used == [b < blocks for b in range(slots)], (dgrad, used)
        C.set_conv_img_mask(15)
        print("row 0 error / limit: conv3_img %.3f, conv_fd_v2 %.1f" % (errs[15], errs[0]))
        assert errs[15] <= 1.0 < errs[0], (dgrad, errs)


@pytest.mark.parametrize("n,hw,c", CASES)
def test_statistics_count_every_pixel_once(n, hw, c):
    """Exact check of which pixels the statistics epilogues count.  With x = 1, dy = 1 and every filter element
    2^-12 each output is m C 2^-12 with m = 4, 6 or 9 taps inside the image: a 4-bit integer times a power of two,
    exact in fp32 and in bf16.  Its square is m^2 <= 81 times a power of two, its product with bx (integers in
    [-2, 2]) at most 18 times one, and any sum of up to 2352 such terms is an integer below 2^18 times that power:
    exact in fp32 in every order of addition.  So the sums must EQUAL the fp64 sums; one pixel dropped or counted
    twice changes sum y by at least 4 C 2^-12."""
    ones = torch.ones(n, hw, hw, c).bfloat16()
    w = torch.full((3, 3, c, c), 2.0 ** -12).bfloat16()
    g = torch.Generator().manual_seed(n + hw)
    bx = torch.randint(-2, 3, (n, hw, hw, c), generator=g).bfloat16()
    mbits = torch.rand(n * hw * hw * c, generator=g) > 0.4
    packed = (mbits.view(-1, 8).to(torch.int32) << torch.arange(8)).sum(1).to(torch.uint8)
    t = {"x": ones, "dy": ones, "w": w}
    y = _conv64(ones.double(), w.double()).reshape(-1, c)    # the filter is symmetric: dx == y
    sbuf = torch.zeros(2, 5, c, device=DEV)
    out = _fwd(t, hw, c, (sbuf[0], sbuf[1]))
    assert torch.equal(out.double().cpu().reshape(-1, c), y)
    assert torch.equal(sbuf[0].double().sum(0).cpu(), y.sum(0))
    assert torch.equal(sbuf[1].double().sum(0).cpu(), (y * y).sum(0))
    bsum = torch.zeros(2, 4, c, device=DEV)
    dx = _dgrad(t, hw, c, bn_stats=(bx.to(DEV), packed.to(DEV), bsum[0], bsum[1], 4))
    assert torch.equal(dx.double().cpu().reshape(-1, c), y)
    gm = y * mbits.view(-1, c).double()
    assert torch.equal(bsum[0].double().sum(0).cpu(), gm.sum(0))
    assert torch.equal(bsum[1].double().sum(0).cpu(), (gm * bx.double().reshape(-1, c)).sum(0))


@pytest.mark.parametrize("env,mask", [("0", 0), ("1", 1), (None, None)])
def test_environment_mask(env, mask):
    """MDTF_CONV_IMG is read once per process as a bit mask: 0 = conv_fd_v2 everywhere, 1 = only the 28x28x128
    forward (not "everything on"), unset = the built-in default, which the override of the other tests leaves
    alone.  A fresh process each, since the value is cached."""
    import subprocess
    code = ("import torch\nfrom mdtf.ops import conv as C\n"
            "print('MASK', C.conv_img_mask(), int(C.conv_img_routed(28, 28, 128, False)), "
            "int(C.conv_img_routed(28, 28, 128, True)), int(C.conv_img_routed(14, 14, 256, False)), "
            "int(C.conv_img_routed(14, 14, 256, True)))\n")
    e = dict(os.environ)
    e.pop("MDTF_CONV_IMG", None)
    if env is not None:
        e["MDTF_CONV_IMG"] = env
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-400:]
    got = [int(v) for v in out.stdout.split("MASK")[1].split()]
    if mask is None:
        from mdtf.ops import conv as C
        C.set_conv_img_mask(-1)
        mask = C.conv_img_mask()                             # this process runs without the variable's override
        C.set_conv_img_mask(15)
    assert got == [mask] + [(mask >> b) & 1 for b in range(4)], (env, got)
