"""Graph-timed 3x3 convolutions of ResNet-50 stages 2 and 3 (batch 256; 28 x 28 x 128 and 14 x 14 x 256): the
image-resident kernel (csrc/conv_img.hip) vs the conv_fd_v2 tiles the step runs, forward with the BN-statistics
epilogue and data gradient with the BN-backward statistics, alternating in one process.  One JSON line per round
and a median summary."""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench.gemm_pp_probe import gtime  # noqa: E402
from mdtf.ops import _native as N  # noqa: E402
from mdtf.ops import conv as C  # noqa: E402

# (H = W, C) -> the step's conv_fd_v2 tiles: (bm, bn, stages, ver) forward, data gradient
SHAPES = {(28, 128): ((128, 128, 2, 2), (64, 128, 2, 2)), (14, 256): ((256, 256, 32, 3), (256, 256, 2, 3))}


def main():
    n = int(os.environ.get("B", "256"))
    dev = "cuda"
    res = {}
    for (hw, c), (ft, dt) in SHAPES.items():
        x = torch.randn(n, hw, hw, c, device=dev).bfloat16()
        wt = (torch.randn(3, 3, c, c, device=dev) / (9 * c) ** 0.5).bfloat16()
        wtt = C.transpose_filter(wt).clone()
        dy = torch.randn(n, hw, hw, c, device=dev).bfloat16()
        bx = torch.randn(n, hw, hw, c, device=dev).bfloat16()
        mask = torch.randint(0, 256, (n * hw * hw * c // 8,), device=dev, dtype=torch.uint8)
        sb = torch.zeros(2, 64, c, device=dev)
        y = torch.empty_like(x)
        dx = torch.empty_like(x)
        geo = C._geo(x.shape, wt.shape, (hw, hw), (1, 1), (1, 1, 1, 1), (1, 1))
        mt = N.I(0)

        def fwd():
            N.check(N.fn("mdtf_conv_fwd_v2")(N.ptr(x), N.ptr(wtt), N.ptr(y), N.ptr(sb[0]), N.ptr(sb[1]), 64, *geo,
                                             C._v2_code(ft[0], ft[2], ft[3]), ft[1], ctypes.byref(mt),
                                             N.stream_ptr()), "conv_fwd_v2")

        def bwd():
            N.check(N.fn("mdtf_conv_dgrad_v2")(N.ptr(dy), N.ptr(wt), N.ptr(dx), *geo, C._v2_code(dt[0], dt[2], dt[3]),
                                               dt[1], 0, N.ptr(bx), N.ptr(mask), N.ptr(sb[0]), N.ptr(sb[1]), 64,
                                               N.ptr(None), N.ptr(None), N.stream_ptr()), "conv_dgrad_v2")

        fl = 2.0 * n * hw * hw * c * c * 9
        r = {0: {"fwd": [], "bwd": []}, 15: {"fwd": [], "bwd": []}}
        for rnd in range(3):
            for m in (0, 15):
                C.set_conv_img_mask(m)
                tf = gtime(fwd) * 1000.0
                tb = gtime(bwd) * 1000.0
                r[m]["fwd"].append(tf)
                r[m]["bwd"].append(tb)
                print(json.dumps({"shape": [hw, c], "round": rnd, "img": int(m > 0), "fwd_us": round(tf, 2),
                                  "bwd_us": round(tb, 2)}), flush=True)
        C.set_conv_img_mask(-1)
        for m in (0, 15):
            f, b = statistics.median(r[m]["fwd"]), statistics.median(r[m]["bwd"])
            res["%dx%dx%d img%d" % (hw, hw, c, int(m > 0))] = {
                "fwd_us": round(f, 2), "bwd_us": round(b, 2), "fwd_TFs": round(fl / f / 1e6, 1),
                "bwd_TFs": round(fl / b / 1e6, 1)}
    print(json.dumps({"summary": res, "B": n}), flush=True)


if __name__ == "__main__":
    main()
