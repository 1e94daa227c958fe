"""``tf.contrib.layers.group_norm`` on the NHWC kernels of ``csrc/groupnorm.hip``.

For an NHWC ``x`` [N, H, W, C], fp32 ``gamma`` / ``beta`` [C] and ``G`` groups of ``C / G`` adjacent channels::

    mean[n, g], var[n, g] (biased) over the H * W * C / G elements of the group
    y = act((x - mean) * rsqrt(var + eps) * gamma[c] + beta[c]),  act in {none, relu}

The HIP kernels run for GPU tensors in bf16 with ``C % 8 == 0``, ``C <= 2048`` and ``C % G == 0``.  Two designs
(``path``: None / 0 auto, 1 resident, 2 streaming): the resident kernels hold an image's strip of groups in LDS (one
read of ``x``, one write), the streaming kernels take any size with a statistics pass and an apply pass.  The forward
saves fp32 ``mean`` / ``rstd`` [N, G]; the backward recomputes the ReLU mask from them.  ``dgamma`` / ``dbeta`` are an
atomic-free two-phase reduction (per-image or per-chunk fp32 partials, then an fp64 sum in index order) that lands in
the variables' fp32 gradient slots when there are any, and everything is bitwise repeatable.

Every other case runs the PyTorch expression in ``ops/nn.py``.
"""
import torch

from . import _native as N
from ..train import variables as V

MAX_C = 2048

# x, gamma, beta, y, mean, rstd, ws | N, H, W, C, G | eps | relu, path | stream
N.register("mdtf_gn_fwd", [N.P] * 7 + [N.I] * 5 + [N.F] + [N.I] * 2 + [N.P])
# x, dy, gamma, beta, mean, rstd, dx, dgamma, dbeta, ws | N, H, W, C, G | relu, accumulate, path | stream
N.register("mdtf_gn_bwd", [N.P] * 10 + [N.I] * 8 + [N.P])
N.register("mdtf_gn_fwd_ws", [N.I] * 6, restype=N.L)
N.register("mdtf_gn_bwd_ws", [N.I] * 6, restype=N.L)
N.register("mdtf_gn_chunk", [N.I], restype=N.L)
N.register("mdtf_gn_resident_fits", [N.I] * 5)


def native_ok(x, groups):
    """Whether the HIP kernels take this call (else the PyTorch expression runs)."""
    if x.dim() != 4:
        return False
    c = x.shape[-1]
    return (N.use_native(x) and x.dtype == torch.bfloat16 and c % 8 == 0 and 8 <= c <= MAX_C and groups >= 1
            and c % groups == 0)


def chunk_vectors(c):
    """16-byte vectors per chunk of the streaming kernels (a whole number of pixels)."""
    return int(N.fn("mdtf_gn_chunk")(c))


def resident_fits(h, w, c, groups, backward):
    """Whether the resident design takes an ``h`` x ``w`` x ``c`` image (``backward``: x and dy both staged)."""
    return bool(N.fn("mdtf_gn_resident_fits")(h, w, c, groups, int(bool(backward))))


def _workspace(query, shape, groups, path, device):
    floats = N.fn(query)(*shape, groups, path)
    return torch.empty(max(int(floats), 1), dtype=torch.float32, device=device)


def forward_nhwc(x, gamma, beta, groups, eps, relu, path=0):
    """``(y, mean, rstd)``: y like ``x``, fp32 statistics [N, G]."""
    n = x.shape[0]
    y = torch.empty_like(x)                                        # every element is stored
    mean = torch.empty((n, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = _workspace("mdtf_gn_fwd_ws", x.shape, groups, path, x.device)
    N.check(N.fn("mdtf_gn_fwd")(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(mean), N.ptr(rstd), N.ptr(ws),
                                *x.shape, groups, float(eps), int(bool(relu)), path, N.stream_ptr()), "gn_fwd")
    return y, mean, rstd


def backward_nhwc(x, dy, gamma, beta, mean, rstd, groups, relu, dgamma, dbeta, accumulate, path=0):
    """``dx``; ``dgamma`` / ``dbeta`` (fp32 [C]) are stored, or added into when ``accumulate``."""
    dx = torch.empty_like(x)
    ws = _workspace("mdtf_gn_bwd_ws", x.shape, groups, path, x.device)
    N.check(N.fn("mdtf_gn_bwd")(N.ptr(x), N.ptr(dy), N.ptr(gamma), N.ptr(beta), N.ptr(mean), N.ptr(rstd), N.ptr(dx),
                                N.ptr(dgamma), N.ptr(dbeta), N.ptr(ws), *x.shape, groups, int(bool(relu)),
                                int(bool(accumulate)), path, N.stream_ptr()), "gn_bwd")
    return dx


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu, path):
        x = x.contiguous()
        g32, b32 = gamma.float().contiguous(), beta.float().contiguous()
        y, mean, rstd = forward_nhwc(x, g32, b32, groups, eps, relu, path)
        ctx.save_for_backward(x, mean, rstd, g32, b32, gamma, beta)
        ctx.args = (groups, relu, path)
        ctx.sinks = (V.grad_sink(gamma), V.grad_sink(beta))
        ctx.mark_non_differentiable(mean, rstd)
        return y, mean, rstd

    @staticmethod
    def backward(ctx, dy, _dmean, _drstd):
        x, mean, rstd, g32, b32, gamma, beta = ctx.saved_tensors
        groups, relu, path = ctx.args
        sg, sb = ctx.sinks
        if sg is not None and sb is not None:                      # straight into the fp32 grad slots
            dg, db = V.accumulate_slot(sg), V.accumulate_slot(sb)
            dx = backward_nhwc(x, dy.contiguous(), g32, b32, mean, rstd, groups, relu, dg, db, True, path)
            return dx, V.grad_marker(gamma), V.grad_marker(beta), None, None, None, None
        dg, db = torch.empty_like(g32), torch.empty_like(b32)
        dx = backward_nhwc(x, dy.contiguous(), g32, b32, mean, rstd, groups, relu, dg, db, False, path)
        return dx, dg.to(gamma.dtype), db.to(beta.dtype), None, None, None, None


def group_norm_nhwc(x, gamma, beta, groups, eps, relu, path=None):
    """The kernels' path (:func:`native_ok` holds): ``(y, mean, rstd)``."""
    return _GroupNorm.apply(x, gamma, beta, int(groups), float(eps), bool(relu), int(path or 0))
