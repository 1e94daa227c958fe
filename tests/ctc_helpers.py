"""Cases, the fp64 oracle and the limits of ``tests/test_ctc.py`` (the limits are explained in its docstring)."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nhwc_helpers as NH  # noqa: E402
from nhwc_helpers import U  # noqa: E402

C_LOGADD = 13.0                 # c: roundings of one guarded three-term log-add, in units of U (test_ctc's docstring)
C_GRAD = 9.0                    # c': roundings of one term of the posterior sum and its share of the tail, in U
G = [1.0, -2.5, 0.5, 1.5]       # the upstream gradient, one value per item


class Case(object):
    """Seeded logits x [T, B, K] (bf16-representable fp32), labels [B, Lmax] and ragged lengths; ``ref`` holds the
    fp64 loss, gradient and their bounds, computed once."""

    def __init__(self, t, b, k, lmax, seed, labels=None, seq=None, lab_len=None):
        gen = torch.Generator().manual_seed(seed)
        self.shape = (t, b, k, lmax)
        self.x = NH.randn((t, b, k), seed, 2.0)
        self.labels = torch.randint(0, k - 1, (b, lmax), generator=gen) if labels is None else torch.tensor(labels)
        self.seq = torch.tensor([t - i for i in range(b)] if seq is None else seq, dtype=torch.int32)
        self.lab_len = torch.tensor([max(lmax - i, 0) for i in range(b)] if lab_len is None else lab_len,
                                    dtype=torch.int32)
        self.g = torch.tensor(G[:b])
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = oracle(self)
        return self._ref


def oracle(c):
    """``F.ctc_loss`` on CPU in fp64 over an fp64 ``log_softmax``, blank = K - 1, the gradient by autograd for the
    upstream ``c.g``; with them the bounds ``e_loss`` [B] and ``acc`` [T, B, K] of an fp32 implementation."""
    t_n, b_n, k, lmax = c.shape
    x = c.x.double().requires_grad_(True)
    lp = torch.log_softmax(x, -1)
    loss = F.ctc_loss(lp, c.labels, c.seq.long(), c.lab_len.long(), blank=k - 1, reduction="none")
    (dx,) = torch.autograd.grad(loss, x, c.g.double())
    lp, xs = lp.detach(), c.x.double().reshape(t_n * b_n, k)
    # alpha of the same fp64 oracle, [B, T, 2 Lmax + 1]
    alpha = torch._ctc_loss(lp, c.labels, c.seq.tolist(), c.lab_len.tolist(), k - 1, False)[1]
    lse = torch.logsumexp(xs, 1)
    chain = 2 * -(-k // 64) + 30                            # as test_losses._chain: a lane's terms, the merges
    e_lse = NH.lse_bound(xs, torch.zeros(t_n * b_n, dtype=torch.long), lse, chain)[0].reshape(t_n, b_n)
    e_loss, occ = torch.zeros(b_n, dtype=torch.float64), torch.zeros(b_n, k, dtype=torch.float64)
    for b in range(b_n):
        tb, ln = int(c.seq[b]), int(c.lab_len[b])
        sym = torch.cat([c.labels[b, :ln], torch.tensor([k - 1])])
        occ[b] = torch.bincount(sym, minlength=k)                       # states that hold each symbol
        occ[b, k - 1] += ln
        p_t = lp[:tb, b][:, sym].abs().max(1).values                    # max_s |lp[t, s]|
        a_t = alpha[b, :tb, :2 * ln + 1].abs()
        a_t = torch.where(torch.isfinite(a_t), a_t, torch.zeros_like(a_t)).max(1).values        # max_s |alpha_t(s)|
        e_loss[b] = (e_lse[:tb, b] + U * (a_t + p_t + C_LOGADD)).sum()
    a = (c.x.double() - lse.reshape(t_n, b_n, 1)).abs()
    p = torch.exp(lp)
    e_p = p * (e_lse[:, :, None] + NH.INTRINSIC_FACTOR * U * (1.4427 * a + 2.0))
    acc = c.g.double().abs()[None, :, None] * (e_p + occ[None] * (2 * e_loss[None, :, None] + C_GRAD * U))
    return dict(loss=loss.detach(), dx=dx, e_loss=e_loss + NH.TINY, acc=acc + NH.TINY)
