"""Body of ``test_optim_kernels.py::test_kernel_variants_bitwise_equal`` (not collected as a test).

``compute()`` runs sgd, momentum (both Nesterov settings), Adam (L2 and decoupled) and ``apply_multi_`` on seeded
inputs on the GPU and returns every output on the CPU.  Run as a script it saves them to ``argv[1]``: the test starts
it as a fresh process per setting of ``MDTF_NT_OPT`` / ``MDTF_ADAM_CHUNK``, which the kernel library reads once.
"""
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N = 4 * (2 * 512 + 257)         # two full Adam chunks and a ragged third; six grid-stride blocks


def compute():
    import optim_helpers as OH
    from mdtf.ops import _native
    from mdtf.ops import optim as O
    _native.lib()
    assert _native.mode() != "torch"
    dev = "cuda"
    inp = OH.make_inputs(N, 41, k=3)
    out = {}

    def fresh(*names):
        return [inp[k].to(dev) for k in names] + [torch.zeros(N, dtype=torch.bfloat16, device=dev)]

    def keep(tag, **tensors):
        for k, t in tensors.items():
            out["%s/%s" % (tag, k)] = t.cpu()

    g = inp["g"][0].to(dev)
    w, sh = fresh("w")
    O.sgd_(w, g, sh, 0.1, 0.5, 1e-2)
    keep("sgd", w=w, shadow=sh)
    for nesterov in (False, True):
        w, a, sh = fresh("w", "acc")
        O.momentum_(w, g, a, sh, 0.1, 0.9, 0.5, 1e-2, nesterov)
        keep("momentum%d" % nesterov, w=w, acc=a, shadow=sh)
    for decoupled in (False, True):
        w, m, v, sh = fresh("w", "m", "v")
        O.adam_(w, g, m, v, sh, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5, 1e-2, decoupled)
        keep("adam%d" % decoupled, w=w, m=m, v=v, shadow=sh)
    grads = [x.to(dev).bfloat16() for x in inp["g"]]
    lrs, lrts = [0.1, 0.05, 0.025], [0.013, 0.011, 0.009]
    for kind, flag in (("sgd", False), ("momentum", True), ("adam", True)):
        w, s1, s2, sh = fresh("w", "m", "v")
        O.apply_multi_(kind, w, grads, s1, s2, sh, lrs, lrts, momentum=0.9, grad_scale=0.5, weight_decay=1e-2,
                       flag=flag)
        keep("multi_" + kind, w=w, s1=s1, s2=s2, shadow=sh)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    torch.save(compute(), sys.argv[1])
