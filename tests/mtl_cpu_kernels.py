"""Stand-in for paddlerec_amd.ops on CPU tensors for the host logic of paddlerec_amd/mtl.py (mmoe.py, ple.py) — TEST
INFRASTRUCTURE ONLY.

The GEMMs, the column sums, dense Adam and the AUC buckets are tests/cpu_kernels.py's; the three rec_mtl_* calls evaluate
the formulas of tests/mtl_ref.py in float32, writing through the same strided views the device kernels write through; the
ReLU pass and the strided copy are torch.  The product never imports this module."""
import numpy as np
import torch

import mtl_ref as R
from cpu_kernels import Workspace, adam_dense, auc_histogram, colsum, gemm, new_status  # noqa: F401

F32 = np.float32


def _n(t):
    return t.detach().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


class MtlMix:
    """paddlerec_amd.ops.MtlMix without the C descriptor."""

    def __init__(self, expert_size, n_slots, gates):
        self.expert_size, self.n_slots = int(expert_size), int(n_slots)
        self.gates = [tuple(int(x) for x in (tuple(g) + (0, 0))[:4]) for g in gates]
        self.n_gates = len(self.gates)
        self.n_logit = sum(g[1] + g[3] for g in self.gates)


def linear_backward(X, G, W, ws, dW, db, relu_src=None, b_image=None, epilogue=None, aux0=None, relu_bits=None, out=None):
    gemm(X, G, ws, trans_a=True, out=dW)
    colsum(G, ws, out=db)
    if relu_src is not None:
        return gemm(G, W, ws, trans_b=True, epilogue="relu_mask", aux0=relu_src, out=out)
    return gemm(G, W, ws, trans_b=True, out=out)


def leaky_relu_fwd(x, slope=0.01, out=None):
    y = torch.where(x > 0, x, x * slope)
    return (x if out is None else out).copy_(y)


def bst_add(x, r=None, out=None):
    y = x.clone() if r is None else x + r
    return (x if out is None else out).copy_(y)


def mtl_mix_fwd(mix, H, logits, prob=None, out=None):
    p, m = R.mix_fwd(_n(H), _n(logits), mix.expert_size, mix.n_slots, R.gate_slots(mix.gates), dtype=F32)
    p, m = _t(p), _t(m)
    return (p if prob is None else prob.copy_(p)), (m if out is None else out.copy_(m))


def mtl_mix_bwd(mix, H, prob, dmix, relu=True, dH=None, dlogits=None):
    a, b = R.mix_bwd(_n(H), _n(prob), _n(dmix), mix.expert_size, mix.n_slots, R.gate_slots(mix.gates), relu, dtype=F32)
    a, b = _t(a), _t(b)
    return (a if dH is None else dH.copy_(a)), (b if dlogits is None else dlogits.copy_(b))


def mtl_head(logits, label, grad_scale=1.0, want_grad=True):
    pred, cost, dl = R.head(_n(logits), _n(label), F32(grad_scale), dtype=F32)
    return _t(pred), _t(cost), (_t(dl) if want_grad else None)
