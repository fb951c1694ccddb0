"""cpu_kernels (the oracle-backed stand-in for paddlerec_amd.ops on CPU tensors) plus ffm_fwd / ffm_bwd from ffm_ref —
TEST INFRASTRUCTURE ONLY: runs the host orchestration of paddlerec_amd.ffm without a GPU."""
import numpy as np
import torch

import ffm_ref
from cpu_kernels import *  # noqa: F401,F403
from cpu_kernels import _n


def _params(W, W1, dense_w, dense_w_one):
    return {"W": _n(W), "W1": _n(W1).reshape(-1, 1), "dense_w": _n(dense_w), "dense_w_one": _n(dense_w_one)}


def ffm_fwd(ids, dense, W, W1, dense_w, dense_w_one, dim, status=None, out=None):
    idn = _n(ids)
    p = _params(W, W1, dense_w, dense_w_one)
    oob = (idn < 0) | (idn >= W.shape[0])
    if oob.any() and status is not None:
        status |= 1
    y1, y2 = ffm_ref.forward(np.where(oob, 0, idn), _n(dense), p, dim)
    y1t, y2t = out if out is not None else (torch.empty(len(idn), 1), torch.empty(len(idn), 1))
    y1t.copy_(torch.from_numpy(y1.astype(np.float32)))
    y2t.copy_(torch.from_numpy(y2.astype(np.float32)))
    return y1t, y2t, status


def ffm_bwd(ids, dense, W, dense_w, dz, dim, ws, out=None, status=None, grad_stride=None):
    idn = _n(ids)
    B, S = idn.shape
    Dn = dense.shape[1]
    R = (S + Dn) * dim
    gs = grad_stride or (R + 3) // 4 * 4
    p = {"W": _n(W), "dense_w": _n(dense_w)}
    rg, dw, dw1 = ffm_ref.backward(idn, _n(dense), p, dim, _n(dz), gs)
    if out is None:
        out = (torch.empty(B * S, gs), torch.empty(Dn, R), torch.empty(Dn))
    for t, a in zip(out, (rg, dw, dw1)):
        t.copy_(torch.from_numpy(a.astype(np.float32)).reshape(t.shape))
    return out
