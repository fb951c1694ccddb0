"""cpu_kernels (the oracle-backed stand-in for paddlerec_amd.ops on CPU tensors) plus the four FAT-DeepFFM operators from
fat_deepffm_ref and relu_mask_ — TEST INFRASTRUCTURE ONLY: runs the host orchestration of paddlerec_amd.fat_deepffm
without a GPU."""
import numpy as np
import torch

import fat_deepffm_ref as FR
from cpu_kernels import *  # noqa: F401,F403
from cpu_kernels import _n


def _put(dst, a):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(dst.shape))
    return dst


def _cube(ids, dense, W, dense_w, dim, status):
    idn = _n(ids)
    if ((idn < 0) | (idn >= W.shape[0])).any() and status is not None:
        status |= 1
    return FR.cube(idn, _n(dense), _n(W), _n(dense_w), dim)


def fatffm_pool_fwd(ids, dense, W, dense_w, dim, status=None, out=None):
    E = _cube(ids, dense, W, dense_w, dim, status)
    F = E.shape[1]
    return _put(out if out is not None else torch.empty(len(E), F * F), FR.pool(E)[0]), status


def fatffm_inter_fwd(ids, dense, W, dense_w, a, dim, status=None, out=None):
    E = _cube(ids, dense, W, dense_w, dim, status)
    H, y1 = FR.inter(E, _n(a))
    Ht, y1t = out if out is not None else (None, None)
    return (_put(Ht if Ht is not None else torch.empty(H.shape), H),
            _put(y1t if y1t is not None else torch.empty(len(E), 1), y1), status)


def fatffm_attn_bwd(ids, dense, W, dense_w, a, dH, dz, dim, status=None, out=None):
    E = _cube(ids, dense, W, dense_w, dim, status)
    d_a = FR.attn_bwd(E, _n(a), _n(dH), _n(dz))
    return _put(out if out is not None else torch.empty(d_a.shape), d_a), status


def fatffm_bwd(ids, dense, W, dense_w, a, dH, dz, d_pooled, dim, ws, out=None, status=None, grad_stride=None):
    E = _cube(ids, dense, W, dense_w, dim, status)
    B, S = ids.shape
    R = E.shape[1] * dim
    gs = grad_stride or (R + 3) // 4 * 4
    rg, ddw = FR.rows_grads(FR.cube_bwd(E, _n(a), _n(dH), _n(dz), _n(d_pooled)), _n(dense), S, gs)
    rgt, ddwt = out if out is not None else (None, None)
    return (_put(rgt if rgt is not None else torch.empty(B * S, gs), rg),
            _put(ddwt if ddwt is not None else torch.empty(ddw.shape), ddw), status)


def relu_mask_(dy, y):
    return dy.mul_((y > 0).to(dy.dtype))
