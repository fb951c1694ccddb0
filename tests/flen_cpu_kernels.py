"""cpu_kernels (the oracle-backed stand-in for paddlerec_amd.ops on CPU tensors) plus the FLEN operators from flen_ref, the
two Adagrad updates and linear_backward — TEST INFRASTRUCTURE ONLY: runs the host orchestration of paddlerec_amd.flen
without a GPU."""
import numpy as np
import torch

import flen_ref
from cpu_kernels import *  # noqa: F401,F403
from cpu_kernels import _merged_rows, _n
from dcn_cpu_kernels import linear_backward  # noqa: F401
from oracle.dcn_v2_ref import dropout_keep  # noqa: F401  (the mask streams of `dropout`)


def _put(dst, a):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(dst.shape))
    return dst


def flen_fwd(ids, W, group_begin, kernel_mf, status=None, out=None):
    B, S = ids.shape
    D, G = W.shape[1], len(group_begin) - 1
    E, live = flen_ref.lookup(_n(ids), _n(W))
    if not live.all() and status is not None:
        status |= 1
    FW, h = flen_ref.flen_forward(E, list(group_begin), _n(kernel_mf))
    X0, H, F = out if out is not None else (None, None, None)
    return (_put(X0 if X0 is not None else torch.empty(B, S * D), E.reshape(B, -1)),
            _put(H if H is not None else torch.empty(B, D), h),
            _put(F if F is not None else torch.empty(B, G * D), FW.reshape(B, -1)), status)


def flen_bwd(ids, num_rows, group_begin, kernel_mf, FW, dH, g, ws, status=None, out=None):
    B, S = ids.shape
    D, G = dH.shape[1], len(group_begin) - 1
    idn = _n(ids)
    live = (idn >= 0) & (idn < num_rows)
    if not live.all() and status is not None:
        status |= 1
    rg, dk = flen_ref.flen_backward(_n(FW).reshape(B, G, D), list(group_begin), _n(kernel_mf), _n(dH),
                                    _n(g).reshape(B, S, D), live)
    _put(g, rg.reshape(B, -1))
    return g, _put(out if out is not None else torch.empty(len(dk)), dk), status


def _adagrad_f32(p, a, g, lr, eps):
    """acc += g*g; p -= lr * g / (sqrt(acc) + eps), every operation rounded to float32 as the kernels do."""
    lr, eps = np.float32(lr), np.float32(eps)
    a = a + g * g
    return p - (lr * g) / (np.sqrt(a) + eps), a


def adagrad_rows(groups, grad, grad_div, P, A, lr, epsilon=1e-6, grad_group=0, grad_group_stride=0, partials=None,
                 grad_index=None):
    merged = _merged_rows(groups, grad, P.shape[1], grad_div, grad_group, grad_group_stride, grad_index)
    Pn, An = P.numpy(), A.numpy()
    Pn[groups.uniq], An[groups.uniq] = _adagrad_f32(Pn[groups.uniq], An[groups.uniq], merged, lr, epsilon)


def adagrad_dense(p, acc, g, lr, epsilon=1e-6):
    pn, an = p.numpy(), acc.numpy()
    pn[...], an[...] = _adagrad_f32(pn, an, g.numpy().reshape(pn.shape), lr, epsilon)
