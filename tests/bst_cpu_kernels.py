"""Stand-in for paddlerec_amd.ops on CPU tensors for BSTLayer's host logic — TEST INFRASTRUCTURE ONLY.

The GEMMs, row merges, dropout masks, loss and AUC are tests/cpu_kernels.py's, the two Adagrad updates
tests/flen_cpu_kernels.py's; the new C-ABI calls (attention, add + layer norm, LeakyReLU, glue) evaluate the formulas of
tests/bst_ref.py in float32, writing through the same strided views the device kernels write through.  The product never
imports this module."""
import numpy as np
import torch

import bst_ref as R
from cpu_kernels import (IdGroups, Workspace, auc_histogram, colsum, dropout, gemm, ids_group, new_status,  # noqa: F401
                         segment_partials, sigmoid_logloss)
from flen_cpu_kernels import adagrad_dense, adagrad_rows  # noqa: F401
from oracle.dcn_v2_ref import dropout_keep

F32 = np.float32


def _n(t):
    return t.detach().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def linear_backward(X, G, W, ws, dW, db, relu_src=None, b_image=None, epilogue=None, aux0=None, relu_bits=None, out=None):
    gemm(X, G, ws, trans_a=True, out=dW)
    colsum(G, ws, out=db)
    return gemm(G, W, ws, trans_b=True, out=out)


def att_mask(B, L, H, p, seed, stream):
    """The softmax-weight mask of rec_mha_*: rec_dropout's keep rule over a virtual [B*H*L, L] matrix, scaled."""
    if not p:
        return None
    return dropout_keep((B * H * L, L), p, seed, stream).astype(F32) * (F32(1) / (F32(1) - F32(p)))


def mha_fwd(q, k, v, B, L, H, scale=1.0, p=0.0, seed=0, stream=0, out=None):
    o, lse, _ = R.mha_fwd(_n(q), _n(k), _n(v), B, L, H, scale, att_mask(B, L, H, p, seed, stream), dtype=F32)
    o = _t(o)
    return (o if out is None else out.copy_(o)), _t(lse)


def mha_bwd(q, k, v, B, L, H, out, lse, d_out, scale=1.0, p=0.0, seed=0, stream=0, grads=None):
    g = [_t(a) for a in R.mha_bwd(_n(q), _n(k), _n(v), B, L, H, _n(d_out), scale, att_mask(B, L, H, p, seed, stream), dtype=F32)]
    if grads is None:
        return tuple(g)
    for dst, src in zip(grads, g):
        dst.copy_(src)
    return tuple(grads)


def add_layer_norm_fwd(x, r=None, eps=1e-5, out=None, out_group=0):
    y, mean, rstd = R.add_layer_norm_fwd(_n(x), None if r is None else _n(r), eps, dtype=F32)
    y = _t(y)
    if out is None:
        out = y
    elif out_group:
        out[:, 1:, :].copy_(y.reshape(-1, out_group, y.shape[1]))
    else:
        out.copy_(y)
    return out, _t(mean), _t(rstd)


def add_layer_norm_bwd(y, rstd, dy, out=None, y_group=0):
    yn = _n(y[:, 1:, :]).reshape(dy.shape) if y_group else _n(y)
    dx = _t(R.add_layer_norm_bwd(yn, _n(rstd), _n(dy), dtype=F32))
    return dx if out is None else out.copy_(dx)


def leaky_relu_fwd(x, slope=0.01, out=None):
    y = _t(R.leaky_relu_fwd(_n(x), slope, dtype=F32))
    return (x if out is None else out).copy_(y)


def leaky_relu_bwd(y, dy, slope=0.01, out=None):
    dx = _t(R.leaky_relu_bwd(_n(y), _n(dy), slope, dtype=F32))
    return (dy if out is None else out).copy_(dx)


def bst_add(x, r=None, out=None):
    y = x.clone() if r is None else x + r
    return (x if out is None else out).copy_(y)


def bst_embed_fwd(ids, tables, X, Z, status):
    B, T = ids[0].shape
    w = [t.shape[1] for t in tables[:3]]
    rows = []
    for i in range(7):
        idn, tab = _n(ids[i]).reshape(B, -1), _n(tables[i])
        ok = (idn >= 0) & (idn < tab.shape[0])
        if not ok.all():
            status |= 1
        rows.append(np.where(ok[..., None], tab[np.where(ok, idn, 0)], F32(0)))
    hist, tgt = np.concatenate(rows[:3], 2), np.concatenate(rows[3:6], 2)
    X.copy_(_t(np.concatenate([hist, tgt], 1).reshape(B * (T + 1), sum(w))))
    Z[:, 0, :].copy_(_t(rows[6][:, 0, :]))


def bst_embed_bwd(dX, B, T, widths):
    d = dX.reshape(B, T + 1, -1)
    out, c = [None] * 6, 0
    for s, w in enumerate(widths):
        out[s] = d[:, :T, c:c + w].reshape(B * T, w).contiguous()
        out[s + 3] = d[:, T, c:c + w].contiguous()
        c += w
    return out


def bst_possum_fwd(z, bias, B):
    return (z.reshape(B, -1).sum(1, keepdim=True) + bias).contiguous()


def bst_possum_bwd(dy, P, dbias):
    dbias.copy_(dy.sum().reshape(1))
    return dy.reshape(-1, 1).repeat(1, P).reshape(-1, 1).contiguous()
