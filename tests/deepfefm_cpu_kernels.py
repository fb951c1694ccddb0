"""cpu_kernels (the oracle-backed stand-in for paddlerec_amd.ops on CPU tensors) plus fefm_fwd / fefm_bwd from
deepfefm_ref and the row updates with the L2 term — TEST INFRASTRUCTURE ONLY: runs the host orchestration of
paddlerec_amd.deepfefm without a GPU."""
import numpy as np
import torch

import cpu_kernels as _base
import deepfefm_ref
from cpu_kernels import *  # noqa: F401,F403
from cpu_kernels import _merged_rows, _n
from oracle import deepfm_ref as R


def _safe(ids_all, N, status):
    """Out-of-range ids are flagged and read as the zero row (id 0), as the device kernels treat them."""
    oob = (ids_all < 0) | (ids_all >= N)
    if oob.any() and status is not None:
        status |= 1
    return np.where(oob, 0, ids_all), oob


def _derived(dense):
    d = _n(dense).astype(np.float32)
    c = (d * np.float32(1e5) + np.float32(1e6)) + np.float32(2)
    ok = np.isfinite(c) & (np.abs(c) < 9.0e18)
    return np.where(ok, np.where(ok, c, 0).astype(np.int64), -1)


def fefm_fwd(ids, dense, W, W1, dense_w_one, FE, dim, ws, status=None, out=None):
    idn = _n(ids)
    B, S = idn.shape
    N = W.shape[0]
    ids_all = np.concatenate([idn, _derived(dense)], axis=1)
    safe, _ = _safe(ids_all, N, status)
    p = {"W": _n(W), "W1": _n(W1), "dense_w_one": _n(dense_w_one), "FE": _n(FE)}
    cols = S * dim + dense.shape[1] + FE.shape[0]
    o = _reference(safe, S, _n(dense), p, dim, np.zeros(B), np.zeros((B, cols)))
    if out is None:
        out = (torch.empty(B, 1), torch.empty(B, 1), torch.empty(B, cols), torch.empty(B, ids_all.shape[1], dtype=torch.int64))
    y1, y2, dnn_in, ia = out
    y1.copy_(torch.from_numpy(o["y1"].astype(np.float32)).reshape(y1.shape))
    y2.copy_(torch.from_numpy(o["y2"].astype(np.float32)).reshape(y2.shape))
    dnn_in.copy_(torch.from_numpy(o["dnn_in"].astype(np.float32)))
    ia.copy_(torch.from_numpy(ids_all))
    return y1, y2, dnn_in, ia, status


def _reference(safe_all, S, dense, p, D, dz, d_dnn_in):
    return deepfefm_ref.kernel_reference(safe_all[:, :S], dense, p, D, dz, d_dnn_in, ids_all=safe_all)


def fefm_bwd(ids_all, dense, W, FE, dz, d_dnn_in, num_slots, dim, ws, want_d_fe=False, out=None, status=None,
             grad_stride=None):
    ia = _n(ids_all)
    B, F = ia.shape
    safe, _ = _safe(ia, W.shape[0], status)
    Dn = dense.shape[1]
    p = {"W": _n(W), "W1": np.zeros(W.shape[0]), "dense_w_one": np.zeros(Dn), "FE": _n(FE)}
    o = _reference(safe, num_slots, _n(dense), p, dim, _n(dz).reshape(B), _n(d_dnn_in))
    gs = grad_stride or (dim + 3) // 4 * 4
    rg = np.zeros((B * F, gs), np.float32)
    rg[:, :dim] = o["row_grad"]
    if out is None:
        out = (torch.empty(B * F, gs), torch.empty(Dn), torch.empty(FE.shape) if want_d_fe else None)
    out[0].copy_(torch.from_numpy(rg))
    out[1].copy_(torch.from_numpy(o["d_dense_w_one"].astype(np.float32)))
    if want_d_fe:
        out[2].copy_(torch.from_numpy(o["d_FE"].astype(np.float32)))
    return out[0], out[1], (out[2] if want_d_fe else None)


def ids_group(ids, num_rows, padding_idx, ws, slot_offset=None, status=None, groups=None, payload=None):
    """As cpu_kernels.ids_group, with the device's treatment of ids outside [0, num_rows): flagged and dropped."""
    idn = _n(ids).reshape(-1)
    oob = (idn < 0) | (idn >= num_rows)
    if oob.any() and status is not None:
        status |= 1
    valid = ~oob & (idn != padding_idx if padding_idx is not None else True)
    groups.spos, groups.uniq, groups.offs = R.group_ids(np.where(valid, idn, 0), valid)
    return groups, status


def _l2(merged, l2, rows):
    return merged + np.float32(l2) * rows if l2 else merged


def sparse_adam_rows(groups, grad, grad_div, P, M, V, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                     partials=None, grad_group=0, grad_group_stride=0, grad_scale=None, grad_index=None, l2=0.0):
    merged = _merged_rows(groups, grad, P.shape[1], grad_div, grad_group, grad_group_stride, grad_index)
    if grad_scale is not None:
        merged = merged * np.float32(float(grad_scale[0]))
    merged = _l2(merged, l2, P.numpy()[groups.uniq])
    R.adam_update_rows(P.numpy(), M.numpy(), V.numpy(), groups.uniq, merged, step, lr=lr, beta1=beta1, beta2=beta2,
                       eps=eps)


def adam_rows_all(groups, grad, grad_div, P, M, V, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                  grad_group=0, grad_group_stride=0, grad_scale=None, partials=None, l2=0.0):
    merged = _merged_rows(groups, grad, P.shape[1], grad_div, grad_group, grad_group_stride)
    if grad_scale is not None:
        merged = merged * np.float32(float(grad_scale[0]))
    Pn, Mn, Vn = P.numpy().copy(), M.numpy().copy(), V.numpy().copy()      # strided views: work on copies
    g = np.zeros_like(Pn)
    g[groups.uniq] = merged
    if l2:
        g = g + np.float32(l2) * Pn
    R.adam_update(Pn, Mn, Vn, g, step, lr=lr, beta1=beta1, beta2=beta2, eps=eps)
    P.copy_(torch.from_numpy(Pn)); M.copy_(torch.from_numpy(Mn)); V.copy_(torch.from_numpy(Vn))


assert _base.Workspace is Workspace  # noqa: F405  (everything else comes from cpu_kernels unchanged)
