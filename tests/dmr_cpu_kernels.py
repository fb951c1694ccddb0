"""Stand-in for paddlerec_amd.ops on CPU tensors for DMRLayer's host logic — TEST INFRASTRUCTURE ONLY.

The lookups, GEMMs, BatchNorm, row merges and Adam updates are tests/cpu_kernels.py's; the new C-ABI calls (prefix pool,
PReLU, match loss, tail glue) evaluate the formulas of tests/dmr_ref.py in float32, writing through the same strided
views the device kernels write through.  The product never imports this module."""
import numpy as np
import torch

import dmr_ref as R
from cpu_kernels import (IdGroups, Workspace, adam_dense, adam_rows_all, auc_histogram, batchnorm_bwd,  # noqa: F401
                         batchnorm_fwd, bce_with_logits, colsum, emb_gather, gemm, ids_group, new_status, segment_partials)

F32 = np.float32


def _n(t):
    return t.detach().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def linear_backward(X, G, W, ws, dW, db, relu_src=None, b_image=None, epilogue=None, aux0=None, relu_bits=None, out=None):
    gemm(X, G, ws, trans_a=True, out=dW)
    colsum(G, ws, out=db)
    return gemm(G, W, ws, trans_b=True, epilogue=epilogue or "none", aux0=aux0, out=out)


def dien_att_feat_fwd(hist, q):
    return torch.cat([hist, q, hist - q, hist * q], -1).reshape(-1, 4 * hist.shape[-1])


def dien_att_feat_bwd(hist, q, dfeat, d_hist, accumulate=True):
    E = hist.shape[-1]
    d0, d1, d2, d3 = (dfeat[:, i * E:(i + 1) * E].reshape(hist.shape) for i in range(4))
    dh = (d0 + d2) + d3 * q
    d_hist.copy_(d_hist + dh if accumulate else dh)
    return (d1 - d2) + d3 * hist


def dmr_prefix_pool_fwd(score, mask, hist, rows, out=None, rel=None):
    B, T, D = hist.shape
    o, w, r = R.prefix_pool_fwd(_n(score).reshape(B, T), _n(mask), _n(hist), rows, dtype=F32)
    o = _t(o.reshape(B, len(rows) * D))
    if out is not None:
        out.copy_(o)
    if rel is not None:
        rel.copy_(_t(r.reshape(B, 1)))
    return (o if out is None else out), _t(w)


def dmr_prefix_pool_bwd(mask, hist, rows, w, d_out, d_hist, d_rel=None, accumulate=True):
    B, T, D = hist.shape
    ds, dh = R.prefix_pool_bwd(_n(mask), _n(hist), rows, _n(w), _n(d_out).reshape(B, len(rows), D),
                               None if d_rel is None else _n(d_rel), dtype=F32)
    d_hist.copy_(_t(dh) + d_hist if accumulate else _t(dh))
    return _t(ds)


def prelu_fwd(X, alpha, period=0, base=0, out=None):
    y = _t(R.prelu_fwd(_n(X), _n(alpha), period, base, dtype=F32))
    return y if out is None else out.copy_(y)


def prelu_bwd(X, dY, alpha, ws, period=0, base=0, dalpha=None, out=None):
    dx, da = R.prelu_bwd(_n(X), _n(dY), _n(alpha), period, base, dtype=F32)
    dx, da = _t(dx), _t(da)
    return (dx if out is None else out.copy_(dx)), (da if dalpha is None else dalpha.copy_(da))


def dmr_match_loss_fwd(U, V, bias, label, ws, status=None):
    loss, lse = R.match_loss_fwd(_n(U), _n(V), None if bias is None else _n(bias), _n(label), dtype=F32)
    return torch.tensor([loss], dtype=torch.float32), _t(lse), status


def dmr_match_loss_bwd(U, V, bias, label, lse, d_loss, dV, ws, accumulate=False):
    dU, dv = R.match_loss_bwd(_n(U), _n(V), None if bias is None else _n(bias), _n(label), d_loss, dtype=F32)
    dV.copy_(_t(dv) + dV if accumulate else _t(dv))
    return _t(dU)


def dmr_tail_fwd(hist, item_eb, uv, match_mask, V, cate_id, hist_sum, prod, rel_u2i, status):
    s = hist.sum(1)
    hist_sum.copy_(s)
    prod.copy_(item_eb * s)
    rel_u2i.copy_((uv[:, 1] * V[cate_id]).sum(-1, keepdim=True))
    return (uv[:, 0] * match_mask.to(torch.float32)).contiguous()


def dmr_tail_bwd_match(dU2, d_rel, uv, match_mask, V, cate_id, dV_rows):
    d_uv = torch.empty_like(uv)
    d_uv[:, 0] = 0 if dU2 is None else dU2 * match_mask.to(torch.float32)
    d_uv[:, 1] = d_rel * V[cate_id]
    dV_rows.copy_(d_rel * uv[:, 1])
    return d_uv


def dmr_tail_bwd_hist(f1, f2, d_sum, d_prod, item_eb, hist_sum, d_item_direct, d_ctx, d_hist, d_item):
    B, T, D = d_hist.shape
    a = (d_sum + d_prod * item_eb)[:, None, :]
    for f in (f1, f2):
        if f is not None:
            a = a + f.reshape(B, T, D)
    d_hist.add_(a)
    d_item.copy_(d_item_direct + d_prod * hist_sum + d_ctx[:, :D].reshape(B, T, D).sum(1))
