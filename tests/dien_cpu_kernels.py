"""Stand-in for paddlerec_amd.ops on CPU tensors for DIENLayer's host logic — TEST INFRASTRUCTURE ONLY.

The lookups, GEMMs, row merges and SGD updates are tests/cpu_kernels.py's; the DIEN ops (GRU layers, auxiliary loss,
position-wise attention) evaluate tests/dien_ref.py in float32.  The product never imports this module."""
import numpy as np
import torch

import dien_ref as R
from cpu_kernels import (IdGroups, Workspace, auc_histogram, bce_with_logits, colsum, emb_gather, gemm,  # noqa: F401
                         ids_group, new_status, segment_partials, sgd_dense, sparse_sgd_rows)

GRU_MAX_HIDDEN = 256
F32 = np.float32


def _n(t):
    return t.detach().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def linear_backward(X, G, W, ws, dW, db, relu_src=None, b_image=None, epilogue=None, aux0=None, relu_bits=None, out=None):
    gemm(X, G, ws, trans_a=True, out=dW)
    colsum(G, ws, out=db)
    return gemm(G, W, ws, trans_b=True, epilogue=epilogue or "none", aux0=aux0, out=out)


def gru_layer_fwd(X, W_ih, W_hh, b_ih, b_hh, ws, want_saved=True):
    H_out, sv = R.gru_fwd(_n(X), _n(W_ih), _n(W_hh), _n(b_ih), _n(b_hh), dtype=F32)
    return _t(H_out), (sv if want_saved else None)


def gru_layer_bwd(X, saved, W_ih, W_hh, ws, dW_ih, dW_hh, db_ih, db_hh, dH_out=None, dh_T=None, want_dX=True, dX_add=None):
    dGi, dGh = R.gru_bwd(saved, _n(W_hh), None if dH_out is None else _n(dH_out), None if dh_T is None else _n(dh_T),
                         dtype=F32)
    g = R.gru_param_grads(_n(X), saved, dGi, dGh, _n(W_ih), dtype=F32)
    for dst, key in ((dW_ih, "weight_ih"), (dW_hh, "weight_hh"), (db_ih, "bias_ih"), (db_hh, "bias_hh")):
        dst.copy_(_t(g[key]))
    if not want_dX:
        return None
    return _t(g["dX"] + (_n(dX_add) if dX_add is not None else 0))


def _neg(neg_item, neg_cat, Wi, Wc, padding_idx):
    return np.concatenate([R.lookup(_n(Wi), _n(neg_item), padding_idx), R.lookup(_n(Wc), _n(neg_cat), padding_idx)], 2)


def dien_aux_fwd(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat, ws, padding_idx=0, status=None, out=None):
    aux, _ = R.aux_fwd(_n(gru_out), _n(hist), _neg(neg_item, neg_cat, W_neg_item, W_neg_cat, padding_idx), dtype=F32)
    return torch.tensor([aux], dtype=torch.float32), status


def dien_aux_bwd(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat, d_hist, accumulate=True, d_aux=1.0,
                 padding_idx=0, status=None):
    d_go, dh, d_neg = R.aux_bwd(_n(gru_out), _n(hist), _neg(neg_item, neg_cat, W_neg_item, W_neg_cat, padding_idx), d_aux,
                                dtype=F32)
    d_hist.copy_(_t(dh + (_n(d_hist) if accumulate else 0)))
    return _t(d_go), _t(d_neg)


def dien_attention_seq(hist, q, mask, att_w, att_b, ws):
    w, x_att, saved = R.attention_fwd(_n(hist), _n(q), _n(mask), [_n(a) for a in att_w], [_n(a) for a in att_b], dtype=F32)
    return _t(w), _t(x_att), saved


def dien_attention_seq_bwd(hist, q, w, saved, att_w, dx_att, d_hist, ws, accumulate=True):
    dh, dq, _ = R.attention_bwd(_n(hist), _n(q), _n(w), saved, [_n(a) for a in att_w], _n(dx_att), dtype=F32)
    d_hist.copy_(_t(dh + (_n(d_hist) if accumulate else 0)))
    return _t(dq)
