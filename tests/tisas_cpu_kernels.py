"""Stand-in for paddlerec_amd.ops on CPU tensors for the host logic of paddlerec_amd/tisas.py — TEST INFRASTRUCTURE ONLY.

Everything tests/aitm_cpu_kernels.py has (GEMM and its epilogues, the gather, the id grouping, the segment partials, the
non-lazy row Adam, the dense Adam, rec_dropout), the ReLU mask, and the new ops: rec_tisas_attn_fwd / _bwd,
rec_affine_layer_norm_fwd / _bwd, rec_tisas_embed_fwd / _bwd and rec_tisas_head evaluate the formulas of tests/tisas_ref.py in
float32, with the masks rec_dropout's keep rule gives for the same (p, seed, stream), writing through the same views the
device kernels write through.  The product never imports this module."""
import numpy as np
import torch

from aitm_cpu_kernels import *  # noqa: F401,F403
from cpu_kernels import emb_gather  # noqa: F401
from gatenet_cpu_kernels import relu_mask_  # noqa: F401
from mtl_cpu_kernels import _n, _t
from oracle.dcn_v2_ref import dropout_keep

import tisas_ref as TR  # noqa: E402  (after the star import, which exports an R of its own)

F32 = np.float32
TISAS_SITES = ("att", "pos_k", "pos_v", "time_k", "time_v")


def keep_mask(shape, p, seed, stream):
    """rec_dropout applied to ones of `shape` ([rows, cols]) -> float32 mask, None for p == 0."""
    if not p:
        return None
    return dropout_keep(shape, p, seed, stream).astype(F32) * (F32(1) / (F32(1) - F32(p)))


def attn_masks(B, L, H, D, probs, seed, streams):
    shapes = dict(att=(B * H * L, L), pos_k=(B * L, D), pos_v=(B * L, D), time_k=(B * L * L, D), time_v=(B * L * L, D))
    p = dict(att=probs[0], pos_k=probs[1], pos_v=probs[1], time_k=probs[2], time_v=probs[2])
    return {s: keep_mask(shapes[s], p[s], seed, st) for s, st in zip(TISAS_SITES, streams)}


def _put(dst, src):
    src = _t(np.ascontiguousarray(src, dtype=F32))
    return src if dst is None else dst.copy_(src.reshape(dst.shape))


def tisas_attn_fwd(q, k, v, tables, tm, log_seqs, H, scale, probs=(0.0, 0.0, 0.0), seed=0, streams=(0, 0, 0, 0, 0),
                   status=None, out=None):
    B, L = log_seqs.shape
    T = tables[2].shape[0]
    tmn = tm.numpy()
    if status is not None and ((tmn < 0) | (tmn >= T)).any():
        status |= 1
    tmn = np.where((tmn < 0) | (tmn >= T), 0, tmn)
    o, lse, _ = TR.attn_fwd(_n(q), _n(k), _n(v), [_n(t) for t in tables], tmn, log_seqs.numpy(), H, scale,
                           attn_masks(B, L, H, q.shape[1], probs, seed, streams), F32)
    return _put(out, o), _t(lse.astype(F32))


def tisas_attn_bwd(q, k, v, tables, tm, log_seqs, H, scale, lse, d_out, d_tables, probs=(0.0, 0.0, 0.0), seed=0,
                   streams=(0, 0, 0, 0, 0), grads=None, accumulate=False, scratch=None):
    B, L = log_seqs.shape
    T = tables[2].shape[0]
    tmn = tm.numpy()
    tmn = np.where((tmn < 0) | (tmn >= T), 0, tmn)
    _, _, c = TR.attn_fwd(_n(q), _n(k), _n(v), [_n(t) for t in tables], tmn, log_seqs.numpy(), H, scale,
                         attn_masks(B, L, H, q.shape[1], probs, seed, streams), F32)
    r = TR.attn_bwd(_n(d_out), c, F32)
    grads = grads if grads is not None else (None, None, None)
    out = tuple(_put(dst, src) for dst, src in zip(grads, r[:3]))
    for dst, src in zip(d_tables, r[3:]):
        src = _t(np.ascontiguousarray(src, dtype=F32))
        dst.add_(src) if accumulate else dst.copy_(src)
    return out


def affine_layer_norm_fwd(x, gamma, beta, eps, r=None, row_ids=None, sum_out=None, out=None):
    y, t, mu, rs = TR.ln_fwd(_n(x), _n(gamma), _n(beta), eps, _n(r) if r is not None else None,
                            row_ids.numpy() if row_ids is not None else None, F32)
    if sum_out is not None:
        _put(sum_out, t)
    return _put(out, y), _t(mu.astype(F32)), _t(rs.astype(F32))


def affine_layer_norm_bwd(t, mean, rstd, gamma, dy, dgamma, dbeta, dy2=None, e1=None, e2=None, row_ids=None, out=None):
    g = _n(dy) + (_n(dy2) if dy2 is not None else F32(0))
    extra = None
    if e1 is not None or e2 is not None:
        extra = (_n(e1) if e1 is not None else F32(0)) + (_n(e2) if e2 is not None else F32(0))
    dx, dg, db = TR.ln_bwd(_n(t), _n(mean), _n(rstd), _n(gamma), g, row_ids.numpy() if row_ids is not None else None, extra, F32)
    _put(dgamma, dg)
    _put(dbeta, db)
    return _put(out, dx)


def tisas_embed_fwd(ids, table, scale, p=0.0, seed=0, stream=0, status=None, out=None):
    idn = ids.numpy().reshape(-1)
    bad = (idn < 0) | (idn >= table.shape[0])
    if status is not None and bad.any():
        status |= 1
    x = TR.embed_fwd(_n(table), np.where(bad, 0, idn), F32(scale), keep_mask((idn.size, table.shape[1]), p, seed, stream), F32)
    return _put(out, x)


def tisas_embed_bwd(ids, d_out, num_rows, scale, p=0.0, seed=0, stream=0, out=None):
    idn = ids.numpy().reshape(-1)
    idn = np.where((idn < 0) | (idn >= num_rows), 0, idn)
    return _put(out, TR.embed_bwd(_n(d_out), idn, F32(scale), keep_mask(tuple(d_out.shape), p, seed, stream), F32))


def tisas_head(feats, pos, neg, table, status=None, d_pos_rows=None, d_neg_rows=None):
    f = _n(feats)
    h = TR.head(f, pos.numpy(), neg.numpy(), _n(table), F32)
    if d_pos_rows is not None:
        _put(d_pos_rows, h["coef_pos"][:, None] * f)
    if d_neg_rows is not None:
        _put(d_neg_rows, h["coef_neg"][:, None] * f)
    one = lambda a: _t(np.ascontiguousarray(a, dtype=F32))
    return (one(np.array([h["loss"], h["cnt"]])), one(h["d_feats"]), one(h["coef_pos"]), one(h["coef_neg"]), one(h["row_loss"]),
            one(h["pl"]), one(h["nl"]))
