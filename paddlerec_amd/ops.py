"""Operator layer: torch tensors in, C-ABI calls out.

torch is plumbing here (device memory, streams); every op below is a hand-written HIP kernel in
librecengine.so.  Tensors must live on a ROCm device — there is deliberately no CPU path.
Reference call sites are cited in include/recengine.h next to each entry point.
"""
import collections
import contextlib
import ctypes as C
import os

import torch

from . import _lib
from ._lib import (EPI, AdagradHyper, AdamHyper, AitmHeadDesc, CinView, DcnCrossDesc, DeepFMDesc, DinDesc, EsmHeadDesc, FatFFMDesc, FEFMDesc, FFMDesc, GemmBImage, GemmDesc, GemmEpilogueArgs, GradLayout,
                   GradSrc, LazyInit, MtlMixDesc, MultislotDesc, PsAccessor, PsLayout, RecError, check)

_recorder = None        # paddlerec_amd.plan.CallPlan while a step is being recorded


def lib():
    """The loaded library — or, while a step is recorded (plan.py), a proxy that also lists every call."""
    h = _lib.lib()
    return h if _recorder is None else _recorder.proxy(h)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream.  torch.cuda.current_stream() builds a Stream object through four python
    layers (7.7 of the 24 profiled microseconds of one ops.gemm call); the raw accessors are one C call each."""
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    p = C.c_void_p(0 if t is None else t.data_ptr())
    if _recorder is not None and t is not None:
        _recorder.note_pointer(p, t)
    return p


_T_CACHE = {}


def _transposed(w):
    """w.t().contiguous(), kept while THIS tensor object is unchanged (the attention MLP is frozen in DIN's dygraph
    mode: one transpose per set_attention instead of one torch kernel per step)."""
    import weakref
    hit = _T_CACHE.get(id(w))
    if hit is None or hit[0]() is not w or hit[1] != w._version:
        if len(_T_CACHE) > 64:
            _T_CACHE.clear()
        hit = _T_CACHE[id(w)] = (weakref.ref(w), w._version, w.t().contiguous())
    return hit[2]


def copy_f32(dst, src):
    """dst[...] = src[...] (contiguous f32 device tensors of one size) as a C-ABI call (rec_copy_async)."""
    _chk(dst, torch.float32, "dst")
    _chk(src, torch.float32, "src")
    if dst.numel() != src.numel():
        raise RecError("copy_f32: %d != %d elements" % (dst.numel(), src.numel()))
    check(lib().rec_copy_async(_p(dst), _p(src), C.c_size_t(dst.numel() * 4), _stream()), "rec_copy_async")
    return dst


def _chk(t, dtype, name, shape=None):
    if t is None:
        return
    if not t.is_cuda:
        raise RecError("%s must be a device tensor (no CPU fallback)" % name)
    if t.dtype != dtype:
        raise RecError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RecError("%s must be contiguous" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RecError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))


def _chk_table(t, name):
    """A table is f32 [N,D] (or [N]) on the device with unit column stride; rows may be strided
    (a column slice of a wider record buffer).  Returns (D, row_stride)."""
    if not t.is_cuda:
        raise RecError("%s must be a device tensor (no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise RecError("%s must be float32, got %s" % (name, t.dtype))
    if t.dim() == 1:
        return 1, (t.stride(0) if t.numel() > 1 else 1)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RecError("%s must be [N,D] with unit column stride" % name)
    D, rs = t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])
    if rs < D:
        raise RecError("%s: row stride %d < D %d" % (name, rs, D))
    if D % 4 == 0 and rs % 4 == 0 and t.data_ptr() % 16 != 0:
        raise RecError("%s: rows must be 16-byte aligned" % name)
    return D, rs


def new_status(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_on_status(status, what="lookup"):
    """Host sync: raises if a kernel flagged an out-of-range id (Paddle raises on OOB [EXT])."""
    s = int(status.item())
    if s & _lib.REC_FLAG_INDEX_OOB:
        raise RecError("%s: index out of range [0, num_rows)" % what)
    if s & _lib.REC_FLAG_EXCHANGE_OVERFLOW:
        raise RecError("%s: a rank needed more distinct rows of one owner than the deduplicated exchange's capacity "
                       "(REC_SHARD_DEDUP_CAP)" % what)


class Workspace:
    """Grow-only device scratch owned by the caller of the C-ABI (the engine never allocates)."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return self.buf


def deepfm_train_step(net, ids, dense, label, step, ws, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, auc_stats=None,
                      num_thresholds=4095, status=None, out=None, side_stream=None):
    """The whole DeepFM train step through ONE C-ABI call (rec_deepfm_train_step).  net: a filled _lib.DeepFMNet (the
    caller keeps the tensors it points into alive).  side_stream (torch stream or None): the large-batch schedule of the
    mirror (grouping and sparse update beside the main stream's GEMMs).  -> (loss [1], pred [B,1])."""
    _chk(ids, torch.int64, "ids")
    _chk(dense, torch.float32, "dense")
    _chk(label, torch.int64, "label")
    B = ids.shape[0]
    if ids.shape[1] != net.num_slots or dense.shape[0] != B or label.numel() != B:
        raise RecError("ids / dense / label shapes do not fit the net")
    dev = ids.device
    if out is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
    else:
        loss, pred = out
    nbytes = C.c_size_t(0)
    check(lib().rec_deepfm_train_step_workspace_bytes(C.byref(net), B, C.byref(nbytes)),
          "rec_deepfm_train_step_workspace_bytes")
    w = ws.get(nbytes.value)
    h = _hyper(lr, beta1, beta2, eps, step)
    pos, neg = (auc_stats[0], auc_stats[1]) if auc_stats is not None else (None, None)
    check(lib().rec_deepfm_train_step(C.byref(net), B, _p(ids), _p(dense), _p(label), C.byref(h), _p(pos), _p(neg),
                                      int(num_thresholds), _p(loss), _p(pred), _p(status), _p(w),
                                      C.c_size_t(w.numel()), _stream(),
                                      C.c_void_p(side_stream.cuda_stream) if side_stream is not None else None),
          "rec_deepfm_train_step")
    return loss, pred


def din_train_step(net, hist_item, hist_cat, target_item, target_cat, label, mask, target_item_seq, target_cat_seq, lr, ws,
                   status=None, out=None, side_stream=None):
    """The whole DIN train step through ONE C-ABI call (rec_din_train_step).  net: a filled _lib.DinNet (the caller keeps
    the tensors it points into alive).  ids / mask [B,T] i64, targets [B] i64, label [B] f32.  -> (loss [1], pred [B,1])."""
    B, T = hist_item.shape
    for t, n in ((hist_item, "hist_item"), (hist_cat, "hist_cat"), (target_item_seq, "target_item_seq"),
                 (target_cat_seq, "target_cat_seq"), (mask, "mask")):
        _chk(t, torch.int64, n, (B, T))
    for t, n in ((target_item, "target_item"), (target_cat, "target_cat")):
        _chk(t, torch.int64, n)
        if t.numel() != B:
            raise RecError("%s must have one id per sample" % n)
    _chk(label, torch.float32, "label")
    if label.numel() != B:
        raise RecError("label must have one value per sample")
    dev = hist_item.device
    if out is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
    else:
        loss, pred = out
    if status is None:
        status = new_status(dev)
    nbytes = C.c_size_t(0)
    check(lib().rec_din_train_step_workspace_bytes(C.byref(net), B, T, C.byref(nbytes)), "rec_din_train_step_workspace_bytes")
    w = ws.get(nbytes.value)
    check(lib().rec_din_train_step(C.byref(net), B, T, _p(hist_item), _p(hist_cat), _p(target_item), _p(target_cat),
                                   _p(label), _p(mask), _p(target_item_seq), _p(target_cat_seq), float(lr), _p(loss),
                                   _p(pred), _p(status), _p(w), C.c_size_t(w.numel()), _stream(),
                                   None if side_stream is None else C.c_void_p(side_stream.cuda_stream)), "rec_din_train_step")
    return loss, pred


def dcn_v2_train_step(net, ids, dense, label, step, lr, ws, auc_stats=None, num_thresholds=4095, status=None, out=None,
                      beta1=0.9, beta2=0.999, eps=1e-8):
    """The whole DCN-v2 train step through ONE C-ABI call (rec_dcn_v2_train_step).  net: a filled _lib.DcnV2Net (the
    caller keeps the tensors it points into alive).  ids [B,S] i64, dense [B,Dn] f32, label [B(,1)] i64; step = Adam step
    count (1-based).  -> (loss [1], pred [B,1])."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[1] != net.num_slots:
        raise RecError("ids must be [batch, num_slots]")
    B = ids.shape[0]
    _chk(dense, torch.float32, "dense", (B, net.dense_dim))
    _chk(label, torch.int64, "label")
    if label.numel() != B:
        raise RecError("label must have one value per sample")
    dev = ids.device
    if out is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
    else:
        loss, pred = out
    if status is None:
        status = new_status(dev)
    pos = neg = None
    if auc_stats is not None:
        pos, neg = auc_stats
        _chk(pos, torch.int64, "stat_pos", (num_thresholds + 1,))
        _chk(neg, torch.int64, "stat_neg", (num_thresholds + 1,))
    h = _hyper(lr, beta1, beta2, eps, step)
    nbytes = C.c_size_t(0)
    check(lib().rec_dcn_v2_train_step_workspace_bytes(C.byref(net), B, C.byref(nbytes)),
          "rec_dcn_v2_train_step_workspace_bytes")
    w = ws.get(nbytes.value)
    check(lib().rec_dcn_v2_train_step(C.byref(net), B, _p(ids), _p(dense), _p(label), C.byref(h), _p(pos), _p(neg),
                                      int(num_thresholds), _p(loss), _p(pred), _p(status), _p(w), C.c_size_t(w.numel()),
                                      _stream()), "rec_dcn_v2_train_step")
    return loss, pred


SUPPORTS_FEAT_LD = True       # deepfm_fm_fwd / _bwd take feat_ld (a padded sample stride of feat)


def make_desc(B, S, Dn, D, num_rows, padding_idx, row_stride=None, w1_stride=1, compact=False, feat_stride=0):
    return DeepFMDesc(int(B), int(S), int(Dn), int(D), int(row_stride or D), int(num_rows),
                      -1 if padding_idx is None else int(padding_idx), int(w1_stride), int(bool(compact)),
                      int(feat_stride))


# ------------------------------------------------------------------ DeepFM FM block
def deepfm_fm_fwd(ids, dense, W, W1, dense_w, dense_w_one, padding_idx=0, slot_offset=None,
                  status=None, out=None, compact=False, feat_ld=0):
    """ids [B,S] i64, dense [B,Dn] f32, W [N,D], W1 [N,1]|[N], dense_w [Dn,D]|[1,Dn,D], dense_w_one [Dn]
    -> y1 [B,1], y2 [B,1], feat [B,S+Dn,D], sum_emb [B,D], status
    compact: feat is [B,S+1,D] — S embedding rows + one row of the raw dense values (rec_deepfm_desc.compact_dense)."""
    B, S = ids.shape
    Dn = dense.shape[1]
    N, D = W.shape
    dev = ids.device
    _chk(ids, torch.int64, "ids")
    _chk(dense, torch.float32, "dense", (B, Dn))
    _, w_stride = _chk_table(W, "W")
    _, w1_stride = _chk_table(W1, "W1")
    _chk(dense_w, torch.float32, "dense_w")
    _chk(dense_w_one, torch.float32, "dense_w_one", (Dn,))
    _chk(slot_offset, torch.int64, "slot_offset", (S,))
    if W1.numel() != N or dense_w.numel() != Dn * D:
        raise RecError("W1 / dense_w shape mismatch")
    if out is None:
        y1 = torch.empty(B, 1, dtype=torch.float32, device=dev)
        y2 = torch.empty(B, 1, dtype=torch.float32, device=dev)
        feat = torch.empty(B, S + 1 if compact else S + Dn, D, dtype=torch.float32, device=dev)
        sum_emb = torch.empty(B, D, dtype=torch.float32, device=dev)
    else:
        y1, y2, feat, sum_emb = out
    if status is None:
        status = new_status(dev)
    if feat_ld:          # feat_ld: feat is a caller-kept zero-initialised [B, feat_ld] buffer (rec_deepfm_desc.feat_stride)
        if out is None or feat.dim() != 2 or feat.shape[1] != feat_ld or not feat.is_contiguous():
            raise RecError("feat_ld needs out=(y1, y2, feat [B, feat_ld], sum_emb)")
    desc = make_desc(B, S, Dn, D, N, padding_idx, w_stride, w1_stride, compact, feat_ld)
    check(lib().rec_deepfm_fm_fwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(W1), _p(dense_w),
                                  _p(dense_w_one), _p(slot_offset), _p(y1), _p(y2), _p(feat),
                                  _p(sum_emb), _p(status), _stream()), "rec_deepfm_fm_fwd")
    return y1, y2, feat, sum_emb, status


def deepfm_fm_bwd(dense, feat, sum_emb, d_feat_dnn, dy1, dy2, S, ws, out=None, dense_w=None, compact=False,
                  row_rank=None, feat_ld=0):
    """-> row_grad [B*S,D], d_dense_w [Dn,D], d_dense_w_one [Dn].
    dense_w ([Dn,D] / [1,Dn,D], optional): recompute the dense part of feat instead of re-reading it.
    compact: feat / d_feat_dnn are [B,S+1,D] and d_dense_w is the FM part only (see deepfm_fm_fwd).
    row_rank [B*S] i32 (IdGroups.rank): row_grad is written in SORTED order (rec_deepfm_fm_bwd_sorted)."""
    if feat_ld:          # feat / d_feat_dnn are [B, feat_ld] (padded sample stride)
        B, D = sum_emb.shape
        Dn = dense.shape[1]
        F = S + 1 if compact else S + Dn
        if feat.shape != (B, feat_ld) or d_feat_dnn.shape != (B, feat_ld) or feat_ld < F * D:
            raise RecError("feat / d_feat_dnn must be [B, feat_ld] with feat_ld >= fields x emb_dim")
    else:
        B, F, D = feat.shape
        Dn = dense.shape[1] if compact else F - S
    dev = feat.device
    for t, n in ((dense, "dense"), (feat, "feat"), (sum_emb, "sum_emb"), (d_feat_dnn, "d_feat_dnn"),
                 (dy1, "dy1"), (dy2, "dy2")):
        _chk(t, torch.float32, n)
    if d_feat_dnn.numel() != feat.numel() or dy1.numel() != B or dy2.numel() != B:
        raise RecError("gradient shape mismatch")
    if not (feat.is_contiguous() and d_feat_dnn.is_contiguous()):
        raise RecError("feat / d_feat_dnn must be contiguous")
    if dense_w is not None:
        _chk(dense_w, torch.float32, "dense_w")
        if dense_w.numel() != Dn * D:
            raise RecError("dense_w shape mismatch")
    if out is None:
        row_grad = torch.empty(B * S, D, dtype=torch.float32, device=dev)
        d_dense_w = torch.empty(Dn, D, dtype=torch.float32, device=dev)
        d_dense_w_one = torch.empty(Dn, dtype=torch.float32, device=dev)
    else:
        row_grad, d_dense_w, d_dense_w_one = out
    desc = make_desc(B, S, Dn, D, 1, None, compact=compact, feat_stride=feat_ld)
    nbytes = C.c_size_t(0)
    check(lib().rec_deepfm_fm_bwd_workspace_bytes(C.byref(desc), C.byref(nbytes)))
    w = ws.get(nbytes.value)
    if row_rank is not None:
        _chk(row_rank, torch.int32, "row_rank")
        if row_rank.numel() < B * S:
            raise RecError("row_rank shorter than B*S")
        check(lib().rec_deepfm_fm_bwd_sorted(C.byref(desc), _p(dense), _p(feat), _p(sum_emb), _p(d_feat_dnn),
                                             _p(dy1), _p(dy2), _p(dense_w), _p(row_rank), _p(row_grad),
                                             _p(d_dense_w), _p(d_dense_w_one), _p(w), C.c_size_t(w.numel()),
                                             _stream()), "rec_deepfm_fm_bwd_sorted")
        return row_grad, d_dense_w, d_dense_w_one
    check(lib().rec_deepfm_fm_bwd(C.byref(desc), _p(dense), _p(feat), _p(sum_emb), _p(d_feat_dnn),
                                  _p(dy1), _p(dy2), _p(dense_w), _p(row_grad), _p(d_dense_w),
                                  _p(d_dense_w_one),
                                  _p(w), C.c_size_t(w.numel()), _stream()), "rec_deepfm_fm_bwd")
    return row_grad, d_dense_w, d_dense_w_one


# ------------------------------------------------------------------ FFM field-aware interaction
def _ffm_desc(ids, dense, dim, W, what):
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2:
        raise RecError("%s: ids must be [B, S]" % what)
    B, S = ids.shape
    _chk(dense, torch.float32, "dense")
    if dense.dim() != 2 or dense.shape[0] != B:
        raise RecError("%s: dense must be [B, Dn]" % what)
    Dn = dense.shape[1]
    width, stride = _chk_table(W, "W")
    R = (S + Dn) * int(dim)
    if width < R:
        raise RecError("%s: W rows hold %d floats, fields x dim = %d" % (what, width, R))
    return B, S, Dn, R, stride


def ffm_fwd(ids, dense, W, W1, dense_w, dense_w_one, dim, status=None, out=None):
    """ids [B,S] i64, dense [B,Dn] f32, W [N, >= R] (R = (S+Dn)*dim; a padded row stride is fine), W1 [N,1]|[N],
    dense_w [Dn,R]|[1,Dn,R], dense_w_one [Dn] -> y1 [B,1], y2 [B,1], status  (rec_ffm_fwd)."""
    B, S, Dn, R, stride = _ffm_desc(ids, dense, dim, W, "ffm_fwd")
    N = W.shape[0]
    _chk(W1, torch.float32, "W1")
    _chk(dense_w, torch.float32, "dense_w")
    _chk(dense_w_one, torch.float32, "dense_w_one", (Dn,))
    if W1.numel() != N or dense_w.numel() != Dn * R:
        raise RecError("ffm_fwd: W1 / dense_w shape mismatch")
    dev = ids.device
    if out is None:
        y1 = torch.empty(B, 1, dtype=torch.float32, device=dev)
        y2 = torch.empty(B, 1, dtype=torch.float32, device=dev)
    else:
        y1, y2 = out
        _chk(y1, torch.float32, "y1")
        _chk(y2, torch.float32, "y2")
        if y1.numel() != B or y2.numel() != B:
            raise RecError("ffm_fwd: y1 / y2 must hold B values")
    if status is None:
        status = new_status(dev)
    desc = FFMDesc(B, S, Dn, int(dim), N, stride, 0)
    check(lib().rec_ffm_fwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(W1), _p(dense_w), _p(dense_w_one), _p(y1),
                            _p(y2), _p(status), _stream()), "rec_ffm_fwd")
    return y1, y2, status


def ffm_bwd(ids, dense, W, dense_w, dz, dim, ws, out=None, status=None, grad_stride=None):
    """dz [B] | [B,1] = dloss / dlogit -> row_grad [B*S, grad_stride] (default: R rounded up to 4 floats; the pad
    columns are 0), d_dense_w [Dn,R], d_dense_w_one [Dn]  (rec_ffm_bwd).  The W1 gradient is dz itself, read with
    grad_div = S by the row updates."""
    B, S, Dn, R, stride = _ffm_desc(ids, dense, dim, W, "ffm_bwd")
    _chk(dense_w, torch.float32, "dense_w")
    _chk(dz, torch.float32, "dz")
    if dense_w.numel() != Dn * R or dz.numel() != B:
        raise RecError("ffm_bwd: dense_w / dz shape mismatch")
    gs = int(grad_stride) if grad_stride else (R + 3) // 4 * 4
    dev = ids.device
    if out is None:
        row_grad = torch.empty(B * S, gs, dtype=torch.float32, device=dev)
        d_dense_w = torch.empty(Dn, R, dtype=torch.float32, device=dev)
        d_dense_w_one = torch.empty(Dn, dtype=torch.float32, device=dev)
    else:
        row_grad, d_dense_w, d_dense_w_one = out
    _chk(row_grad, torch.float32, "row_grad", (B * S, gs))
    _chk(d_dense_w, torch.float32, "d_dense_w")
    _chk(d_dense_w_one, torch.float32, "d_dense_w_one", (Dn,))
    if d_dense_w.numel() != Dn * R:
        raise RecError("ffm_bwd: d_dense_w must hold Dn x R floats")
    desc = FFMDesc(B, S, Dn, int(dim), W.shape[0], stride, gs)
    nbytes = C.c_size_t(0)
    check(lib().rec_ffm_bwd_workspace_bytes(C.byref(desc), C.byref(nbytes)), "rec_ffm_bwd_workspace_bytes")
    w = ws.get(nbytes.value)
    check(lib().rec_ffm_bwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(dense_w), _p(dz), _p(row_grad), _p(d_dense_w),
                            _p(d_dense_w_one), _p(w), C.c_size_t(w.numel()), _p(status), _stream()), "rec_ffm_bwd")
    return row_grad, d_dense_w, d_dense_w_one


# ------------------------------------------------------------------ FAT-DeepFFM CENet / field-pair kernels (fat_deepffm)
def _fat_mat(t, B, cols, name, what):
    """A [B, >= cols] float32 device matrix with unit column stride (a padded row stride is fine) -> leading dimension."""
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.shape[0] != B or t.shape[1] < cols or \
            (t.shape[1] > 1 and t.stride(1) != 1):
        raise RecError("%s: %s must be a float32 device matrix [B, >= %d] with unit column stride" % (what, name, cols))
    return max(t.stride(0), cols) if B > 1 else max(t.shape[1], cols)


def _fat_out(out, B, cols, dev):
    return out if out is not None else torch.empty(B, cols, dtype=torch.float32, device=dev)


def _fat_desc(ids, dense, W, dense_w, dim, what, attn=(), pair=(), grad_stride=0):
    """attn / pair: (tensor, name) matrices that share ld_attn / ld_pair."""
    B, S, Dn, R, stride = _ffm_desc(ids, dense, dim, W, what)
    _chk(dense_w, torch.float32, "dense_w")
    if dense_w.numel() != Dn * R:
        raise RecError("%s: dense_w must hold Dn x R floats" % what)
    F = S + Dn
    lds = []
    for mats, cols in ((attn, F * F), (pair, F * (F - 1) // 2 * int(dim))):
        ld = {_fat_mat(t, B, cols, n, what) for t, n in mats}
        if len(ld) > 1:
            raise RecError("%s: %s must share one leading dimension" % (what, " / ".join(n for _, n in mats)))
        lds.append(ld.pop() if ld else cols)
    return FatFFMDesc(FFMDesc(B, S, Dn, int(dim), W.shape[0], stride, int(grad_stride)), lds[0], lds[1]), B, S, Dn, R


def fatffm_pool_fwd(ids, dense, W, dense_w, dim, status=None, out=None):
    """ids [B,S] i64, dense [B,Dn] f32, W [N, >= R] (R = (S+Dn)*dim), dense_w [Dn,R]|[1,Dn,R] -> pooled [B, F*F] (or the
    wider-rowed matrix given as out: its row stride is used), status  (rec_fatffm_pool_fwd)."""
    F = ids.shape[1] + dense.shape[1]
    pooled = _fat_out(out, ids.shape[0], F * F, ids.device)
    desc, B, S, Dn, R = _fat_desc(ids, dense, W, dense_w, dim, "fatffm_pool_fwd", attn=[(pooled, "pooled")])
    if status is None:
        status = new_status(ids.device)
    check(lib().rec_fatffm_pool_fwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(dense_w), _p(pooled), _p(status),
                                    _stream()), "rec_fatffm_pool_fwd")
    return pooled, status


def fatffm_inter_fwd(ids, dense, W, dense_w, a, dim, status=None, out=None):
    """+ a [B, F*F] -> H [B, P*dim] (P = F(F-1)/2; or the wider-rowed matrix given as out[0]), y1 [B,1], status
    (rec_fatffm_inter_fwd)."""
    B, F = ids.shape[0], ids.shape[1] + dense.shape[1]
    H, y1 = out if out is not None else (None, None)
    H = _fat_out(H, B, F * (F - 1) // 2 * int(dim), ids.device)
    if y1 is None:
        y1 = torch.empty(B, 1, dtype=torch.float32, device=ids.device)
    _chk(y1, torch.float32, "y1")
    if y1.numel() != B:
        raise RecError("fatffm_inter_fwd: y1 must hold B values")
    desc, B, S, Dn, R = _fat_desc(ids, dense, W, dense_w, dim, "fatffm_inter_fwd", attn=[(a, "a")], pair=[(H, "H")])
    if status is None:
        status = new_status(ids.device)
    check(lib().rec_fatffm_inter_fwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(dense_w), _p(a), _p(H), _p(y1),
                                     _p(status), _stream()), "rec_fatffm_inter_fwd")
    return H, y1, status


def fatffm_attn_bwd(ids, dense, W, dense_w, a, dH, dz, dim, status=None, out=None):
    """+ dH [B, P*dim] = dloss / dH, dz [B]|[B,1] = dloss / dlogit -> d_a [B, F*F] (row stride of a), status
    (rec_fatffm_attn_bwd)."""
    B, F = ids.shape[0], ids.shape[1] + dense.shape[1]
    d_a = out if out is not None else torch.empty_like(a)
    _chk(dz, torch.float32, "dz")
    if dz.numel() != B:
        raise RecError("fatffm_attn_bwd: dz must hold B values")
    desc, B, S, Dn, R = _fat_desc(ids, dense, W, dense_w, dim, "fatffm_attn_bwd", attn=[(a, "a"), (d_a, "d_a")],
                                  pair=[(dH, "dH")])
    if status is None:
        status = new_status(ids.device)
    check(lib().rec_fatffm_attn_bwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(dense_w), _p(a), _p(dH), _p(dz),
                                    _p(d_a), _p(status), _stream()), "rec_fatffm_attn_bwd")
    return d_a, status


def fatffm_bwd(ids, dense, W, dense_w, a, dH, dz, d_pooled, dim, ws, out=None, status=None, grad_stride=None):
    """+ d_pooled [B, F*F] (row stride of a) -> row_grad [B*S, grad_stride] (default: R rounded up to 4 floats; the pad
    columns are 0), d_dense_w [Dn,R], status  (rec_fatffm_bwd)."""
    B, S = ids.shape
    Dn = dense.shape[1]
    R = (S + Dn) * int(dim)
    gs = int(grad_stride) if grad_stride else (R + 3) // 4 * 4
    _chk(dz, torch.float32, "dz")
    if dz.numel() != B:
        raise RecError("fatffm_bwd: dz must hold B values")
    desc, B, S, Dn, R = _fat_desc(ids, dense, W, dense_w, dim, "fatffm_bwd", attn=[(a, "a"), (d_pooled, "d_pooled")],
                                  pair=[(dH, "dH")], grad_stride=gs)
    dev = ids.device
    row_grad, d_dense_w = out if out is not None else (None, None)
    if row_grad is None:
        row_grad = torch.empty(B * S, gs, dtype=torch.float32, device=dev)
    if d_dense_w is None:
        d_dense_w = torch.empty(Dn, R, dtype=torch.float32, device=dev)
    _chk(row_grad, torch.float32, "row_grad", (B * S, gs))
    _chk(d_dense_w, torch.float32, "d_dense_w")
    if d_dense_w.numel() != Dn * R:
        raise RecError("fatffm_bwd: d_dense_w must hold Dn x R floats")
    if status is None:
        status = new_status(dev)
    nbytes = C.c_size_t(0)
    check(lib().rec_fatffm_bwd_workspace_bytes(C.byref(desc), C.byref(nbytes)), "rec_fatffm_bwd_workspace_bytes")
    w = ws.get(nbytes.value)
    check(lib().rec_fatffm_bwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(dense_w), _p(a), _p(dH), _p(dz),
                               _p(d_pooled), _p(row_grad), _p(d_dense_w), _p(w), C.c_size_t(w.numel()), _p(status),
                               _stream()), "rec_fatffm_bwd")
    return row_grad, d_dense_w, status


# ------------------------------------------------------------------ FEFM field-pair bilinear interaction (deepfefm)
def _fefm_desc(ids, dense, dim, W, what):
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2:
        raise RecError("%s: ids must be [B, S]" % what)
    B = ids.shape[0]
    _chk(dense, torch.float32, "dense")
    if dense.dim() != 2 or dense.shape[0] != B:
        raise RecError("%s: dense must be [B, Dn]" % what)
    width, stride = _chk_table(W, "W")
    if W.dim() != 2 or width < int(dim):
        raise RecError("%s: W rows hold %d floats, dim = %d" % (what, width, int(dim)))
    return B, dense.shape[1], stride


def _fefm_ld(t, B, cols, name):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.shape[0] != B or t.shape[1] < cols or \
            (t.shape[1] > 1 and t.stride(1) != 1):
        raise RecError("%s must be a float32 device matrix [B, >= %d] with unit column stride" % (name, cols))
    return t.stride(0) if B > 1 else max(t.stride(0), t.shape[1])


def fefm_fwd(ids, dense, W, W1, dense_w_one, FE, dim, ws, status=None, out=None):
    """ids [B,S] i64, dense [B,Dn] f32, W [N, >= dim] (a padded row stride is fine), W1 [N,1]|[N], dense_w_one [Dn],
    FE [P,dim,dim] (P = F(F-1)/2 pairs, F = S+Dn) -> y1 [B,1], y2 [B,1], dnn_in [B, S*dim+Dn+P] (or the wider buffer
    given as out[2]: its row stride is used), ids_all [B,F] i64, status  (rec_fefm_fwd)."""
    B, Dn, stride = _fefm_desc(ids, dense, dim, W, "fefm_fwd")
    S, D = ids.shape[1], int(dim)
    F = S + Dn
    P = F * (F - 1) // 2
    N = W.shape[0]
    _chk(W1, torch.float32, "W1")
    _chk(dense_w_one, torch.float32, "dense_w_one", (Dn,))
    _chk(FE, torch.float32, "FE", (P, D, D))
    if W1.numel() != N:
        raise RecError("fefm_fwd: W1 must hold one value per row of W")
    dev = ids.device
    cols = S * D + Dn + P
    if out is None:
        y1 = torch.empty(B, 1, dtype=torch.float32, device=dev)
        y2 = torch.empty(B, 1, dtype=torch.float32, device=dev)
        dnn_in = torch.empty(B, cols, dtype=torch.float32, device=dev)
        ids_all = torch.empty(B, F, dtype=torch.int64, device=dev)
    else:
        y1, y2, dnn_in, ids_all = out
        _chk(y1, torch.float32, "y1")
        _chk(y2, torch.float32, "y2")
        _chk(ids_all, torch.int64, "ids_all", (B, F))
        if y1.numel() != B or y2.numel() != B:
            raise RecError("fefm_fwd: y1 / y2 must hold B values")
    ld = _fefm_ld(dnn_in, B, cols, "dnn_in")
    if status is None:
        status = new_status(dev)
    desc = FEFMDesc(B, S, Dn, D, N, stride, 0, ld)
    nbytes = C.c_size_t(0)
    check(lib().rec_fefm_fwd_workspace_bytes(C.byref(desc), C.byref(nbytes)), "rec_fefm_fwd_workspace_bytes")
    w = ws.get(nbytes.value)
    check(lib().rec_fefm_fwd(C.byref(desc), _p(ids), _p(dense), _p(W), _p(W1), _p(dense_w_one), _p(FE), _p(y1), _p(y2),
                             _p(dnn_in), _p(ids_all), _p(w), C.c_size_t(w.numel()), _p(status), _stream()),
          "rec_fefm_fwd")
    return y1, y2, dnn_in, ids_all, status


def fefm_bwd(ids_all, dense, W, FE, dz, d_dnn_in, num_slots, dim, ws, want_d_fe=False, out=None, status=None,
             grad_stride=None):
    """ids_all [B,F] i64 (from fefm_fwd), dz [B]|[B,1] = dloss / dlogit, d_dnn_in [B, >= S*dim+Dn+P] = dloss / d dnn_in
    -> row_grad [B*F, grad_stride] (default: dim rounded up to 4 floats; pad columns and padding positions are 0),
    d_dense_w_one [Dn], d_FE [P,dim,dim] or None (want_d_fe False: that work is skipped)  (rec_fefm_bwd).  The W1
    gradient is dz itself, read with grad_div = S over a grouping of the sparse ids [B,S]."""
    B, Dn, stride = _fefm_desc(ids_all, dense, dim, W, "fefm_bwd")
    F, D, S = ids_all.shape[1], int(dim), int(num_slots)
    if S + Dn != F:
        raise RecError("fefm_bwd: ids_all has %d fields, num_slots + Dn = %d" % (F, S + Dn))
    P = F * (F - 1) // 2
    _chk(FE, torch.float32, "FE", (P, D, D))
    _chk(dz, torch.float32, "dz")
    if dz.numel() != B:
        raise RecError("fefm_bwd: dz must hold B values")
    ld = _fefm_ld(d_dnn_in, B, S * D + Dn + P, "d_dnn_in")
    gs = int(grad_stride) if grad_stride else (D + 3) // 4 * 4
    dev = ids_all.device
    if out is None:
        row_grad = torch.empty(B * F, gs, dtype=torch.float32, device=dev)
        d_dense_w_one = torch.empty(Dn, dtype=torch.float32, device=dev)
        d_FE = torch.empty(P, D, D, dtype=torch.float32, device=dev) if want_d_fe else None
    else:
        row_grad, d_dense_w_one, d_FE = out
        if not want_d_fe:
            d_FE = None
    _chk(row_grad, torch.float32, "row_grad", (B * F, gs))
    _chk(d_dense_w_one, torch.float32, "d_dense_w_one", (Dn,))
    if want_d_fe:
        if d_FE is None:
            raise RecError("fefm_bwd: want_d_fe needs a d_FE tensor in out")
        _chk(d_FE, torch.float32, "d_FE", (P, D, D))
    desc = FEFMDesc(B, S, Dn, D, W.shape[0], stride, gs, ld)
    nbytes = C.c_size_t(0)
    check(lib().rec_fefm_bwd_workspace_bytes(C.byref(desc), int(bool(want_d_fe)), C.byref(nbytes)),
          "rec_fefm_bwd_workspace_bytes")
    w = ws.get(nbytes.value)
    check(lib().rec_fefm_bwd(C.byref(desc), _p(ids_all), _p(dense), _p(W), _p(FE), _p(dz), _p(d_dnn_in), _p(row_grad),
                             _p(d_dense_w_one), _p(d_FE), _p(w), C.c_size_t(w.numel()), _p(status), _stream()),
          "rec_fefm_bwd")
    return row_grad, d_dense_w_one, d_FE


# ------------------------------------------------------------------ DCN vector-form cross network (rank/dcn)
def _dcn_rows(t, B, d, name):
    """A [B, d] float32 device matrix with unit column stride (a column block of a wider buffer is fine) -> row stride."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or \
            tuple(t.shape) != (B, d) or (d > 1 and t.stride(1) != 1):
        raise RecError("%s must be a float32 device matrix [%d, %d] with unit column stride" % (name, B, d))
    ld = t.stride(0) if B > 1 else max(t.stride(0), d)
    if ld < d:
        raise RecError("%s: row stride %d < d %d" % (name, ld, d))
    return ld


def _dcn_vec(t, d, name):
    _chk(t, torch.float32, name)
    if t.numel() != d:
        raise RecError("%s must hold d = %d floats" % (name, d))


def dcn_cross_fwd(x0, w, b, num_layers, ws, l2_coeff=1.0, want_saved=True, want_l2=True, out=None):
    """The whole cross stack of dcn/net.py:117-135 in one pass (rec_dcn_cross_fwd): x0 [B,d] (rows may be strided), w / b
    [d] shared by the num_layers layers -> (x_L [B,d], saved [B,L] = the per-row scalars s_l = <x_l, w> or None,
    l2 [1] = l2_coeff * sum_l sum (x_l * w)^2 or None).  want_saved / want_l2 False: the inference form, nothing is
    stored or summed for them.  out = (x_L, saved, l2): x_L may be a column block of a wider buffer."""
    if x0.dim() != 2:
        raise RecError("dcn_cross_fwd: x0 must be [B, d]")
    B, d = x0.shape
    L = int(num_layers)
    ld_x0 = _dcn_rows(x0, B, d, "x0")
    _dcn_vec(w, d, "w")
    _dcn_vec(b, d, "b")
    dev = x0.device
    xl, saved, l2 = out if out is not None else (None, None, None)
    if xl is None:
        xl = torch.empty(B, d, dtype=torch.float32, device=dev)
    ld_out = _dcn_rows(xl, B, d, "x_L")
    if want_saved:
        if saved is None:
            saved = torch.empty(B, max(L, 0), dtype=torch.float32, device=dev)
        _chk(saved, torch.float32, "saved", (B, L))
    else:
        saved = None
    if want_l2:
        if l2 is None:
            l2 = torch.empty(1, dtype=torch.float32, device=dev)
        _chk(l2, torch.float32, "l2", (1,))
        if B == 0:
            l2.zero_()
    else:
        l2 = None
    desc = DcnCrossDesc(B, d, L, ld_x0, ld_out, 0, 0, float(l2_coeff), 0)
    wk = None
    if want_l2:
        nbytes = C.c_size_t(0)
        check(lib().rec_dcn_cross_bwd_workspace_bytes(C.byref(desc), C.byref(nbytes)), "rec_dcn_cross_bwd_workspace_bytes")
        wk = ws.get(nbytes.value)
    check(lib().rec_dcn_cross_fwd(C.byref(desc), _p(x0), _p(w), _p(b), _p(xl), _p(saved), _p(l2), _p(wk),
                                  C.c_size_t(wk.numel() if wk is not None else 0), _stream()), "rec_dcn_cross_fwd")
    return xl, saved, l2


def dcn_cross_bwd(x0, w, b, saved, dxl, ws, l2_coeff=1.0, accumulate=False, out=None, dz=None, u=None):
    """Backward of dcn_cross_fwd and of its l2 term (rec_dcn_cross_bwd): dxl [B,d] = dloss / d x_L (rows may be strided)
    -> (dx0 [B,d], d_w [d], d_b [d]).  out = (dx0, d_w, d_b); accumulate=True adds into out[0] (required then) instead
    of writing it.  Rank-1 form: dxl=None with dz [B]|[B,1] and u [d] reads the upstream gradient as dz[r] * u[k]."""
    if x0.dim() != 2:
        raise RecError("dcn_cross_bwd: x0 must be [B, d]")
    B, d = x0.shape
    ld_x0 = _dcn_rows(x0, B, d, "x0")
    _dcn_vec(w, d, "w")
    _dcn_vec(b, d, "b")
    _chk(saved, torch.float32, "saved")
    if saved.dim() != 2 or saved.shape[0] != B:
        raise RecError("dcn_cross_bwd: saved must be [B, L]")
    L = saved.shape[1]
    ld_dxl = 0
    if dxl is not None:
        ld_dxl = _dcn_rows(dxl, B, d, "dxl")
        dz = u = None
    else:
        if dz is None or u is None:
            raise RecError("dcn_cross_bwd: give dxl, or dz and u (the rank-1 form)")
        _chk(dz, torch.float32, "dz")
        if dz.numel() != B:
            raise RecError("dcn_cross_bwd: dz must hold B values")
        _dcn_vec(u, d, "u")
    dev = x0.device
    dx0, d_w, d_b = out if out is not None else (None, None, None)
    if dx0 is None:
        if accumulate:
            raise RecError("dcn_cross_bwd: accumulate=True needs the buffer to add into as out[0]")
        dx0 = torch.empty(B, d, dtype=torch.float32, device=dev)
    ld_dx0 = _dcn_rows(dx0, B, d, "dx0")
    if d_w is None:
        d_w = torch.empty(d, dtype=torch.float32, device=dev)
    if d_b is None:
        d_b = torch.empty(d, dtype=torch.float32, device=dev)
    _dcn_vec(d_w, d, "d_w")
    _dcn_vec(d_b, d, "d_b")
    if B == 0:
        d_w.zero_()
        d_b.zero_()
    desc = DcnCrossDesc(B, d, L, ld_x0, 0, ld_dxl, ld_dx0, float(l2_coeff), int(bool(accumulate)))
    nbytes = C.c_size_t(0)
    check(lib().rec_dcn_cross_bwd_workspace_bytes(C.byref(desc), C.byref(nbytes)), "rec_dcn_cross_bwd_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_dcn_cross_bwd(C.byref(desc), _p(x0), _p(w), _p(b), _p(saved), _p(dxl), _p(dz), _p(u), _p(dx0), _p(d_w),
                                  _p(d_b), _p(wk), C.c_size_t(wk.numel()), _stream()), "rec_dcn_cross_bwd")
    return dx0, d_w, d_b


# ------------------------------------------------------------------ FLEN field-wise bi-interaction (rank/flen)
def _span(t):
    """[first byte, one past the last byte) a 2-D view touches."""
    n = ((t.shape[0] - 1) * t.stride(0) + (t.shape[1] - 1) * t.stride(1) + 1) if t.numel() else 0
    return t.data_ptr(), t.data_ptr() + 4 * n


def _overlap(a, b):
    (a0, a1), (b0, b1) = _span(a), _span(b)
    return a0 < b1 and b0 < a1


def _flen_args(ids, group_begin, kernel_mf, what):
    """Checks shared by flen_fwd / flen_bwd -> (B, S, G, the bounds as a C int32 array)."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[1] < 2:
        raise RecError("%s: ids must be [B, S] with S >= 2" % what)
    B, S = ids.shape
    try:
        gb = [int(x) for x in group_begin]
    except TypeError:
        raise RecError("%s: group_begin must be a sequence of G + 1 ints" % what)
    G = len(gb) - 1
    if not 2 <= G <= _lib.REC_FLEN_MAX_GROUPS:
        raise RecError("%s: group_begin must hold G + 1 bounds for 2 <= G <= %d groups, got %d values"
                       % (what, _lib.REC_FLEN_MAX_GROUPS, len(gb)))
    if gb[0] != 0 or gb[-1] != S or any(a >= b for a, b in zip(gb, gb[1:])):
        raise RecError("%s: group_begin %s must rise strictly from 0 to S = %d" % (what, gb, S))
    _chk(kernel_mf, torch.float32, "kernel_mf")
    if kernel_mf is None or kernel_mf.numel() != G * (G - 1) // 2:
        raise RecError("%s: kernel_mf must hold G (G - 1) / 2 = %d floats" % (what, G * (G - 1) // 2))
    return B, S, G, (C.c_int32 * (G + 1))(*gb)


def flen_fwd(ids, W, group_begin, kernel_mf, status=None, out=None):
    """Lookup + field-wise bi-interaction in one pass (rec_flen_fwd): ids [B,S] i64, W [N,D] (rows may be strided),
    group_begin the G + 1 slot bounds of the field groups (host ints), kernel_mf [P] -> X0 [B, S*D] (the lookups side by
    side), h_mf [B, D] = sum over group pairs of kernel_mf[p] * FW_i * FW_j, FW [B, G*D] (the group sums, contiguous: the
    backward reads it).  out = (X0, h_mf, FW), new tensors where None; X0 and h_mf may be column blocks of wider buffers
    (unit column stride; the rest of a row is not touched).  -> (X0, h_mf, FW, status)."""
    B, S, G, gb = _flen_args(ids, group_begin, kernel_mf, "flen_fwd")
    _, w_stride = _chk_table(W, "W")
    if W.dim() != 2:
        raise RecError("flen_fwd: W must be [N, D]")
    N, D = W.shape
    X0, H, FW = out if out is not None else (None, None, None)
    dev = ids.device
    if X0 is None:
        X0 = torch.empty(B, S * D, dtype=torch.float32, device=dev)
    if H is None:
        H = torch.empty(B, D, dtype=torch.float32, device=dev)
    if FW is None:
        FW = torch.empty(B, G * D, dtype=torch.float32, device=dev)
    ld_x, ld_h = _dcn_rows(X0, B, S * D, "X0"), _dcn_rows(H, B, D, "h_mf")
    _chk(FW, torch.float32, "FW", (B, G * D))
    if _overlap(X0, H) or _overlap(X0, FW) or _overlap(H, FW):
        raise RecError("flen_fwd: X0, h_mf and FW must not overlap")
    if status is None:
        status = new_status(dev)
    check(lib().rec_flen_fwd(B, S, G, D, w_stride, N, _p(ids), _p(W), gb, _p(kernel_mf), _p(X0), ld_x, _p(H), ld_h,
                             _p(FW), _p(status), _stream()), "rec_flen_fwd")
    return X0, H, FW, status


def flen_bwd(ids, num_rows, group_begin, kernel_mf, FW, dH, g, ws, status=None, out=None):
    """Backward of flen_fwd IN PLACE and without the table (rec_flen_bwd): g [B, S*D] (a view as X0 there) holds
    dloss / d X0 on entry and the per-lookup row gradient on return; dH [B, D] = dloss / d h_mf, FW the forward's.
    -> (g, d_kernel_mf [P] = out or a new tensor, status).  d_kernel_mf is a fixed-order sum: reruns are bit-identical."""
    B, S, G, gb = _flen_args(ids, group_begin, kernel_mf, "flen_bwd")
    P = G * (G - 1) // 2
    if int(num_rows) < 1:
        raise RecError("flen_bwd: num_rows must be >= 1")
    if not torch.is_tensor(dH) or dH.dim() != 2:
        raise RecError("flen_bwd: dH must be a float32 device matrix [B, D]")
    D = dH.shape[1]
    ld_dh, ld_g = _dcn_rows(dH, B, D, "dH"), _dcn_rows(g, B, S * D, "g")
    _chk(FW, torch.float32, "FW", (B, G * D))
    if _overlap(g, FW) or _overlap(g, dH):
        raise RecError("flen_bwd: g must not overlap FW or dH")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=ids.device)
    _chk(out, torch.float32, "d_kernel_mf")
    if out.numel() != P:
        raise RecError("flen_bwd: d_kernel_mf must hold P = %d floats" % P)
    if status is None:
        status = new_status(ids.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_flen_bwd_workspace_bytes(B, S, G, D, C.byref(nbytes)), "rec_flen_bwd_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_flen_bwd(B, S, G, D, int(num_rows), _p(ids), gb, _p(kernel_mf), _p(FW), _p(dH), ld_dh, _p(g), ld_g,
                             _p(out), _p(status), _p(wk), C.c_size_t(wk.numel()), _stream()), "rec_flen_bwd")
    return g, out, status


# ------------------------------------------------------------------ AutoFIS gated pair term (rank/autofis)
class AutofisPairs:
    """A pair list of AutoFIS, checked once: cols / rows (host int32 arrays, 0 <= cols[p] < rows[p] < num_fields) and the
    device image rec_autofis_plan lays out from them (cols | rows | the per-field adjacency of the backward)."""

    def __init__(self, cols, rows, num_fields, device):
        try:
            c, r = [int(x) for x in cols], [int(x) for x in rows]
        except TypeError:
            raise RecError("autofis: cols and rows must be sequences of ints")
        S, P = int(num_fields), len(c)
        if len(r) != P:
            raise RecError("autofis: cols and rows must have one length (%d, %d)" % (P, len(r)))
        if not 2 <= S <= _lib.REC_AUTOFIS_MAX_FIELDS:
            raise RecError("autofis: num_fields %d must be 2 .. %d" % (S, _lib.REC_AUTOFIS_MAX_FIELDS))
        if not 1 <= P <= min(_lib.REC_AUTOFIS_MAX_PAIRS, S * (S - 1) // 2):
            raise RecError("autofis: %d pairs; must be 1 .. min(%d, num_fields (num_fields - 1) / 2 = %d)"
                           % (P, _lib.REC_AUTOFIS_MAX_PAIRS, S * (S - 1) // 2))
        for p, (a, b) in enumerate(zip(c, r)):
            if not 0 <= a < b < S:
                raise RecError("autofis: pair %d = (%d, %d) must satisfy 0 <= col < row < num_fields = %d" % (p, a, b, S))
        self.num_fields, self.n = S, P
        self.cols, self.rows = (C.c_int32 * P)(*c), (C.c_int32 * P)(*r)
        n = C.c_size_t(0)
        check(lib().rec_autofis_plan_ints(S, P, C.byref(n)), "rec_autofis_plan_ints")
        host = (C.c_int32 * n.value)()
        check(lib().rec_autofis_plan(S, P, self.cols, self.rows, host), "rec_autofis_plan")
        self.plan = torch.tensor(list(host), dtype=torch.int32, device=device)


def _autofis_args(pairs, gamma, beta, mask, what):
    if not isinstance(pairs, AutofisPairs):
        raise RecError("%s: pairs must be an ops.AutofisPairs" % what)
    P = pairs.n
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (mask, "mask")):
        if not torch.is_tensor(t):
            raise RecError("%s: %s must be a float32 device tensor" % (what, nm))
        _chk(t, torch.float32, nm)
        if t.numel() != P:
            raise RecError("%s: %s must hold P = %d floats" % (what, nm, P))
    return P


def autofis_fwd(ids, V, W1, pairs, gamma, beta, mask, running_mean, running_var, ws, training=True, momentum=0.9,
                eps=1e-5, want_L=False, status=None, out=None):
    """Lookup + gated, batch-normalised pair term in one pass (rec_autofis_fwd): ids [B,S] i64, V [N,D] and W1 [N] or
    [N,1] (rows may be strided), pairs an AutofisPairs, gamma / beta / mask [P] and the running statistics [P] of the pair
    BatchNorm -> (X0 [B, S*D], s [B] = sum_s W1[ids] + sum_p mask_p BN_p(L)[b], L [B,P] or None, save_mean, save_invstd
    (None in eval mode), status).  training: batch statistics, the running ones move, L is written; eval: the running
    statistics, L only with want_L.  out = (X0, L): column blocks of wider buffers are fine (unit column stride)."""
    P = _autofis_args(pairs, gamma, beta, mask, "autofis_fwd")
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[1] != pairs.num_fields:
        raise RecError("autofis_fwd: ids must be [B, S = %d]" % pairs.num_fields)
    B, S = ids.shape
    _, v_stride = _chk_table(V, "V")
    if V.dim() != 2 or not 1 <= V.shape[1] <= _lib.REC_AUTOFIS_MAX_DIM:
        raise RecError("autofis_fwd: V must be [N, D] with 1 <= D <= %d" % _lib.REC_AUTOFIS_MAX_DIM)
    N, D = V.shape
    w_dim, w_stride = _chk_table(W1, "W1")
    if w_dim != 1 or W1.shape[0] != N:
        raise RecError("autofis_fwd: W1 must be [N] or [N, 1] with the rows of V")
    for t, nm in ((running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, torch.float32, nm, (P,))
    dev = ids.device
    X0, L = out if out is not None else (None, None)
    if X0 is None:
        X0 = torch.empty(B, S * D, dtype=torch.float32, device=dev)
    writes_L = bool(training) or bool(want_L)
    if L is None and writes_L:
        L = torch.empty(B, P, dtype=torch.float32, device=dev)
    ld_x = _dcn_rows(X0, B, S * D, "X0")
    ld_l = _dcn_rows(L, B, P, "L") if writes_L else 0
    if writes_L and _overlap(X0, L):
        raise RecError("autofis_fwd: X0 and L must not overlap")
    s = torch.empty(B, dtype=torch.float32, device=dev)
    sm = si = None
    if training:
        sm = torch.empty(P, dtype=torch.float32, device=dev)
        si = torch.empty(P, dtype=torch.float32, device=dev)
    if status is None:
        status = new_status(dev)
    nbytes = C.c_size_t(0)
    check(lib().rec_autofis_fwd_workspace_bytes(B, S, D, P, C.byref(nbytes)), "rec_autofis_fwd_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_autofis_fwd(B, S, D, v_stride, w_stride, N, _p(ids), _p(V), _p(W1), P, pairs.cols, pairs.rows,
                                _p(pairs.plan), _p(gamma), _p(beta), _p(mask), _p(running_mean), _p(running_var),
                                float(momentum), float(eps), int(bool(training)), int(bool(want_L)), _p(X0), ld_x,
                                _p(L if writes_L else None), ld_l, _p(s), _p(sm), _p(si), _p(status), _p(wk),
                                C.c_size_t(wk.numel()), _stream()), "rec_autofis_fwd")
    return X0, s, (L if writes_L else None), sm, si, status


def autofis_bwd(dz, L, X0, pairs, save_mean, save_invstd, gamma, beta, mask, dX, ws, out=None):
    """Backward of the training autofis_fwd (rec_autofis_bwd): dz [B] or [B,1] = dloss / d s; dX [B, S*D] (a view as X0)
    holds the DNN's layer-0 gradient on entry and gets the pair term's gradient ADDED in place (a field in no pair is not
    written).  -> (dX, d_mask [P], d_gamma [P], d_beta [P]); out = the three gradients.  Fixed-order sums."""
    P = _autofis_args(pairs, gamma, beta, mask, "autofis_bwd")
    S = pairs.num_fields
    if not torch.is_tensor(dz):
        raise RecError("autofis_bwd: dz must be a float32 device tensor")
    _chk(dz, torch.float32, "dz")
    B = dz.numel()
    if not torch.is_tensor(X0) or X0.dim() != 2 or X0.shape[1] % S:
        raise RecError("autofis_bwd: X0 must be a float32 device matrix [B, S * D]")
    D = X0.shape[1] // S
    if not 1 <= D <= _lib.REC_AUTOFIS_MAX_DIM:
        raise RecError("autofis_bwd: D = %d must be 1 .. %d" % (D, _lib.REC_AUTOFIS_MAX_DIM))
    ld_x, ld_l, ld_dx = _dcn_rows(X0, B, S * D, "X0"), _dcn_rows(L, B, P, "L"), _dcn_rows(dX, B, S * D, "dX")
    if _overlap(dX, X0) or _overlap(dX, L):
        raise RecError("autofis_bwd: dX must not overlap X0 or L")
    for t, nm in ((save_mean, "save_mean"), (save_invstd, "save_invstd")):
        _chk(t, torch.float32, nm, (P,))
    dev = dz.device
    d_mask, d_gamma, d_beta = out if out is not None else (None, None, None)
    made = []
    for t, nm in ((d_mask, "d_mask"), (d_gamma, "d_gamma"), (d_beta, "d_beta")):
        if t is None:
            t = torch.empty(P, dtype=torch.float32, device=dev)
        _chk(t, torch.float32, nm)
        if t.numel() != P:
            raise RecError("autofis_bwd: %s must hold P = %d floats" % (nm, P))
        made.append(t)
    d_mask, d_gamma, d_beta = made
    nbytes = C.c_size_t(0)
    check(lib().rec_autofis_bwd_workspace_bytes(B, S, D, P, C.byref(nbytes)), "rec_autofis_bwd_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_autofis_bwd(B, S, D, P, pairs.cols, pairs.rows, _p(pairs.plan), _p(dz), _p(L), ld_l, _p(X0), ld_x,
                                _p(save_mean), _p(save_invstd), _p(gamma), _p(beta), _p(mask), _p(dX), ld_dx, _p(d_mask),
                                _p(d_gamma), _p(d_beta), _p(wk), C.c_size_t(wk.numel()), _stream()), "rec_autofis_bwd")
    return dX, d_mask, d_gamma, d_beta


def batchnorm_relu_fwd(X, gamma, beta, running_mean, running_var, ws, training=True, momentum=0.9, eps=1e-5, out=None):
    """relu(BatchNorm(X)) for Linear -> BN -> ReLU (autofis/net.py:84-88): batchnorm_fwd with the ReLU in its apply pass.
    -> (Y, save_mean, save_invstd).  Y is not X: batchnorm_relu_bwd reads both."""
    ldx = _chk_mat(X, "X")
    m, n = X.shape
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, torch.float32, nm, (n,))
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=X.device)
    ldy = _chk_mat(out, "out")
    if tuple(out.shape) != (m, n) or _overlap(out, X):
        raise RecError("batchnorm_relu_fwd: out must be [m, n] and must not overlap X")
    sm = torch.empty(n, dtype=torch.float32, device=X.device)
    si = torch.empty(n, dtype=torch.float32, device=X.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_batchnorm_workspace_bytes(m, n, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_batchnorm_relu_fwd(m, n, _p(X), ldx, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                       float(momentum), float(eps), int(bool(training)), _p(out), ldy, _p(sm), _p(si),
                                       _p(w), C.c_size_t(w.numel()), _stream()), "rec_batchnorm_relu_fwd")
    return out, sm, si


def batchnorm_relu_bwd(X, Y, dY, gamma, save_mean, save_invstd, ws, dgamma=None, dbeta=None, out=None):
    """Backward of batchnorm_relu_fwd: dY counts only where Y > 0, in the column sums and in dX.
    -> (dX, dgamma, dbeta)."""
    ldx, ldy, lddy = _chk_mat(X, "X"), _chk_mat(Y, "Y"), _chk_mat(dY, "dY")
    m, n = X.shape
    if tuple(Y.shape) != (m, n) or tuple(dY.shape) != (m, n):
        raise RecError("batchnorm_relu_bwd: X, Y and dY must have one shape")
    dev = X.device
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=dev)
    if tuple(out.shape) != (m, n) or _overlap(out, X) or _overlap(out, Y):
        raise RecError("batchnorm_relu_bwd: dX must be [m, n] and must not overlap X or Y")
    if dgamma is None:
        dgamma = torch.empty(n, dtype=torch.float32, device=dev)
    if dbeta is None:
        dbeta = torch.empty(n, dtype=torch.float32, device=dev)
    for t, nm in ((gamma, "gamma"), (save_mean, "save_mean"), (save_invstd, "save_invstd"), (dgamma, "dgamma"),
                  (dbeta, "dbeta")):
        _chk(t, torch.float32, nm, (n,))
    nbytes = C.c_size_t(0)
    check(lib().rec_batchnorm_workspace_bytes(m, n, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_batchnorm_relu_bwd(m, n, _p(X), ldx, _p(Y), ldy, _p(dY), lddy, _p(gamma), _p(save_mean),
                                       _p(save_invstd), _p(out), _chk_mat(out, "dX"), _p(dgamma), _p(dbeta), _p(w),
                                       C.c_size_t(w.numel()), _stream()), "rec_batchnorm_relu_bwd")
    return out, dgamma, dbeta


def grda_step(p, acc, g, lr, l1_accumulation, first_iter):
    """SimpleGrda.step() on one parameter (rec_grda_step): acc += first_iter * p - lr * g; p = sign(acc) * max(|acc| -
    l1_accumulation, 0).  p, acc, g contiguous float32 of one length; the caller keeps iterations and l1_accumulation."""
    for t, n in ((p, "p"), (acc, "acc"), (g, "g")):
        if not torch.is_tensor(t):
            raise RecError("%s must be a float32 device tensor" % n)
        _chk(t, torch.float32, n)
    if not (p.numel() == acc.numel() == g.numel()):
        raise RecError("p, acc and g must have one length (%d, %d, %d)" % (p.numel(), acc.numel(), g.numel()))
    if first_iter not in (0, 1) or not float(l1_accumulation) >= 0.0:
        raise RecError("grda_step: first_iter must be 0 or 1 and l1_accumulation >= 0")
    check(lib().rec_grda_step(p.numel(), _p(p), _p(acc), _p(g), float(lr), float(l1_accumulation), int(first_iter),
                              _stream()), "rec_grda_step")


# ------------------------------------------------------------------ GateNet gates (rank/gatenet)
def _gate_emb_args(ids, W, gate_w, what):
    """Checks shared by gate_emb_fwd / gate_emb_bwd -> (B, S, D, table row stride, N)."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[1] < 1:
        raise RecError("%s: ids must be [B, S]" % what)
    B, S = ids.shape
    _, w_stride = _chk_table(W, "W")
    if W.dim() != 2:
        raise RecError("%s: W must be [N, D]" % what)
    N, D = W.shape
    _chk(gate_w, torch.float32, "gate_w")
    if gate_w.numel() != S:
        raise RecError("%s: gate_w must hold S = %d floats (one scalar per field)" % (what, S))
    return B, S, D, w_stride, N


def gate_emb_fwd(ids, W, gate_w, padding_idx=None, status=None, out=None):
    """Lookup + embedding gate in one pass (rec_gate_emb_fwd): ids [B,S] i64, W [N,D] (rows may be strided), gate_w [S]
    -> out [B, S*D] with out[b, s*D:(s+1)*D] = e * sigmoid(gate_w[s] * sum(e)), e = W[ids[b,s]].  out may be the head
    columns of a wider feature buffer (unit column stride; the rest of a row is not touched).  -> (out, status)."""
    B, S, D, w_stride, N = _gate_emb_args(ids, W, gate_w, "gate_emb_fwd")
    if out is None:
        out = torch.empty(B, S * D, dtype=torch.float32, device=ids.device)
    ld = _dcn_rows(out, B, S * D, "out")
    if status is None:
        status = new_status(ids.device)
    check(lib().rec_gate_emb_fwd(B * S, S, D, w_stride, N, -1 if padding_idx is None else padding_idx, _p(ids), _p(W),
                                 _p(gate_w), _p(out), ld, _p(status), _stream()), "rec_gate_emb_fwd")
    return out, status


def gate_emb_bwd(ids, W, gate_w, g, ws, padding_idx=None, status=None, out=None):
    """Backward of gate_emb_fwd IN PLACE (rec_gate_emb_bwd): g [B, S*D] (a view as `out` there) holds dloss / d out on
    entry and dloss / d e on return; W must still hold the forward's rows.  -> (g, d_gate_w [S] = out or a new tensor,
    status).  d_gate_w is a fixed-order sum: reruns are bit-identical."""
    B, S, D, w_stride, N = _gate_emb_args(ids, W, gate_w, "gate_emb_bwd")
    ld = _dcn_rows(g, B, S * D, "g")
    if out is None:
        out = torch.empty(S, dtype=torch.float32, device=ids.device)
    _chk(out, torch.float32, "d_gate_w")
    if out.numel() != S:
        raise RecError("gate_emb_bwd: d_gate_w must hold S = %d floats" % S)
    if status is None:
        status = new_status(ids.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_gate_emb_bwd_workspace_bytes(B * S, S, C.byref(nbytes)), "rec_gate_emb_bwd_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_gate_emb_bwd(B * S, S, D, w_stride, N, -1 if padding_idx is None else padding_idx, _p(ids), _p(W),
                                 _p(gate_w), _p(g), ld, _p(out), _p(status), _p(wk), C.c_size_t(wk.numel()), _stream()),
          "rec_gate_emb_bwd")
    return g, out, status


def _gate_rows(ts, what):
    """Float32 device matrices of ONE shape [B, n] with unit column stride -> (B, n, their row strides)."""
    B, n = ts[0][0].shape if torch.is_tensor(ts[0][0]) and ts[0][0].dim() == 2 else (-1, -1)
    if B < 0 or n < 1:
        raise RecError("%s: %s must be a matrix [B, n] with n >= 1" % (what, ts[0][1]))
    return B, n, [_dcn_rows(t, B, n, name) for t, name in ts]


def gate_hidden_fwd(y, t, out=None):
    """x = y * tanh(t) for t = y @ G (rec_gate_hidden_fwd); t is overwritten with h = tanh(t).  -> (x, h)."""
    if out is None:
        out = torch.empty(tuple(y.shape), dtype=torch.float32, device=y.device) if torch.is_tensor(y) else None
    B, n, (ld_y, ld_t, ld_x) = _gate_rows([(y, "y"), (t, "t"), (out, "x")], "gate_hidden_fwd")
    check(lib().rec_gate_hidden_fwd(B, n, _p(y), ld_y, _p(t), ld_t, _p(out), ld_x, _stream()), "rec_gate_hidden_fwd")
    return out, t


def gate_hidden_bwd(u, y, h, out=None):
    """Upstream u = dloss / d x, the forward's y and h -> (dt = u * y * (1 - h^2), uh = u * h) (rec_gate_hidden_bwd).
    out = (dt, uh), new tensors where None."""
    dt, uh = out if out is not None else (None, None)
    if torch.is_tensor(u) and u.dim() == 2:
        if dt is None:
            dt = torch.empty(tuple(u.shape), dtype=torch.float32, device=u.device)
        if uh is None:
            uh = torch.empty(tuple(u.shape), dtype=torch.float32, device=u.device)
    B, n, ld = _gate_rows([(u, "u"), (y, "y"), (h, "h"), (dt, "dt"), (uh, "uh")], "gate_hidden_bwd")
    check(lib().rec_gate_hidden_bwd(B, n, _p(u), ld[0], _p(y), ld[1], _p(h), ld[2], _p(dt), ld[3], _p(uh), ld[4],
                                    _stream()), "rec_gate_hidden_bwd")
    return dt, uh


def relu_mask_(dy, y):
    """dy *= (y > 0) in place (rec_relu_mask_inplace); floats between the rows of a strided dy keep their values."""
    B, n, (ld_dy, ld_y) = _gate_rows([(dy, "dy"), (y, "y")], "relu_mask_")
    check(lib().rec_relu_mask_inplace(B, n, _p(dy), ld_dy, _p(y), ld_y, _stream()), "rec_relu_mask_inplace")
    return dy


def dense_fold_fwd(S, dense_w, W0, M):
    """M[j,:] = dense_w[j,:] @ W0[(S+j)*D:(S+j+1)*D, :]   (dense embeddings folded into MLP layer 0)."""
    Dn, D = dense_w.shape[-2], dense_w.shape[-1]
    for t, n in ((dense_w, "dense_w"), (W0, "W0")):
        _chk(t, torch.float32, n)
    if not M.is_cuda or M.dtype != torch.float32 or not M.is_contiguous() or tuple(M.shape) != (Dn, W0.shape[1]):
        raise RecError("M must be a contiguous float32 device tensor [Dn, n_out]")
    check(lib().rec_dense_fold_fwd(int(S), Dn, D, W0.shape[1], _p(dense_w), _p(W0), _p(M), _stream()),
          "rec_dense_fold_fwd")
    return M


def dense_fold_bwd(S, dense_w, W0, dM, dW0, d_dense_w, accumulate=True):
    """dW0 dense rows = dense_w (x) dM;  d_dense_w (+)= dM @ W0_dense^T."""
    Dn, D = dense_w.shape[-2], dense_w.shape[-1]
    for t, n in ((dense_w, "dense_w"), (W0, "W0"), (dM, "dM"), (dW0, "dW0"), (d_dense_w, "d_dense_w")):
        _chk(t, torch.float32, n)
    check(lib().rec_dense_fold_bwd(int(S), Dn, D, W0.shape[1], _p(dense_w), _p(W0), _p(dM), _p(dW0),
                                   _p(d_dense_w), int(accumulate), _stream()), "rec_dense_fold_bwd")


def dense_fold_fwd_full(S, dense_w, W0, W0_folded):
    """W0_folded [(S+1)*D, n_out]: sparse rows of W0 + the folded dense rows M, one launch."""
    Dn, D = dense_w.shape[-2], dense_w.shape[-1]
    for t, n in ((dense_w, "dense_w"), (W0, "W0"), (W0_folded, "W0_folded")):
        _chk(t, torch.float32, n)
    if tuple(W0_folded.shape) != ((S + 1) * D, W0.shape[1]) or W0.shape[0] != (S + Dn) * D or Dn > D:
        raise RecError("W0 must be [(S+Dn)*D, n_out] and W0_folded [(S+1)*D, n_out] with Dn <= D")
    check(lib().rec_dense_fold_fwd_full(int(S), Dn, D, W0.shape[1], _p(dense_w), _p(W0), _p(W0_folded), _stream()),
          "rec_dense_fold_fwd_full")
    return W0_folded


def dense_fold_bwd_full(S, dense_w, W0, dW0_folded, dW0, d_dense_w, accumulate=True):
    """dW0_folded = feat'^T dZ0 [(S+1)*D, n_out] (scratch) -> dW0 (sparse rows copied, dense rows = dense_w (x) dM) and
    d_dense_w (+)= dM @ W0_dense^T, one launch."""
    Dn, D = dense_w.shape[-2], dense_w.shape[-1]
    for t, n in ((dense_w, "dense_w"), (W0, "W0"), (dW0_folded, "dW0_folded"), (dW0, "dW0"), (d_dense_w, "d_dense_w")):
        _chk(t, torch.float32, n)
    if (tuple(dW0_folded.shape) != ((S + 1) * D, W0.shape[1]) or tuple(dW0.shape) != tuple(W0.shape)
            or W0.shape[0] != (S + Dn) * D or Dn > D):
        raise RecError("dW0 must be [(S+Dn)*D, n_out] and dW0_folded [(S+1)*D, n_out] with Dn <= D")
    check(lib().rec_dense_fold_bwd_full(int(S), Dn, D, W0.shape[1], _p(dense_w), _p(W0), _p(dW0_folded), _p(dW0),
                                        _p(d_dense_w), int(accumulate), _stream()), "rec_dense_fold_bwd_full")


# ------------------------------------------------------------------ lookups
def emb_gather(ids, W, padding_idx=None, status=None, out=None, out_group=0, out_group_stride=0):
    """out[i,:] = W[ids[i],:] (zero row where ids[i]==padding_idx).  W [N,D] f32.
    out_group/out_group_stride: write lookup i at out + (i//group)*stride + (i%group)*D (floats)."""
    _chk(ids, torch.int64, "ids")
    _, w_stride = _chk_table(W, "W")
    N, D = W.shape
    if out is None:
        out = torch.empty(*ids.shape, D, dtype=torch.float32, device=ids.device)
    else:
        if out_group <= 0:
            _chk(out, torch.float32, "out")
            if out.numel() != ids.numel() * D:
                raise RecError("out has %d elements, expected %d" % (out.numel(), ids.numel() * D))
        elif not out.is_cuda or out.dtype != torch.float32:
            raise RecError("out must be a float32 device tensor")
    if status is None:
        status = new_status(ids.device)
    check(lib().rec_emb_gather(ids.numel(), D, w_stride, N,
                               -1 if padding_idx is None else padding_idx, _p(ids), _p(W), _p(out),
                               int(out_group), int(out_group_stride), _p(status), _stream()),
          "rec_emb_gather")
    return out, status


def emb_gather_sumpool(ids, lod, W, padding_idx=0, status=None):
    """ids [nnz] i64, lod [B+1] i64 -> (bow [B,D], counts [B] i32, status)"""
    _chk(ids, torch.int64, "ids")
    _chk(lod, torch.int64, "lod")
    _chk(W, torch.float32, "W")
    N, D = W.shape
    B = lod.numel() - 1
    out = torch.empty(B, D, dtype=torch.float32, device=W.device)
    counts = torch.empty(B, dtype=torch.int32, device=W.device)
    if status is None:
        status = new_status(W.device)
    check(lib().rec_emb_gather_sumpool(B, D, W.stride(0), N,
                                       -1 if padding_idx is None else padding_idx, _p(ids), _p(lod),
                                       _p(W), _p(out), _p(counts), _p(status), _stream()),
          "rec_emb_gather_sumpool")
    return out, counts, status


def emb_sumpool_bwd(lod, d_out, nnz):
    _chk(lod, torch.int64, "lod")
    _chk(d_out, torch.float32, "d_out")
    B, D = d_out.shape
    row_grad = torch.empty(nnz, D, dtype=torch.float32, device=d_out.device)
    check(lib().rec_emb_sumpool_bwd(B, D, _p(lod), _p(d_out), _p(row_grad), _stream()),
          "rec_emb_sumpool_bwd")
    return row_grad


class MultislotBatch:
    """Device-resident slot-major CSR of one batch (the layout rec_parse_feasign_slots writes):
    values [nnz] i64, lod [S, B+1] i64, slot_base [S+1] i64."""

    def __init__(self, values, lod, slot_base):
        _chk(values, torch.int64, "values")
        _chk(lod, torch.int64, "lod")
        _chk(slot_base, torch.int64, "slot_base")
        if lod.dim() != 2 or slot_base.numel() != lod.shape[0] + 1:
            raise RecError("lod must be [S, B+1] and slot_base [S+1]")
        self.values, self.lod, self.slot_base = values, lod, slot_base
        self.num_slots, self.batch = lod.shape[0], lod.shape[1] - 1
        self.nnz = values.numel()


def multislot_sumpool(mb, W, num_rows=None, padding_idx=0, key_mode=0, status=None, out=None, want_counts=True,
                      want_backward=True, lazy_init=None):
    """All slots of a batch in one launch (slot_dnn/net.py:63-77): -> (out [B, S*D], counts [B,S] i32 | None,
    seg_of_value [nnz] i32 | None, rows [nnz] i64 | None, status).  W [N,D] table view (row stride allowed);
    key_mode 1: values are uint64 feasigns hashed to rows on the device (feasign_rows).
    lazy_init = (state_offset, init_dims, init_range, seed): PS rows are born at their first pull (PsTable.lazy_init)."""
    D, stride = _chk_table(W, "W")
    N = int(num_rows if num_rows is not None else W.shape[0])
    B, S = mb.batch, mb.num_slots
    dev = W.device
    if B * S >= 2 ** 31:
        raise RecError("batch x slots must stay below 2^31")
    if out is None:
        out = torch.empty(B, S * D, dtype=torch.float32, device=dev)
    else:       # [B, ld] with ld >= S * D: the kernel writes the first S * D columns of a row (rec_multislot_desc.out_stride)
        _chk(out, torch.float32, "out")
        if out.dim() != 2 or out.shape[0] != B or out.shape[1] < S * D:
            raise RecError("out must be [batch, >= slots * emb_dim]")
    counts = torch.empty(B, S, dtype=torch.int32, device=dev) if want_counts else None
    seg = torch.empty(max(mb.nnz, 1), dtype=torch.int32, device=dev) if want_backward else None
    rows = torch.empty(max(mb.nnz, 1), dtype=torch.int64, device=dev) if want_backward else None
    if status is None:
        status = new_status(dev)
    d = MultislotDesc(B, S, D, stride, int(key_mode), N, -1 if padding_idx is None else int(padding_idx),
                      mb.lod.stride(0), out.shape[1], *(lazy_init if lazy_init is not None else (0, 0, 0.0, 0)))
    check(lib().rec_multislot_sumpool_fwd(C.byref(d), _p(mb.values), _p(mb.lod), _p(mb.slot_base), _p(W), _p(out),
                                          _p(counts), _p(seg), _p(rows), _p(status), _stream()),
          "rec_multislot_sumpool_fwd")
    return out, counts, seg, rows, status


def multislot_sumpool_bwd(seg_of_value, d_out, num_slots, emb_dim, nnz=None):
    """Rows form of the pool's gradient: row_grad [nnz, D], row k = d_out[b, s*D:(s+1)*D] of value k's segment b*S+s
    (what a binder that needs the SelectedRows value as a dense tensor hands to the optimizer; rows = the forward's)."""
    _chk(seg_of_value, torch.int32, "seg_of_value")
    _chk(d_out, torch.float32, "d_out")
    S, D = int(num_slots), int(emb_dim)
    if d_out.dim() != 2 or d_out.shape[1] < S * D or d_out.stride(1) != 1:
        raise RecError("d_out must be [batch, >= slots * emb_dim]")
    n = int(seg_of_value.numel() if nnz is None else nnz)
    row_grad = torch.empty(n, D, dtype=torch.float32, device=d_out.device)
    d = MultislotDesc(d_out.shape[0], S, D, D, 0, 1, -1, 0, d_out.stride(0), 0, 0, 0.0, 0)
    check(lib().rec_multislot_sumpool_bwd(C.byref(d), n, _p(seg_of_value), _p(d_out), _p(row_grad), _stream()),
          "rec_multislot_sumpool_bwd")
    return row_grad


def feasign_rows(keys, num_rows, out=None):
    """uint64 feasign bit patterns (int64 tensor) -> rows of a hashed table: 0 -> 0, f -> 1 + mix64(f) % (N-1)."""
    _chk(keys, torch.int64, "keys")
    if out is None:
        out = torch.empty_like(keys)
    check(lib().rec_feasign_rows(keys.numel(), int(num_rows), _p(keys), _p(out), _stream()), "rec_feasign_rows")
    return out


def feasign_rows_host(keys, num_rows):
    """Host variant over a numpy uint64 array (bit-identical to the device kernel)."""
    import numpy as np
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.empty(k.shape, np.int64)
    check(lib().rec_feasign_rows_host(k.size, int(num_rows), k.ctypes.data_as(C.c_void_p),
                                      out.ctypes.data_as(C.c_void_p)), "rec_feasign_rows_host")
    return out


# ------------------------------------------------------------------ SelectedRows merge + optimizers
class IdGroups:
    """Result buffers of rec_ids_group (device)."""

    def __init__(self, n, device):
        self.n = n
        self.sorted_pos = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self.uniq_rows = torch.empty(max(n, 1), dtype=torch.int64, device=device)
        self.seg_offset = torch.empty(n + 1, dtype=torch.int32, device=device)
        self.n_uniq = torch.zeros(4, dtype=torch.int32, device=device)
        self.rank = None            # [n] i32, filled by ids_group_slots / ids_rank when asked for

    def want_rank(self):
        if self.rank is None:
            self.rank = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.sorted_pos.device)
        return self.rank

    def host(self):
        """(sorted_pos[:n_valid], uniq_rows[:U], seg_offset[:U+1]) on the CPU — host sync."""
        U, nv = (int(x) for x in self.n_uniq.tolist()[:2])
        return (self.sorted_pos[:nv].cpu().numpy(), self.uniq_rows[:U].cpu().numpy(),
                self.seg_offset[:U + 1].cpu().numpy())


def ids_group(ids, num_rows, padding_idx, ws, slot_offset=None, status=None, groups=None, payload=None):
    """payload [n] int32 (or None): what groups.sorted_pos holds for every lookup instead of its position
    (rec_ids_group_payload) — the multi-slot path passes the (sample, slot) segment of every value."""
    _chk(ids, torch.int64, "ids")
    if payload is not None:
        _chk(payload, torch.int32, "payload")
        if payload.numel() < ids.numel():
            raise RecError("payload shorter than ids")
    n = ids.numel()
    S = ids.shape[-1] if ids.dim() > 1 else 1
    dev = ids.device
    if groups is None:
        groups = IdGroups(n, dev)
    if status is None:
        status = new_status(dev)
    nbytes = C.c_size_t(0)
    check(lib().rec_ids_group_workspace_bytes(n, num_rows, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_ids_group_payload(n, S, num_rows, -1 if padding_idx is None else padding_idx, _p(ids),
                                      _p(slot_offset), _p(payload), _p(groups.sorted_pos), _p(groups.uniq_rows),
                                      _p(groups.seg_offset), _p(groups.n_uniq), _p(status), _p(w),
                                      C.c_size_t(w.numel()), _stream()), "rec_ids_group_payload")
    return groups, status


def ids_group_slots(ids, slot_rows, padding_idx, ws, status=None, groups=None, want_rank=False):
    """ids [B,S] whose slot s owns rows [s*slot_rows, (s+1)*slot_rows) (rec_ids_group_slots): the grouping of
    ids_group(ids, S*slot_rows, ..., slot_offset = arange(S)*slot_rows), slot-local sort; want_rank: groups.rank[pos] =
    sorted index of lookup pos (-1 = dropped)."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2:
        raise RecError("ids must be [B, S]")
    B, S = ids.shape
    dev = ids.device
    if groups is None:
        groups = IdGroups(B * S, dev)
    if status is None:
        status = new_status(dev)
    rank = groups.want_rank() if want_rank else None
    nbytes = C.c_size_t(0)
    check(lib().rec_ids_group_slots_workspace_bytes(B, S, int(slot_rows), C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_ids_group_slots(B, S, int(slot_rows), -1 if padding_idx is None else padding_idx, _p(ids),
                                    _p(groups.sorted_pos), _p(groups.uniq_rows), _p(groups.seg_offset),
                                    _p(groups.n_uniq), _p(rank), _p(status), _p(w), C.c_size_t(w.numel()), _stream()),
          "rec_ids_group_slots")
    return groups, status


def group_slots_eligible(B, S, slot_rows):
    """True when rec_ids_group_slots sorts slot by slot for this shape (csrc/ids_group_slots.hip sg::eligible)."""
    return (B >= 8192 and 1 <= S <= 60 and 2 <= slot_rows <= (1 << 20) and B * S < 2 ** 31 - 1 and B <= 32 * 8192
            and S * slot_rows < 2 ** 32 - 1 and os.environ.get("REC_GROUP_SLOTS", "1") != "0")


def ids_rank(groups):
    """groups.rank[pos] = k with sorted_pos[k] = pos (-1 for dropped lookups) for a grouping made without payload."""
    rank = groups.want_rank()
    check(lib().rec_ids_rank(groups.n, _p(groups.n_uniq), _p(groups.sorted_pos), _p(rank), _stream()), "rec_ids_rank")
    return rank


def _gl(div, group, group_stride, partials=None, index=None, sorted_=False):
    if index is not None:
        _chk(index, torch.int32, "grad index")
    return GradLayout(int(div), int(group), int(group_stride), partials.data_ptr() if partials is not None else None,
                      index.data_ptr() if index is not None else None, int(bool(sorted_)))


def segment_partials(groups, grad, D, grad_div=1, grad_group=0, grad_group_stride=0, out=None, grad_index=None,
                     grad_sorted=False):
    """Tile partial sums of the long segments (hot rows) of `grad` under `groups` -> tensor to pass as
    `partials=` to the row-update ops together with the SAME grad and layout."""
    nbytes = C.c_size_t(0)
    check(lib().rec_segment_partials_bytes(groups.n, int(D), C.byref(nbytes)))
    need = max(nbytes.value // 4, 1)
    if out is None or out.numel() < need:
        out = torch.empty(need, dtype=torch.float32, device=grad.device)
    check(lib().rec_segment_partials(groups.n, int(D), _p(groups.n_uniq), _p(groups.seg_offset),
                                     _p(groups.sorted_pos), _p(grad),
                                     C.byref(_gl(grad_div, grad_group, grad_group_stride, None, grad_index, grad_sorted)),
                                     _p(out), _stream()),
          "rec_segment_partials")
    return out


def _hyper(lr, beta1, beta2, eps, step):
    return AdamHyper(float(lr), float(beta1), float(beta2), float(eps), int(step))


def sparse_adam_rows(groups, grad, grad_div, P, M, V, step, lr=1e-3, beta1=0.9, beta2=0.999,
                     eps=1e-8, grad_group=0, grad_group_stride=0, grad_scale=None, partials=None, grad_index=None,
                     l2=None):
    """grad_div / grad_group / grad_group_stride: rec_grad_layout (where position pos's row lives in
    grad); grad_scale: device float[1] clipping coefficient or None.  l2 given (a float, 0.0 included): L2Decay on the touched
    rows through rec_sparse_adam_rows_l2, whose zero coefficient runs the kernels of rec_sparse_adam_rows; None: the old
    entry point."""
    if grad_group <= 0:
        _chk(grad, torch.float32, "grad")
    elif not grad.is_cuda or grad.dtype != torch.float32:
        raise RecError("grad must be a float32 device tensor")
    D, stride = _chk_table(P, "P")
    sstride = _chk_table(M, "M")[1]
    for t, n in ((M, "M"), (V, "V")):
        if _chk_table(t, n) != (D, sstride) or t.shape[0] != P.shape[0]:
            raise RecError("%s must have the shape of P (M and V share one row stride)" % n)
    h = _hyper(lr, beta1, beta2, eps, step)
    if l2 is not None:
        check(lib().rec_sparse_adam_rows_l2(groups.n, D, stride, sstride, _p(groups.n_uniq), _p(groups.uniq_rows),
                                            _p(groups.seg_offset), _p(groups.sorted_pos), _p(grad),
                                            C.byref(_gl(grad_div, grad_group, grad_group_stride, partials, grad_index)),
                                            _p(grad_scale), _p(P), _p(M), _p(V), C.byref(h), float(l2), _stream()),
              "rec_sparse_adam_rows_l2")
        return
    check(lib().rec_sparse_adam_rows(groups.n, D, stride, sstride, _p(groups.n_uniq), _p(groups.uniq_rows),
                                     _p(groups.seg_offset), _p(groups.sorted_pos), _p(grad),
                                     C.byref(_gl(grad_div, grad_group, grad_group_stride, partials, grad_index)),
                                     _p(grad_scale), _p(P), _p(M), _p(V), C.byref(h), _stream()),
          "rec_sparse_adam_rows")


def sparse_adam_record(groups, grad, grad1, grad1_div, rec, mv, D, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                       v_offset=None, grad_scale=None, partials=None, partials1=None, grad_sorted=False):
    """Lazy Adam on BOTH embeddings of a DeepFM row in one pass: rec [N, stride] = W(D) | W1 | m1 | v1 | pad,
    mv [N, sstride] = m(D) | v(D) at v_offset.  grad [n,D] row gradients, grad1 = dz with layout {grad1_div,0,0}."""
    _chk(grad, torch.float32, "grad")
    _chk(grad1, torch.float32, "grad1")
    for t, n in ((rec, "rec"), (mv, "mv")):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
            raise RecError("%s must be a 2-D float32 device tensor with unit column stride" % n)
    if mv.shape[0] != rec.shape[0]:
        raise RecError("rec and mv must have the same number of rows")
    if v_offset is None:
        v_offset = (D + 3) // 4 * 4
    h = _hyper(lr, beta1, beta2, eps, step)
    check(lib().rec_sparse_adam_record(groups.n, int(D), rec.stride(0), mv.stride(0), int(v_offset),
                                       _p(groups.n_uniq), _p(groups.uniq_rows), _p(groups.seg_offset),
                                       _p(groups.sorted_pos), _p(grad),
                                       C.byref(_gl(1, 0, 0, partials, None, grad_sorted)), _p(grad1),
                                       C.byref(_gl(grad1_div, 0, 0, partials1)), _p(grad_scale), _p(rec), _p(mv),
                                       C.byref(h), _stream()), "rec_sparse_adam_record")


def adam_record_all(groups, grad, grad1, grad1_div, rec, mv, D, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                    v_offset=None, grad_scale=None, partials=None, partials1=None):
    """lazy_mode=False Adam (dygraph default) on BOTH embeddings of every row of the record layout of sparse_adam_record in
    one pass (rec_adam_record_all)."""
    _chk(grad, torch.float32, "grad")
    _chk(grad1, torch.float32, "grad1")
    for t, n in ((rec, "rec"), (mv, "mv")):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
            raise RecError("%s must be a 2-D float32 device tensor with unit column stride" % n)
    if mv.shape[0] != rec.shape[0]:
        raise RecError("rec and mv must have the same number of rows")
    if v_offset is None:
        v_offset = (D + 3) // 4 * 4
    h = _hyper(lr, beta1, beta2, eps, step)
    check(lib().rec_adam_record_all(rec.shape[0], int(D), rec.stride(0), mv.stride(0), int(v_offset),
                                    _p(groups.n_uniq), _p(groups.uniq_rows), _p(groups.seg_offset),
                                    _p(groups.sorted_pos), _p(grad), C.byref(_gl(1, 0, 0, partials)), _p(grad1),
                                    C.byref(_gl(grad1_div, 0, 0, partials1)), _p(grad_scale), _p(rec), _p(mv),
                                    C.byref(h), _stream()), "rec_adam_record_all")


def adam_rows_all(groups, grad, grad_div, P, M, V, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                  grad_group=0, grad_group_stride=0, grad_scale=None, partials=None, l2=None):
    """lazy_mode=False Adam (dygraph default): every row of P/M/V moves, absent rows with g = 0.  l2 given (a float, 0.0
    included): L2Decay, every row moves with g + l2 * w, through rec_adam_rows_all_l2 (a zero coefficient runs the
    kernels of rec_adam_rows_all); None: the old entry point."""
    D, stride = _chk_table(P, "P")
    sstride = _chk_table(M, "M")[1]
    for t, n in ((M, "M"), (V, "V")):
        if _chk_table(t, n) != (D, sstride) or t.shape[0] != P.shape[0]:
            raise RecError("%s must have the shape of P (M and V share one row stride)" % n)
    h = _hyper(lr, beta1, beta2, eps, step)
    if l2 is not None:
        check(lib().rec_adam_rows_all_l2(P.shape[0], D, stride, sstride, _p(groups.n_uniq), _p(groups.uniq_rows),
                                         _p(groups.seg_offset), _p(groups.sorted_pos), _p(grad),
                                         C.byref(_gl(grad_div, grad_group, grad_group_stride, partials)),
                                         _p(grad_scale), _p(P), _p(M), _p(V), C.byref(h), float(l2), _stream()),
              "rec_adam_rows_all_l2")
        return
    check(lib().rec_adam_rows_all(P.shape[0], D, stride, sstride, _p(groups.n_uniq), _p(groups.uniq_rows),
                                  _p(groups.seg_offset), _p(groups.sorted_pos), _p(grad),
                                  C.byref(_gl(grad_div, grad_group, grad_group_stride, partials)),
                                  _p(grad_scale), _p(P), _p(M), _p(V), C.byref(h), _stream()),
          "rec_adam_rows_all")


def sparse_adagrad_rows(groups, grad, rec, emb_dim, num_slots, label=None, lr=0.05, initial_g2sum=3.0,
                        bounds=(-10.0, 10.0), grad_div=1, grad_group=0, grad_group_stride=0, partials=None,
                        grad_index=None):
    """PS accessor rule (SparseAdaGradSGDRule + show/click) on the touched rows of a record table
    rec [N, stride] = [show | click | g2sum_w | g2sum_x | W(D) | pad]."""
    if rec.dim() != 2 or rec.dtype != torch.float32 or not rec.is_cuda or rec.stride(1) != 1:
        raise RecError("rec must be a 2-D float32 device tensor with unit column stride")
    if label is not None:
        _chk(label, torch.int64, "label")
    h = AdagradHyper(float(lr), float(initial_g2sum), float(bounds[0]), float(bounds[1]))
    check(lib().rec_sparse_adagrad_rows(groups.n, int(emb_dim), rec.stride(0), int(num_slots), _p(groups.n_uniq),
                                        _p(groups.uniq_rows), _p(groups.seg_offset), _p(groups.sorted_pos),
                                        _p(grad),
                                        C.byref(_gl(grad_div, grad_group, grad_group_stride, partials, grad_index)),
                                        _p(label), _p(rec), C.byref(h), _stream()), "rec_sparse_adagrad_rows")


class PsTable:
    """A PS / gpubox sparse table on the device: record rows + the accessor parameters
    (slot_dnn/config_online.yaml:57-89; arithmetic = Paddle's published CtrCommonAccessor / SparseAdaGradSGDRule,
    see include/recengine.h and oracle/ps_ref.py).  kind "slot": W = [embed_w, embedx(D-1)] (slot_dnn / dnn: the
    looked-up vector is the whole W); kind "deepfm": embedx = the D-dim embedding at 0, embed_w = the first-order
    weight behind it.  Rows are zero memory until their first push (state float); a key that does not exist reads as
    zeros, as PullSparse returns it."""

    NUM_STATS = 7   # show, click, g2sum_w, g2sum_x, state, delta_score, unseen_days

    def __init__(self, num_rows, emb_dim, device, kind="slot", lr=0.05, initial_g2sum=3.0, bounds=(-10.0, 10.0),
                 initial_range=1e-4, embedx_threshold=10.0, nonclk_coeff=0.1, click_coeff=1.0, seed=2025,
                 row_stride=None, row_mul=1, row_add=0, embedx_lr=None, embedx_initial_g2sum=None,
                 embedx_bounds=None, embedx_initial_range=None, grad_scale=1.0, show_scale=True,
                 embed_zero_init=True):
        D = int(emb_dim)
        if kind == "slot":      # [W(D) | 7 statistics]: D = 9 -> 16 floats = one 64-B half line
            need = D + self.NUM_STATS
            stride = int(row_stride or (16 if need <= 16 else (need + 31) // 32 * 32))
            self.layout = PsLayout(stride, 0, 1, D - 1, D)
            self.w_cols = slice(0, D)
            stat0 = D
        elif kind == "deepfm":  # [W(D) | W1 | 7 statistics | pad]
            need = D + 1 + self.NUM_STATS
            stride = int(row_stride or (need + 31) // 32 * 32)
            self.layout = PsLayout(stride, D, 0, D, D + 1)
            self.w_cols = slice(0, D)
            stat0 = D + 1
        else:
            raise RecError("kind must be 'slot' or 'deepfm'")
        if stride < need:
            raise RecError("row_stride %d < %d" % (stride, need))
        self.stat = slice(stat0, stat0 + 4)                  # show, click, g2sum_w, g2sum_x
        self.stat_all = slice(stat0, stat0 + self.NUM_STATS)
        self.state_col = stat0 + 4
        self.delta_col, self.unseen_col = stat0 + 5, stat0 + 6
        self.kind, self.emb_dim, self.num_rows = kind, D, int(num_rows)
        self.rec = torch.zeros(int(num_rows), stride, dtype=torch.float32, device=device)
        self.W = self.rec[:, self.w_cols]
        xb = embedx_bounds if embedx_bounds is not None else bounds
        self.accessor = PsAccessor(
            float(lr), float(initial_g2sum), float(bounds[0]), float(bounds[1]), float(initial_range),
            float(lr if embedx_lr is None else embedx_lr),
            float(initial_g2sum if embedx_initial_g2sum is None else embedx_initial_g2sum), float(xb[0]), float(xb[1]),
            float(initial_range if embedx_initial_range is None else embedx_initial_range),
            float(embedx_threshold), float(nonclk_coeff), float(click_coeff), float(grad_scale),
            1 if show_scale else 0, 1 if embed_zero_init else 0, int(seed), int(row_mul), int(row_add))

    @property
    def lazy_init(self):
        """(state_offset, init_dims, init_range, seed) for the lookups: what a key that does not exist reads as.
        Paddle's default (embed_zero_init): zeros = the memory itself, lazy init off (range 0).  Otherwise embed_w
        (element 0 of a 'slot' vector) reads as its creation value, which the first push stores."""
        a = self.accessor
        rng = 0.0 if a.embed_zero_init else a.initial_range
        return (self.state_col - self.w_cols.start, 1, rng, a.seed)


def record_gather(rows, rec, D, out_w, out_w1, status, table=None):
    """Owner-side lookup: both embeddings of every row from its one record line (rec [N, stride] = W(D) | W1 | ...).
    table (PsTable, kind 'deepfm'): unborn rows read as their creation values."""
    _chk(rows, torch.int64, "rows")
    if rec.dim() != 2 or rec.dtype != torch.float32 or not rec.is_cuda or rec.stride(1) != 1:
        raise RecError("rec must be a 2-D float32 device tensor with unit column stride")
    n = rows.numel()
    _chk(out_w, torch.float32, "out_w")               # the kernel writes row i at out_w + i * D and out_w1[i]: no strides
    _chk(out_w1, torch.float32, "out_w1")
    if out_w.numel() != n * int(D) or out_w1.numel() != n:
        raise RecError("record_gather: out_w must hold [n, D] and out_w1 [n] floats (n %d, D %d)" % (n, int(D)))
    lz = None
    if table is not None and not table.accessor.embed_zero_init and table.accessor.initial_range > 0:
        a = table.accessor      # embed_w (W1) of a key that does not exist yet reads as its creation value
        lz = LazyInit(table.state_col, 1, a.initial_range, a.seed, a.row_mul, a.row_add)
    check(lib().rec_record_gather(n, int(D), rec.stride(0), rec.shape[0], _p(rows), _p(rec), _p(out_w), _p(out_w1),
                                  C.byref(lz) if lz is not None else None, _p(status), _stream()),
          "rec_record_gather")
    return out_w, out_w1


def ps_push_rows(table, groups, grad, num_slots, grad_pitch=None, grad_index=None, grad1=None, grad1_div=1,
                 show=None, click=None, grad1_pitch=1, grad_group=0, grad_group_stride=0):
    """CtrCommonAccessor::Update on the touched rows of `table` (PsTable).  kind 'slot': grad rows [*, D] hold
    [g_embed_w, g_embedx...]; kind 'deepfm': grad = the D-dim row gradients, grad1 = dz [B] (layout {grad1_div}).
    grad_group / grad_group_stride: rec_grad_layout (rows of `grad_group` segments at a padded stride)."""
    D = table.emb_dim
    pitch = int(grad_pitch or D)
    if table.kind == "slot":
        gx = GradSrc(grad.data_ptr(), _gl(1, grad_group, grad_group_stride, None, grad_index), pitch, 1)
        gw = GradSrc(grad.data_ptr(), _gl(1, grad_group, grad_group_stride, None, grad_index), pitch, 0)
    else:
        if grad1 is None:
            raise RecError("kind 'deepfm' needs grad1 (the first-order gradient)")
        gx = GradSrc(grad.data_ptr(), _gl(1, 0, 0, None, grad_index), pitch, 0)
        gw = GradSrc(grad1.data_ptr(), _gl(grad1_div, 0, 0, None, None), int(grad1_pitch), 0)
    for t, n in ((show, "show"), (click, "click")):
        if t is not None:
            _chk(t, torch.int64, n)
    check(lib().rec_ps_push_rows(groups.n, int(num_slots), C.byref(table.layout), _p(groups.n_uniq),
                                 _p(groups.uniq_rows), _p(groups.seg_offset), _p(groups.sorted_pos), C.byref(gx),
                                 C.byref(gw), _p(show), _p(click), _p(table.rec), C.byref(table.accessor), _stream()),
          "rec_ps_push_rows")


def ps_shrink_rows(table, decay=0.98, delete_threshold=0.8, delete_after_unseen_days=float("inf")):
    """CtrCommonAccessor::Shrink: counters decay; values below delete_threshold or unseen for more than
    delete_after_unseen_days are deleted.  -> number deleted (host sync)."""
    n = torch.zeros(1, dtype=torch.int64, device=table.rec.device)
    check(lib().rec_ps_shrink_rows(table.num_rows, C.byref(table.layout), _p(table.rec), float(decay),
                                   float(delete_threshold), float(min(delete_after_unseen_days, 3.0e38)),
                                   C.byref(table.accessor), _p(n), _stream()),
          "rec_ps_shrink_rows")
    return int(n.item())


def ps_save_select(table, param, base_threshold=1.5, delta_threshold=0.25, delta_keep_days=16.0):
    """CtrCommonAccessor::Save(param) + UpdateStatAfterSave(param) over the table -> bool [N] device mask of the rows a
    save of this kind writes (0 all, 1 delta, 2 base, 3 all + unseen_days += 1)."""
    sel = torch.zeros(table.num_rows, dtype=torch.uint8, device=table.rec.device)
    check(lib().rec_ps_save_select(table.num_rows, C.byref(table.layout), _p(table.rec), int(param),
                                   float(base_threshold), float(delta_threshold), float(delta_keep_days),
                                   C.byref(table.accessor), _p(sel), None, _stream()), "rec_ps_save_select")
    return sel.bool()


def adam_dense(p, m, v, g, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=None):
    for t, n in ((p, "p"), (m, "m"), (v, "v"), (g, "g")):
        _chk(t, torch.float32, n)
    h = _hyper(lr, beta1, beta2, eps, step)
    check(lib().rec_adam_dense(p.numel(), _p(p), _p(m), _p(v), _p(g), _p(grad_scale), C.byref(h),
                               _stream()), "rec_adam_dense")


def adagrad_rows(groups, grad, grad_div, P, A, lr, epsilon=1e-6, grad_group=0, grad_group_stride=0, partials=None,
                 grad_index=None):
    """paddle.optimizer.Adagrad on the touched rows (rec_adagrad_rows): acc += g*g; p -= lr * g / (sqrt(acc) + epsilon) with
    g the MERGED gradient of each unique row of `groups`.  A: the accumulator table, the shape of P (created by the caller
    at initial_accumulator_value).  grad_div / grad_group / grad_group_stride / partials as sparse_adam_rows."""
    if grad_group <= 0:
        _chk(grad, torch.float32, "grad")
    elif not torch.is_tensor(grad) or not grad.is_cuda or grad.dtype != torch.float32:
        raise RecError("grad must be a float32 device tensor")
    D, stride = _chk_table(P, "P")
    if _chk_table(A, "A")[0] != D or A.shape[0] != P.shape[0]:
        raise RecError("A must have the shape of P")
    sstride = _chk_table(A, "A")[1]
    if A.data_ptr() == P.data_ptr():
        raise RecError("A must not be P")
    check(lib().rec_adagrad_rows(groups.n, D, stride, sstride, _p(groups.n_uniq), _p(groups.uniq_rows),
                                 _p(groups.seg_offset), _p(groups.sorted_pos), _p(grad),
                                 C.byref(_gl(grad_div, grad_group, grad_group_stride, partials, grad_index)),
                                 _p(P), _p(A), float(lr), float(epsilon), _stream()), "rec_adagrad_rows")


def adagrad_dense(p, acc, g, lr, epsilon=1e-6):
    """paddle.optimizer.Adagrad over a flat buffer (rec_adagrad_dense): p, acc, g contiguous float32 of one length."""
    for t, n in ((p, "p"), (acc, "acc"), (g, "g")):
        if not torch.is_tensor(t):
            raise RecError("%s must be a float32 device tensor" % n)
        _chk(t, torch.float32, n)
    if not (p.numel() == acc.numel() == g.numel()):
        raise RecError("p, acc and g must have one length (%d, %d, %d)" % (p.numel(), acc.numel(), g.numel()))
    check(lib().rec_adagrad_dense(p.numel(), _p(p), _p(acc), _p(g), float(lr), float(epsilon), _stream()),
          "rec_adagrad_dense")


def _sumsq_ws(ws):
    nbytes = C.c_size_t(0)
    check(lib().rec_sumsq_workspace_bytes(C.byref(nbytes)))
    return ws.get(nbytes.value)


def sumsq(x, out, ws, accumulate=False):
    """out[0] (+)= sum(x^2), fixed reduction order."""
    _chk(x, torch.float32, "x")
    _chk(out, torch.float32, "out")
    w = _sumsq_ws(ws)
    check(lib().rec_sumsq(x.numel(), _p(x), _p(out), int(accumulate), _p(w), C.c_size_t(w.numel()),
                          _stream()), "rec_sumsq")
    return out


def sparse_rows_sumsq(groups, grad, D, out, ws, accumulate=False, grad_div=1, grad_group=0,
                      grad_group_stride=0, partials=None):
    """out[0] (+)= sum over merged rows of |sum of the row's duplicate gradients|^2."""
    _chk(out, torch.float32, "out")
    w = _sumsq_ws(ws)
    check(lib().rec_sparse_rows_sumsq(groups.n, int(D), _p(groups.n_uniq), _p(groups.seg_offset),
                                      _p(groups.sorted_pos), _p(grad),
                                      C.byref(_gl(grad_div, grad_group, grad_group_stride, partials)),
                                      _p(out), int(accumulate), _p(w), C.c_size_t(w.numel()), _stream()),
          "rec_sparse_rows_sumsq")
    return out


def dropout(x, p, seed, stream_a, stream_b=None, out=None, step_stride=0):
    """Train-mode Dropout (upscale_in_train) on a 2-D float32 matrix (row stride allowed), in place by default.
    stream_b: a second mask stream applied in the same pass (keep = keepA & keepB, scale 1/(1-p)^2).
    step_stride: by how much the caller's mask streams advance per training step (a recorded step re-derives them)."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise RecError("x must be a 2-D float32 device tensor with unit column stride")
    if out is None:
        out = x
    sa, sb = C.c_uint64(int(stream_a)), C.c_uint64(int(stream_b or 0))
    if _recorder is not None:
        if not step_stride:
            raise RecError("dropout inside a recorded step needs step_stride")
        _recorder.note_step_arg(sa, step_stride)
        if stream_b is not None:
            _recorder.note_step_arg(sb, step_stride)
    check(lib().rec_dropout(x.shape[0], x.shape[1], x.stride(0), out.stride(0), _p(x), _p(out), float(p), int(seed),
                            sa, sb, 2 if stream_b is not None else 1, _stream()),
          "rec_dropout")
    return out


def l2_decay_grad(grad, w, coeff, grad_scale=None):
    """grad += (coeff / grad_scale) * w  (L2Decay appended after clipping; grad / w contiguous float32 views)."""
    _chk(grad, torch.float32, "grad")
    _chk(w, torch.float32, "w")
    check(lib().rec_l2_decay_grad(grad.numel(), _p(grad), _p(w), float(coeff), _p(grad_scale), _stream()),
          "rec_l2_decay_grad")
    return grad


def clip_scale(sumsq_t, clip_norm, out):
    """out[0] = clip_norm / max(sqrt(sumsq), clip_norm)  (ClipGradByGlobalNorm coefficient)."""
    check(lib().rec_clip_scale(_p(sumsq_t), float(clip_norm), _p(out), _stream()), "rec_clip_scale")
    return out


def din_attention_pool(hist_item, hist_cat, tgt_item_seq, tgt_cat_seq, mask, w_hist_item, w_hist_cat,
                       w_tgt_item_seq, w_tgt_cat_seq, att_w, att_b, status=None, want_weights=True, saved=None, ws=None):
    """Fused DIN attention-pool forward (din/net.py:141-173).  ids/mask [B,T] i64; att_w/att_b: the three
    attention Linear layers ([4E,H1],[H1,H2],[H2,1] / biases).  -> (out [B,E], att_weight [B,T] | None, status)
    saved: a dict the training caller hands in; it receives what the backward can reuse ("out", and "act1"
    [B,T,H1] when the engine saves layer-1 activations for this shape) — pass it on to din_attention_pool_bwd.
    ws (ops.Workspace, optional): lets a batch of few samples run one block per history tile
    (rec_din_attention_pool_fwd_ws)."""
    B, T = hist_item.shape
    for t, n in ((hist_item, "hist_item"), (hist_cat, "hist_cat"), (tgt_item_seq, "tgt_item_seq"),
                 (tgt_cat_seq, "tgt_cat_seq"), (mask, "mask")):
        _chk(t, torch.int64, n, (B, T))
    Ei, ldi = _chk_table(w_hist_item, "w_hist_item")
    Ec, ldc = _chk_table(w_hist_cat, "w_hist_cat")
    if _chk_table(w_tgt_item_seq, "w_tgt_item_seq") != (Ei, ldi) or _chk_table(w_tgt_cat_seq, "w_tgt_cat_seq") != (Ec, ldc):
        raise RecError("target tables must have the shape/stride of the history tables")
    E, H1, H2 = Ei + Ec, att_w[0].shape[1], att_w[1].shape[1]
    _chk(att_w[0], torch.float32, "att_w1", (4 * E, H1))
    _chk(att_w[1], torch.float32, "att_w2", (H1, H2))
    for t, n in ((att_w[2], "att_w3"), (att_b[0], "att_b1"), (att_b[1], "att_b2"), (att_b[2], "att_b3")):
        _chk(t, torch.float32, n)
    dev = hist_item.device
    out = torch.empty(B, E, dtype=torch.float32, device=dev)
    attw = torch.empty(B, T, dtype=torch.float32, device=dev) if want_weights else None
    if status is None:
        status = new_status(dev)
    d = DinDesc(B, T, Ei, Ec, H1, H2, w_hist_item.shape[0], w_hist_cat.shape[0], ldi, ldc)
    act1 = None
    if saved is not None and lib().rec_din_saves_act1(C.byref(d)):
        act1 = saved.get("act1")
        if act1 is None or act1.shape != (B, T, H1) or act1.device != dev:
            act1 = torch.empty(B, T, H1, dtype=torch.float32, device=dev)
    wk, nb = None, 0
    if ws is not None:
        nbytes = C.c_size_t(0)
        check(lib().rec_din_attention_pool_fwd_workspace_bytes(C.byref(d), C.byref(nbytes)))
        if nbytes.value:
            wk = ws.get(nbytes.value)
            nb = wk.numel()
    args = (C.byref(d), _p(hist_item), _p(hist_cat), _p(tgt_item_seq), _p(tgt_cat_seq), _p(mask),
            _p(w_hist_item), _p(w_hist_cat), _p(w_tgt_item_seq), _p(w_tgt_cat_seq), _p(att_w[0]), _p(att_b[0]),
            _p(att_w[1]), _p(att_b[1]), _p(att_w[2]), _p(att_b[2]), _p(out), _p(attw), _p(act1), _p(status))
    if ws is None:           # no workspace at all: the entry point without one (the _ws form owes what its query names)
        check(lib().rec_din_attention_pool_fwd(*args, _stream()), "rec_din_attention_pool_fwd")
    else:
        check(lib().rec_din_attention_pool_fwd_ws(*args, _p(wk), C.c_size_t(nb), _stream()), "rec_din_attention_pool_fwd_ws")
    if saved is not None:
        saved["out"], saved["act1"] = out, act1
    return out, attw, status


def din_attention_pool_bwd(hist_item, hist_cat, tgt_item_seq, tgt_cat_seq, w_hist_item, w_hist_cat,
                           w_tgt_item_seq, w_tgt_cat_seq, att_w, att_b, att_weight, d_out, saved=None, ws=None):
    """-> (d_hist [B,T,E], d_tgt_seq [B,T,E]): per-position gradients of the gathered rows.
    saved: the dict the forward filled (optional; without it the hidden activations are recomputed).
    ws (ops.Workspace, optional): large batches draw their samples from a ticket counter in it
    (rec_din_attention_pool_bwd_ws)."""
    B, T = hist_item.shape
    Ei, ldi = _chk_table(w_hist_item, "w_hist_item")
    Ec, ldc = _chk_table(w_hist_cat, "w_hist_cat")
    E, H1, H2 = Ei + Ec, att_w[0].shape[1], att_w[1].shape[1]
    _chk(att_weight, torch.float32, "att_weight", (B, T))
    _chk(d_out, torch.float32, "d_out", (B, E))
    w1t = _transposed(att_w[0])
    dev = hist_item.device
    dh = torch.empty(B, T, E, dtype=torch.float32, device=dev)
    dq = torch.empty(B, T, E, dtype=torch.float32, device=dev)
    d = DinDesc(B, T, Ei, Ec, H1, H2, w_hist_item.shape[0], w_hist_cat.shape[0], ldi, ldc)
    out_s = act1_s = None
    if saved is not None and saved.get("act1") is not None and saved.get("out") is not None:
        out_s, act1_s = saved["out"], saved["act1"]
        _chk(out_s, torch.float32, "saved out", (B, E))
        _chk(act1_s, torch.float32, "saved act1", (B, T, H1))
    wk, nb = None, 0
    if ws is not None:
        nbytes = C.c_size_t(0)
        check(lib().rec_din_attention_pool_bwd_workspace_bytes(C.byref(d), C.byref(nbytes)))
        if nbytes.value:
            wk = ws.get(nbytes.value)
            nb = wk.numel()
    args = (C.byref(d), _p(hist_item), _p(hist_cat), _p(tgt_item_seq), _p(tgt_cat_seq), _p(w_hist_item),
            _p(w_hist_cat), _p(w_tgt_item_seq), _p(w_tgt_cat_seq), _p(att_w[0]), _p(w1t), _p(att_b[0]),
            _p(att_w[1]), _p(att_b[1]), _p(att_w[2]), _p(att_weight), _p(out_s), _p(act1_s), _p(d_out), _p(dh), _p(dq))
    if ws is None:
        check(lib().rec_din_attention_pool_bwd(*args, _stream()), "rec_din_attention_pool_bwd")
    else:
        check(lib().rec_din_attention_pool_bwd_ws(*args, _p(wk), C.c_size_t(nb), _stream()), "rec_din_attention_pool_bwd_ws")
    return dh, dq


# ------------------------------------------------------------------ DIEN (rank/dien): GRU recurrence, aux loss, attention
GRU_MAX_HIDDEN = 256


def _gru_dims(t, cols, name):
    """t [B, T, cols * H] contiguous f32 -> (B, T, H)."""
    _chk(t, torch.float32, name)
    if t.dim() != 3 or t.shape[2] % cols or t.shape[1] < 1:
        raise RecError("%s must be [B, T, %d * H] with T >= 1" % (name, cols))
    B, T, H = t.shape[0], t.shape[1], t.shape[2] // cols
    if H % 4 or not 0 < H <= GRU_MAX_HIDDEN:
        raise RecError("%s: hidden size %d unsupported (a multiple of 4, at most %d)" % (name, H, GRU_MAX_HIDDEN))
    return B, T, H


def gru_seq_fwd(Gi, W_hh, b_hh, want_saved=True):
    """The whole time loop of one GRU layer in one launch (rec_gru_seq_fwd).  Gi [B,T,3H] = X W_ih^T + b_ih (gate order
    r, z, c), W_hh [3H,H], b_hh [3H]; h_0 = 0.  -> (H_out [B,T,H], saved [B,T,5H] = r | z | c | hc | h_prev, or None)."""
    B, T, H = _gru_dims(Gi, 3, "Gi")
    _chk(W_hh, torch.float32, "W_hh", (3 * H, H))
    _chk(b_hh, torch.float32, "b_hh", (3 * H,))
    H_out = torch.empty(B, T, H, dtype=torch.float32, device=Gi.device)
    saved = torch.empty(B, T, 5 * H, dtype=torch.float32, device=Gi.device) if want_saved else None
    check(lib().rec_gru_seq_fwd(B, T, H, _p(Gi), _p(W_hh), _p(b_hh), _p(H_out), _p(saved), _stream()), "rec_gru_seq_fwd")
    return H_out, saved


def gru_seq_bwd(saved, W_hh, dH_out=None, dh_T=None):
    """Backward through time in one launch (rec_gru_seq_bwd) from a per-step gradient dH_out [B,T,H] and / or a gradient
    of the last state dh_T [B,H].  -> (dGi, dGh) [B,T,3H]."""
    B, T, H = _gru_dims(saved, 5, "saved")
    _chk(W_hh, torch.float32, "W_hh", (3 * H, H))
    _chk(dH_out, torch.float32, "dH_out", (B, T, H))
    _chk(dh_T, torch.float32, "dh_T", (B, H))
    dGi = torch.empty(B, T, 3 * H, dtype=torch.float32, device=saved.device)
    dGh = torch.empty(B, T, 3 * H, dtype=torch.float32, device=saved.device)
    check(lib().rec_gru_seq_bwd(B, T, H, _p(saved), _p(W_hh), _p(dH_out), _p(dh_T), _p(dGi), _p(dGh), _stream()),
          "rec_gru_seq_bwd")
    return dGi, dGh


def gru_layer_fwd(X, W_ih, W_hh, b_ih, b_hh, ws, want_saved=True):
    """One GRU layer over X [B,T,E]: the input projection on rec_gemm_f32 (all B*T rows at once), the recurrence in
    gru_seq_fwd.  W_ih [3H,E].  -> (H_out, saved)."""
    _chk(X, torch.float32, "X")
    if X.dim() != 3:
        raise RecError("gru_layer_fwd: X must be [B, T, E]")
    B, T, E = X.shape
    H = W_hh.shape[1]
    _chk(W_ih, torch.float32, "W_ih", (3 * H, E))
    Gi = gemm(X.view(B * T, E), W_ih, ws, trans_b=True, epilogue="bias", bias=b_ih)
    return gru_seq_fwd(Gi.view(B, T, 3 * H), W_hh, b_hh, want_saved=want_saved)


def gru_layer_bwd(X, saved, W_ih, W_hh, ws, dW_ih, dW_hh, db_ih, db_hh, dH_out=None, dh_T=None, want_dX=True, dX_add=None):
    """Backward of gru_layer_fwd: the time loop in gru_seq_bwd, then one GEMM each over the B*T rows — dW_ih = dGi^T X,
    dW_hh = dGh^T H_prev, the bias gradients as column sums and dX = dGi W_ih (+ dX_add [B,T,E]).  -> dX | None."""
    B, T, E = X.shape
    dGi, dGh = gru_seq_bwd(saved, W_hh, dH_out=dH_out, dh_T=dh_T)
    H = W_hh.shape[1]
    gi, gh = dGi.view(B * T, 3 * H), dGh.view(B * T, 3 * H)
    gemm(gi, X.view(B * T, E), ws, trans_a=True, out=dW_ih)
    gemm(gh, saved.view(B * T, 5 * H)[:, 4 * H:], ws, trans_a=True, out=dW_hh)
    colsum(gi, ws, out=db_ih)
    colsum(gh, ws, out=db_hh)
    if not want_dX:
        return None
    if dX_add is None:
        return gemm(gi, W_ih, ws).view(B, T, E)
    return gemm(gi, W_ih, ws, epilogue="add", aux1=dX_add.view(B * T, E)).view(B, T, E)


def _dien_aux_args(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat):
    _chk(gru_out, torch.float32, "gru_out")
    if gru_out.dim() != 3:
        raise RecError("dien aux: gru_out must be [B, T, H]")
    B, T, H = gru_out.shape
    _chk(hist, torch.float32, "hist", (B, T, H))
    _chk(neg_item, torch.int64, "neg_item", (B, T))
    _chk(neg_cat, torch.int64, "neg_cat", (B, T))
    Ei, si = _chk_table(W_neg_item, "W_neg_item")
    Ec, sc = _chk_table(W_neg_cat, "W_neg_cat")
    if Ei + Ec != H:
        raise RecError("dien aux: item_dim %d + cat_dim %d != H %d" % (Ei, Ec, H))
    return B, T, Ei, Ec, si, sc


def dien_aux_fwd(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat, ws, padding_idx=0, status=None, out=None):
    """DIEN's auxiliary loss (rec_dien_aux_fwd; dien/net.py:219-254).  -> (aux [1], status)."""
    B, T, Ei, Ec, si, sc = _dien_aux_args(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=gru_out.device)
    if status is None:
        status = new_status(gru_out.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_dien_aux_workspace_bytes(B, T, C.byref(nbytes)), "rec_dien_aux_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_dien_aux_fwd(B, T, Ei, Ec, _p(gru_out), _p(hist), _p(neg_item), _p(neg_cat), _p(W_neg_item), si,
                                 W_neg_item.shape[0], _p(W_neg_cat), sc, W_neg_cat.shape[0],
                                 -1 if padding_idx is None else padding_idx, _p(out), _p(status), _p(wk),
                                 C.c_size_t(wk.numel()), _stream()), "rec_dien_aux_fwd")
    return out, status


def dien_aux_bwd(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat, d_hist, accumulate=True, d_aux=1.0,
                 padding_idx=0, status=None):
    """Backward of dien_aux_fwd (rec_dien_aux_bwd): d_hist [B,T,H] receives (accumulate: is added) the t+1-shifted
    contribution.  -> (d_gru_out [B,T,H], d_neg [B,T,H])."""
    B, T, Ei, Ec, si, sc = _dien_aux_args(gru_out, hist, neg_item, neg_cat, W_neg_item, W_neg_cat)
    _chk(d_hist, torch.float32, "d_hist", (B, T, Ei + Ec))
    d_go, d_neg = torch.empty_like(gru_out), torch.empty_like(gru_out)
    if status is None:
        status = new_status(gru_out.device)
    check(lib().rec_dien_aux_bwd(B, T, Ei, Ec, _p(gru_out), _p(hist), _p(neg_item), _p(neg_cat), _p(W_neg_item), si,
                                 W_neg_item.shape[0], _p(W_neg_cat), sc, W_neg_cat.shape[0],
                                 -1 if padding_idx is None else padding_idx, float(d_aux), _p(d_go), _p(d_hist),
                                 int(bool(accumulate)), _p(d_neg), _p(status), _stream()), "rec_dien_aux_bwd")
    return d_go, d_neg


def dien_att_feat_fwd(hist, q):
    """feat [n, 4E] = [h, q, h - q, h * q] (rec_dien_att_feat_fwd); hist, q [.., E]."""
    _chk(hist, torch.float32, "hist")
    _chk(q, torch.float32, "q", tuple(hist.shape))
    E = hist.shape[-1]
    n = hist.numel() // E
    feat = torch.empty(n, 4 * E, dtype=torch.float32, device=hist.device)
    check(lib().rec_dien_att_feat_fwd(n, E, _p(hist), _p(q), _p(feat), _stream()), "rec_dien_att_feat_fwd")
    return feat


def dien_att_feat_bwd(hist, q, dfeat, d_hist, accumulate=True):
    """d_hist (+)= d0 + d2 + d3 * q; -> d_q = d1 - d2 + d3 * h (rec_dien_att_feat_bwd)."""
    E = hist.shape[-1]
    n = hist.numel() // E
    _chk(hist, torch.float32, "hist")
    _chk(q, torch.float32, "q", tuple(hist.shape))
    _chk(dfeat, torch.float32, "dfeat", (n, 4 * E))
    _chk(d_hist, torch.float32, "d_hist", tuple(hist.shape))
    d_q = torch.empty_like(hist)
    check(lib().rec_dien_att_feat_bwd(n, E, _p(hist), _p(q), _p(dfeat), _p(d_hist), int(bool(accumulate)), _p(d_q),
                                      _stream()), "rec_dien_att_feat_bwd")
    return d_q


def dien_softmax_weight_fwd(score, mask, hist, scale):
    """w [B,T] = softmax_t((score + mask) * scale), x_att = w * hist (rec_dien_attention_seq_fwd)."""
    _chk(hist, torch.float32, "hist")
    if hist.dim() != 3:
        raise RecError("dien attention seq: hist must be [B, T, E]")
    B, T, E = hist.shape
    _chk(score, torch.float32, "score")
    _chk(mask, torch.float32, "mask")
    if score.numel() != B * T or mask.numel() != B * T:
        raise RecError("dien attention seq: score and mask must hold B * T floats")
    w = torch.empty(B, T, dtype=torch.float32, device=hist.device)
    x_att = torch.empty_like(hist)
    check(lib().rec_dien_attention_seq_fwd(B, T, E, _p(score), _p(mask), _p(hist), float(scale), _p(w), _p(x_att),
                                           _stream()), "rec_dien_attention_seq_fwd")
    return w, x_att


def dien_softmax_weight_bwd(w, hist, dx_att, scale, d_hist, accumulate=True):
    """-> dscore [B,T] (the gradient of the attention MLP's output); d_hist (+)= w * dx_att (rec_dien_attention_seq_bwd)."""
    B, T, E = hist.shape
    _chk(w, torch.float32, "w", (B, T))
    _chk(hist, torch.float32, "hist")
    _chk(dx_att, torch.float32, "dx_att", (B, T, E))
    _chk(d_hist, torch.float32, "d_hist", (B, T, E))
    dscore = torch.empty(B, T, dtype=torch.float32, device=hist.device)
    check(lib().rec_dien_attention_seq_bwd(B, T, E, _p(w), _p(hist), _p(dx_att), float(scale), _p(dscore), _p(d_hist),
                                           int(bool(accumulate)), _stream()), "rec_dien_attention_seq_bwd")
    return dscore


def dien_attention_seq(hist, q, mask, att_w, att_b, ws):
    """DIEN's position-wise attention (dien/net.py:192-209): features, the attention MLP on rec_gemm_f32 (sigmoids in the
    epilogues), the scaled masked softmax over T and the weighting.  hist, q [B,T,E]; mask f32 [B,T] (0 / -1e9);
    att_w [4E,H1],[H1,H2],[H2,1].  -> (w [B,T], x_att [B,T,E], saved = (feat, a1, a2) for the backward)."""
    B, T, E = hist.shape
    feat = dien_att_feat_fwd(hist, q)
    a1 = gemm(feat, att_w[0], ws, epilogue="bias_sigmoid", bias=att_b[0])
    a2 = gemm(a1, att_w[1], ws, epilogue="bias_sigmoid", bias=att_b[1])
    score = gemm(a2, att_w[2], ws, epilogue="bias", bias=att_b[2])
    w, x_att = dien_softmax_weight_fwd(score, mask, hist, float(E) ** -0.5)
    return w, x_att, (feat, a1, a2)


def dien_attention_seq_bwd(hist, q, w, saved, att_w, dx_att, d_hist, ws, accumulate=True):
    """Backward of dien_attention_seq from dx_att [B,T,E]: d_hist (+)= the weighting's and the features' gradients;
    -> d_q [B,T,E].  The attention MLP's weights get no gradient (they are not parameters of the reference's model)."""
    B, T, E = hist.shape
    _, a1, a2 = saved
    dscore = dien_softmax_weight_bwd(w, hist, dx_att, float(E) ** -0.5, d_hist, accumulate=accumulate)
    d2 = gemm(dscore.view(B * T, 1), att_w[2], ws, trans_b=True, epilogue="dsigmoid", aux0=a2)
    d1 = gemm(d2, att_w[1], ws, trans_b=True, epilogue="dsigmoid", aux0=a1)
    dfeat = gemm(d1, att_w[0], ws, trans_b=True)
    return dien_att_feat_bwd(hist, q, dfeat, d_hist, accumulate=True)


# ------------------------------------------------------------------ DMR (rank/dmr): prefix pool, PReLU, match loss, tail glue
def _view_ld(t):
    """Row stride (floats / ids) of a 2-D view with unit column stride."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RecError("expected a 2-D view with unit column stride, got shape %s strides %s" % (tuple(t.shape), t.stride()))
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _dev(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise RecError("%s must be a device tensor (no CPU fallback)" % name)
    if t.dtype != dtype:
        raise RecError("%s must be %s, got %s" % (name, dtype, t.dtype))


def _pool_args(score, mask, hist, rows):
    _chk(score, torch.float32, "score")
    _dev(mask, torch.int64, "mask")
    _dev(hist, torch.float32, "hist")
    if hist.dim() != 3 or hist.stride(2) != 1 or (hist.shape[0] > 1 and hist.stride(0) != hist.shape[1] * hist.stride(1)):
        raise RecError("dmr prefix pool: hist must be [B, T, D] with one row stride")
    B, T, D = hist.shape
    if score.numel() != B * T or tuple(mask.shape) != (B, T):
        raise RecError("dmr prefix pool: score and mask must be [B, T]")
    rows = [int(r) for r in rows]
    if not 1 <= len(rows) <= 8 or any(not 0 <= r < T for r in rows):
        raise RecError("dmr prefix pool: rows must be 1..8 positions in [0, T), got %s" % (rows,))
    return B, T, D, rows, (C.c_int32 * len(rows))(*rows)


def dmr_prefix_pool_fwd(score, mask, hist, rows, out=None, rel=None):
    """Causal masked-softmax pooling for the listed query positions (rec_dmr_prefix_pool_fwd; dmr/net.py:259-281 and
    338-350).  score [B,T] f32, mask [B,T] i64 (valid iff 1; a strided view is fine), hist [B,T,D] (row stride allowed).
    out: a [B, R*D] view (row stride allowed) or None; rel: a [B,1] view (the sum of the raw scores at valid positions) or
    None.  -> (out [B,R*D], w [B,R,T])."""
    B, T, D, rows, crows = _pool_args(score, mask, hist, rows)
    R = len(rows)
    if out is None:
        out = torch.empty(B, R * D, dtype=torch.float32, device=hist.device)
    _dev(out, torch.float32, "out")
    _dev(rel, torch.float32, "rel")
    if tuple(out.shape) != (B, R * D) or (rel is not None and tuple(rel.shape) != (B, 1)):
        raise RecError("dmr prefix pool: out must be [B, R*D] and rel [B, 1]")
    w = torch.empty(B, R, T, dtype=torch.float32, device=hist.device)
    check(lib().rec_dmr_prefix_pool_fwd(B, T, D, _p(score), _p(mask), _view_ld(mask), _p(hist), hist.stride(1), R, crows,
                                        _p(out), _view_ld(out), _p(rel), _view_ld(rel) if rel is not None else 0, _p(w), _stream()),
          "rec_dmr_prefix_pool_fwd")
    return out, w


def dmr_prefix_pool_bwd(mask, hist, rows, w, d_out, d_hist, d_rel=None, accumulate=True):
    """Backward of dmr_prefix_pool_fwd: d_out [B, R*D] view, d_rel [B,1] view or None; d_hist [B,T,D] (row stride allowed)
    receives (accumulate: is added) sum_r w d_out.  -> dscore [B,T]."""
    B, T, D = hist.shape
    rows = [int(r) for r in rows]
    R = len(rows)
    _chk(w, torch.float32, "w", (B, R, T))
    for t, n in ((hist, "hist"), (d_out, "d_out"), (d_hist, "d_hist"), (d_rel, "d_rel")):
        _dev(t, torch.float32, n)
    _dev(mask, torch.int64, "mask")
    if tuple(d_out.shape) != (B, R * D) or tuple(d_hist.shape) != (B, T, D) or d_hist.stride(2) != 1 or \
            (B > 1 and d_hist.stride(0) != T * d_hist.stride(1)) or (d_rel is not None and tuple(d_rel.shape) != (B, 1)):
        raise RecError("dmr prefix pool bwd: d_out must be [B, R*D], d_hist [B, T, D] with one row stride, d_rel [B, 1]")
    if not 1 <= R <= 8 or any(not 0 <= r < T for r in rows):
        raise RecError("dmr prefix pool: rows must be 1..8 positions in [0, T), got %s" % (rows,))
    dscore = torch.empty(B, T, dtype=torch.float32, device=hist.device)
    check(lib().rec_dmr_prefix_pool_bwd(B, T, D, _p(mask), _view_ld(mask), _p(hist), hist.stride(1), R,
                                        (C.c_int32 * R)(*rows), _p(w), _p(d_out), _view_ld(d_out), _p(d_rel),
                                        _view_ld(d_rel) if d_rel is not None else 0, _p(dscore), _p(d_hist), d_hist.stride(1),
                                        int(bool(accumulate)), _stream()), "rec_dmr_prefix_pool_bwd")
    return dscore


def prelu_fwd(X, alpha, period=0, base=0, out=None):
    """paddle.nn.PReLU on X [m, n] (rec_prelu_fwd).  period 0: the channel is the column (alpha [n]); period > 0: the
    channel is base + row % period (axis 1 of a [B, period, n] input given as [B*period, n])."""
    ldx = _chk_mat(X, "X")
    _chk(alpha, torch.float32, "alpha")
    m, n = X.shape
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=X.device)
    check(lib().rec_prelu_fwd(m, n, _p(X), ldx, _p(alpha), alpha.numel(), int(period > 0), int(period), int(base), _p(out),
                              _chk_mat(out, "out"), _stream()), "rec_prelu_fwd")
    return out


def prelu_bwd(X, dY, alpha, ws, period=0, base=0, dalpha=None, out=None):
    """-> (dX, dalpha [alpha.numel()]): dX = x > 0 ? dy : alpha dy; dalpha[ch] = sum of dy x over x <= 0, every entry
    written (rec_prelu_bwd)."""
    ldx, lddy = _chk_mat(X, "X"), _chk_mat(dY, "dY")
    _chk(alpha, torch.float32, "alpha")
    m, n = X.shape
    if tuple(dY.shape) != (m, n):
        raise RecError("prelu_bwd: dY has shape %s, expected %s" % (tuple(dY.shape), (m, n)))
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=X.device)
    if dalpha is None:
        dalpha = torch.empty(alpha.numel(), dtype=torch.float32, device=X.device)
    _chk(dalpha, torch.float32, "dalpha")
    if dalpha.numel() != alpha.numel():
        raise RecError("prelu_bwd: dalpha must have alpha's size")
    nbytes = C.c_size_t(0)
    check(lib().rec_prelu_workspace_bytes(m, n, int(period > 0), int(period), C.byref(nbytes)), "rec_prelu_workspace_bytes")
    wk = ws.get(nbytes.value)
    check(lib().rec_prelu_bwd(m, n, _p(X), ldx, _p(dY), lddy, _p(alpha), alpha.numel(), int(period > 0), int(period),
                              int(base), _p(out), _chk_mat(out, "dX"), _p(dalpha), _p(wk), C.c_size_t(wk.numel()),
                              _stream()), "rec_prelu_bwd")
    return out, dalpha


def _match_args(U, V, bias, label):
    ldu, ldv = _chk_mat(U, "U"), _chk_mat(V, "V")
    B, K = U.shape
    Cn = V.shape[0]
    if V.shape[1] != K:
        raise RecError("dmr match loss: U is [B, %d] but V [C, %d]" % (K, V.shape[1]))
    _chk(bias, torch.float32, "bias", (Cn,))
    _dev(label, torch.int64, "label")
    if label.dim() != 1 or label.shape[0] != B:
        raise RecError("dmr match loss: label must be [B] (a strided view is fine)")
    fb, bb = C.c_size_t(0), C.c_size_t(0)
    check(lib().rec_dmr_match_loss_workspace_bytes(B, Cn, K, C.byref(fb), C.byref(bb)), "rec_dmr_match_loss_workspace_bytes")
    return B, Cn, K, ldu, ldv, (label.stride(0) if B > 1 else 1), fb.value, bb.value


def dmr_match_loss_fwd(U, V, bias, label, ws, status=None):
    """Mean softmax cross-entropy of U V^T + bias over ALL classes without a [B, C] buffer (rec_dmr_match_loss_fwd;
    dmr/net.py:298-301).  U [B,K], V [C,K], bias [C] or None, label [B] i64.  -> (loss [1], lse [B], status)."""
    B, Cn, K, ldu, ldv, ldl, fb, _ = _match_args(U, V, bias, label)
    loss = torch.empty(1, dtype=torch.float32, device=U.device)
    lse = torch.empty(B, dtype=torch.float32, device=U.device)
    if status is None:
        status = new_status(U.device)
    wk = ws.get(fb)
    check(lib().rec_dmr_match_loss_fwd(B, Cn, K, _p(U), ldu, _p(V), ldv, _p(bias), _p(label), ldl, _p(loss), _p(lse),
                                       _p(status), _p(wk), C.c_size_t(wk.numel()), _stream()), "rec_dmr_match_loss_fwd")
    return loss, lse, status


def dmr_match_loss_bwd(U, V, bias, label, lse, d_loss, dV, ws, accumulate=False):
    """Backward of dmr_match_loss_fwd (the logits are recomputed): dV [C,K] (row stride allowed) receives (accumulate: is
    added) the DENSE gradient of every class row.  -> dU [B,K]."""
    B, Cn, K, ldu, ldv, ldl, _, bb = _match_args(U, V, bias, label)
    _chk(lse, torch.float32, "lse", (B,))
    lddv = _chk_mat(dV, "dV")
    if tuple(dV.shape) != (Cn, K):
        raise RecError("dmr match loss: dV must be [C, K]")
    dU = torch.empty(B, K, dtype=torch.float32, device=U.device)
    wk = ws.get(bb)
    check(lib().rec_dmr_match_loss_bwd(B, Cn, K, _p(U), ldu, _p(V), ldv, _p(bias), _p(label), ldl, _p(lse), float(d_loss),
                                       _p(dU), K, _p(dV), lddv, int(bool(accumulate)), _p(wk), C.c_size_t(wk.numel()),
                                       _stream()), "rec_dmr_match_loss_bwd")
    return dU


def dmr_tail_fwd(hist, item_eb, uv, match_mask, V, cate_id, hist_sum, prod, rel_u2i, status):
    """The glue of DMR's tower input (rec_dmr_tail_fwd): hist_sum = sum_t hist (unmasked), prod = item_eb * hist_sum,
    rel_u2i = uv[:,1] . V[cate_id], all written into the given [B, .] views; -> U2 [B,E] = uv[:,0] * match_mask.
    hist [B,T,2E]; item_eb, hist_sum, prod [B,2E] views; uv [B,2,E]; match_mask [B,1] i64 view; rel_u2i [B,1] view."""
    B, T, D = hist.shape
    _chk(uv, torch.float32, "uv", (B, 2, D // 2))
    _chk(cate_id, torch.int64, "cate_id", (B,))
    for t, n in ((hist, "hist"), (item_eb, "item_eb"), (hist_sum, "hist_sum"), (prod, "prod"), (rel_u2i, "rel_u2i")):
        _dev(t, torch.float32, n)
    _dev(match_mask, torch.int64, "match_mask")
    ldv = _chk_mat(V, "V")
    if D % 2 or V.shape[1] != D // 2 or any(tuple(t.shape) != (B, D) for t in (item_eb, hist_sum, prod)) or \
            tuple(rel_u2i.shape) != (B, 1) or tuple(match_mask.shape) != (B, 1):
        raise RecError("dmr_tail_fwd: shapes do not fit hist [B, T, 2E]")
    if hist.stride(2) != 1 or (B > 1 and hist.stride(0) != T * hist.stride(1)):     # the kernel walks sample b at b * T * ldh
        raise RecError("dmr_tail_fwd: hist must be [B, T, D] with one row stride")
    U2 = torch.empty(B, D // 2, dtype=torch.float32, device=hist.device)
    check(lib().rec_dmr_tail_fwd(B, T, D, _p(hist), hist.stride(1), _p(item_eb), _view_ld(item_eb), _p(uv), _p(match_mask),
                                 _view_ld(match_mask), _p(V), ldv, V.shape[0], _p(cate_id), _p(hist_sum), _view_ld(hist_sum), _p(prod),
                                 _view_ld(prod), _p(rel_u2i), _view_ld(rel_u2i), _p(U2), _p(status), _stream()), "rec_dmr_tail_fwd")
    return U2


def dmr_tail_bwd_match(dU2, d_rel, uv, match_mask, V, cate_id, dV_rows):
    """-> d_uv [B,2,E]: row 0 = dU2 * match_mask (dU2 None: 0), row 1 = d_rel V[cate_id]; dV_rows [B,E] view = d_rel
    uv[:,1] (rec_dmr_tail_bwd_match)."""
    B, _, E = uv.shape
    _chk(uv, torch.float32, "uv")
    _chk(dU2, torch.float32, "dU2", (B, E))
    _chk(cate_id, torch.int64, "cate_id", (B,))
    _dev(d_rel, torch.float32, "d_rel")
    _dev(dV_rows, torch.float32, "dV_rows")
    _dev(match_mask, torch.int64, "match_mask")
    if tuple(d_rel.shape) != (B, 1) or tuple(dV_rows.shape) != (B, E) or tuple(match_mask.shape) != (B, 1):
        raise RecError("dmr_tail_bwd_match: d_rel / match_mask must be [B, 1] and dV_rows [B, E]")
    if uv.shape[1] != 2 or V.dim() != 2 or V.shape[1] != E:           # the kernel reads E floats of a row of V per sample
        raise RecError("dmr_tail_bwd_match: uv must be [B, 2, E] and V [C, E]")
    d_uv = torch.empty(B, 2, E, dtype=torch.float32, device=uv.device)
    check(lib().rec_dmr_tail_bwd_match(B, E, _p(dU2), _p(d_rel), _view_ld(d_rel), _p(uv), _p(match_mask), _view_ld(match_mask), _p(V),
                                       _chk_mat(V, "V"), V.shape[0], _p(cate_id), _p(d_uv), _p(dV_rows), _view_ld(dV_rows),
                                       _stream()), "rec_dmr_tail_bwd_match")
    return d_uv


def dmr_tail_bwd_hist(f1, f2, d_sum, d_prod, item_eb, hist_sum, d_item_direct, d_ctx, d_hist, d_item):
    """d_hist [B,T,D] += f1 + f2 + d_sum + d_prod * item_eb (broadcast over T); d_item [B,D] = d_item_direct + d_prod *
    hist_sum + sum_t d_ctx[b,t,:D] (rec_dmr_tail_bwd_hist).  f1, f2 [B,T,D] contiguous or None; d_ctx [B*T, >= D] view."""
    B, T, D = d_hist.shape
    _chk(f1, torch.float32, "f1", (B, T, D))
    _chk(f2, torch.float32, "f2", (B, T, D))
    for t, n in ((d_sum, "d_sum"), (d_prod, "d_prod"), (item_eb, "item_eb"), (hist_sum, "hist_sum"),
                 (d_item_direct, "d_item_direct"), (d_item, "d_item")):
        _dev(t, torch.float32, n)
        if tuple(t.shape) != (B, D):
            raise RecError("dmr_tail_bwd_hist: %s must be [B, D]" % n)
    _dev(d_ctx, torch.float32, "d_ctx")
    _dev(d_hist, torch.float32, "d_hist")
    if d_ctx.shape[0] != B * T or d_ctx.shape[1] < D or d_hist.stride(2) != 1 or \
            (B > 1 and d_hist.stride(0) != T * d_hist.stride(1)):
        raise RecError("dmr_tail_bwd_hist: d_ctx must be [B*T, >= D] and d_hist [B, T, D] with one row stride")
    check(lib().rec_dmr_tail_bwd_hist(B, T, D, _p(f1), _p(f2), _p(d_sum), _view_ld(d_sum), _p(d_prod), _view_ld(d_prod), _p(item_eb),
                                      _view_ld(item_eb), _p(hist_sum), _view_ld(hist_sum), _p(d_item_direct), _view_ld(d_item_direct),
                                      _p(d_ctx), _view_ld(d_ctx), _p(d_hist), d_hist.stride(1), _p(d_item), _view_ld(d_item),
                                      _stream()), "rec_dmr_tail_bwd_hist")


# ------------------------------------------------------------------ BST: attention, add + layer norm, LeakyReLU, glue
MHA_MAX_L, MHA_MAX_D = 8192, 64


def _rows_view(t, name):
    """A 2-D float32 device view with unit column stride -> its row stride."""
    _dev(t, torch.float32, name)
    return _view_ld(t)


def _mha_args(q, k, v, B, L, H, what):
    ldq, ldk, ldv = _rows_view(q, "q"), _rows_view(k, "k"), _rows_view(v, "v")
    if B < 0 or L < 1 or H < 1 or q.shape[0] != B * L or k.shape != q.shape or v.shape[0] != B * L \
            or q.shape[1] % H or v.shape[1] % H:
        raise RecError("%s: q, k must be [B*L, H*d_k] and v [B*L, H*d_v] (B %d, L %d, H %d; got %s, %s, %s)"
                       % (what, B, L, H, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    return q.shape[1] // H, v.shape[1] // H, ldq, ldk, ldv


def mha_fwd(q, k, v, B, L, H, scale=1.0, p=0.0, seed=0, stream=0, out=None):
    """Multi-head attention over [B, L] tokens without an [B,H,L,L] buffer (rec_mha_fwd).  q, k [B*L, H*d_k], v [B*L, H*d_v]:
    2-D views with a row stride (column ranges of one packed projection output, or separate matrices).  p > 0: dropout on
    the softmax weights with rec_dropout's keep rule over a virtual [B*H*L, L] matrix.  -> (out [B*L, H*d_v], lse [B,H,L])."""
    dk, dv, ldq, ldk, ldv = _mha_args(q, k, v, B, L, H, "mha_fwd")
    if out is None:
        out = torch.empty(B * L, H * dv, dtype=torch.float32, device=q.device)
    ldo = _rows_view(out, "out")
    if tuple(out.shape) != (B * L, H * dv):
        raise RecError("mha_fwd: out must be [B*L, H*d_v]")
    lse = torch.empty(B, H, L, dtype=torch.float32, device=q.device)
    check(lib().rec_mha_fwd(B, L, H, dk, dv, _p(q), ldq, _p(k), ldk, _p(v), ldv, float(scale), float(p), int(seed), int(stream),
                            _p(out), ldo, _p(lse), _stream()), "rec_mha_fwd")
    return out, lse


def mha_bwd(q, k, v, B, L, H, out, lse, d_out, scale=1.0, p=0.0, seed=0, stream=0, grads=None):
    """Backward of mha_fwd (the weights are recomputed from lse; `out` is the forward's output).  grads: (dq, dk, dv) views
    to write (e.g. column ranges of one packed gradient) or None.  -> (dq, dk, dv)."""
    dk_, dv_, ldq, ldk, ldv = _mha_args(q, k, v, B, L, H, "mha_bwd")
    _chk(lse, torch.float32, "lse", (B, H, L))
    if grads is None:
        grads = (torch.empty(B * L, H * dk_, dtype=torch.float32, device=q.device),
                 torch.empty(B * L, H * dk_, dtype=torch.float32, device=q.device),
                 torch.empty(B * L, H * dv_, dtype=torch.float32, device=q.device))
    dq, dk, dv = grads
    for t, n, w in ((out, "out", dv_), (d_out, "d_out", dv_), (dq, "dq", dk_), (dk, "dk", dk_), (dv, "dv", dv_)):
        _rows_view(t, n)
        if tuple(t.shape) != (B * L, H * w):
            raise RecError("mha_bwd: %s must be [B*L, %d], got %s" % (n, H * w, tuple(t.shape)))
    delta = torch.empty(B, H, L, dtype=torch.float32, device=q.device)
    check(lib().rec_mha_bwd(B, L, H, dk_, dv_, _p(q), ldq, _p(k), ldk, _p(v), ldv, float(scale), float(p), int(seed), int(stream),
                            _p(out), _view_ld(out), _p(d_out), _view_ld(d_out), _p(lse), _p(delta), _p(dq), _view_ld(dq),
                            _p(dk), _view_ld(dk), _p(dv), _view_ld(dv), _stream()), "rec_mha_bwd")
    return dq, dk, dv


def _y_group(y, m, n, group):
    """out=(tensor, group): row i of y is row 1 + i % group of sample i // group of a [B, group + 1, n] tower input."""
    if group <= 0:
        return _rows_view(y, "y"), 0, 0
    _chk(y, torch.float32, "y")
    if y.dim() != 3 or y.shape[1] != group + 1 or y.shape[2] != n or y.shape[0] * group != m:
        raise RecError("grouped y must be [m / group, group + 1, n]")
    return n, group, (group + 1) * n


def add_layer_norm_fwd(x, r=None, eps=1e-5, out=None, out_group=0):
    """y = LN(x + r) over the last axis, no affine parameters, biased variance (rec_add_layer_norm_fwd).  x, r [m, n] views
    (r may be None); out may be x.  out_group G > 0: out is a [m / G, G + 1, n] tensor whose rows 1.. of every sample are
    written.  -> (y, mean [m], rstd [m])."""
    ldx = _rows_view(x, "x")
    m, n = x.shape
    if r is not None and (tuple(r.shape) != (m, n)):
        raise RecError("add_layer_norm_fwd: r must have x's shape")
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    ldy, g, ldg = _y_group(out, m, n, out_group)
    if not g and tuple(out.shape) != (m, n):
        raise RecError("add_layer_norm_fwd: out must have x's shape")
    mean = torch.empty(m, dtype=torch.float32, device=x.device)
    rstd = torch.empty(m, dtype=torch.float32, device=x.device)
    yp = C.c_void_p(out.data_ptr() + n * 4) if g else _p(out)            # grouped: row 1 of sample 0
    check(lib().rec_add_layer_norm_fwd(m, n, _p(x), ldx, _p(r), _rows_view(r, "r") if r is not None else 0, float(eps), yp, ldy,
                                       g, ldg, _p(mean), _p(rstd), _stream()), "rec_add_layer_norm_fwd")
    return out, mean, rstd


def add_layer_norm_bwd(y, rstd, dy, out=None, y_group=0):
    """-> dx [m, n] = rstd (dy - mean(dy) - y mean(dy y)): the gradient of x + r (rec_add_layer_norm_bwd).  out may be dy."""
    lddy = _rows_view(dy, "dy")
    m, n = dy.shape
    ldy, g, ldg = _y_group(y, m, n, y_group)
    _chk(rstd, torch.float32, "rstd", (m,))
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=dy.device)
    if tuple(out.shape) != (m, n) or (not g and tuple(y.shape) != (m, n)):
        raise RecError("add_layer_norm_bwd: y, dy and out must have one shape")
    check(lib().rec_add_layer_norm_bwd(m, n, C.c_void_p(y.data_ptr() + n * 4) if g else _p(y), ldy, g, ldg, _p(rstd), _p(dy), lddy, _p(out),
                                       _rows_view(out, "out"), _stream()), "rec_add_layer_norm_bwd")
    return out


def leaky_relu_fwd(x, slope=0.01, out=None):
    """paddle.nn.LeakyReLU on a [m, n] view (rec_leaky_relu_fwd); in place by default."""
    ldx = _rows_view(x, "x")
    if out is None:
        out = x
    if out.shape != x.shape:
        raise RecError("leaky_relu_fwd: out must have x's shape")
    check(lib().rec_leaky_relu_fwd(x.shape[0], x.shape[1], _p(x), ldx, float(slope), _p(out), _rows_view(out, "out"), _stream()),
          "rec_leaky_relu_fwd")
    return out


def leaky_relu_bwd(y, dy, slope=0.01, out=None):
    """dx = y > 0 ? dy : slope dy, from the OUTPUT y (rec_leaky_relu_bwd); in place on dy by default."""
    ldy, lddy = _rows_view(y, "y"), _rows_view(dy, "dy")
    if out is None:
        out = dy
    if out.shape != y.shape or dy.shape != y.shape:
        raise RecError("leaky_relu_bwd: y, dy and out must have one shape")
    check(lib().rec_leaky_relu_bwd(y.shape[0], y.shape[1], _p(y), ldy, _p(dy), lddy, float(slope), _p(out), _rows_view(out, "out"),
                                   _stream()), "rec_leaky_relu_bwd")
    return out


def bst_add(x, r=None, out=None):
    """out = x + r over [m, n] views (r None: a strided copy); in place on x by default (rec_bst_add)."""
    ldx = _rows_view(x, "x")
    if out is None:
        out = x
    if out.shape != x.shape or (r is not None and r.shape != x.shape):
        raise RecError("bst_add: x, r and out must have one shape")
    check(lib().rec_bst_add(x.shape[0], x.shape[1], _p(x), ldx, _p(r), _rows_view(r, "r") if r is not None else 0, _p(out),
                            _rows_view(out, "out"), _stream()), "rec_bst_add")
    return out


def _bst_widths(tables):
    w = [int(tables[i].shape[1]) for i in range(3)]
    if [int(tables[i].shape[1]) for i in range(3, 6)] != w or tables[6].shape[1] != sum(w):
        raise RecError("bst: the target tables must have the hist tables' widths and the user table their sum")
    return w


def bst_embed_fwd(ids, tables, X, Z, status):
    """The seven lookups of BST (rec_bst_embed_fwd).  ids: hist item / cat / position [B,T] i64 (strided views are fine),
    target item / cat / position and user [B] or [B,1] i64; tables: the seven weights in the same order.  X [B*(T+1),
    d_model] receives [item | cat | position] per position (the target last), Z [B, T+2, d_model] its row 0 = the user row."""
    B, T = ids[0].shape
    w = _bst_widths(tables)
    dm = sum(w)
    ld = []
    for i, t in enumerate(ids):
        _dev(t, torch.int64, "ids[%d]" % i)
        if i < 3:
            if tuple(t.shape) != (B, T) or (T > 1 and t.stride(1) != 1):
                raise RecError("bst_embed_fwd: the history ids must be [B, T] with unit column stride")
        elif t.numel() != B or t.dim() not in (1, 2):
            raise RecError("bst_embed_fwd: the target and user ids must be [B] or [B, 1]")
        ld.append(t.stride(0) if B > 1 else max(T, 1))
    for i, t in enumerate(tables):
        _chk(t, torch.float32, "tables[%d]" % i)
    _chk(X, torch.float32, "X", (B * (T + 1), dm))
    _chk(Z, torch.float32, "Z", (B, T + 2, dm))
    check(lib().rec_bst_embed_fwd(B, T, (C.c_void_p * 7)(*[_p(t) for t in ids]), (C.c_int64 * 7)(*ld),
                                  (C.c_void_p * 7)(*[_p(t) for t in tables]), (C.c_int64 * 7)(*[t.shape[0] for t in tables]),
                                  (C.c_int32 * 3)(*w), _p(X), dm, _p(Z), (T + 2) * dm, _p(status), _stream()), "rec_bst_embed_fwd")


def bst_embed_bwd(dX, B, T, widths):
    """dX [B*(T+1), d_model] -> the contiguous gradient rows of the six sequence lookups: three [B*T, w], three [B, w]
    (rec_bst_embed_bwd)."""
    lddx = _rows_view(dX, "dX")
    w = [int(x) for x in widths]
    if tuple(dX.shape) != (B * (T + 1), sum(w)):
        raise RecError("bst_embed_bwd: dX must be [B*(T+1), d_model]")
    g = [torch.empty(B * T, x, dtype=torch.float32, device=dX.device) for x in w] + \
        [torch.empty(B, x, dtype=torch.float32, device=dX.device) for x in w]
    check(lib().rec_bst_embed_bwd(B, T, (C.c_int32 * 3)(*w), _p(dX), lddx, (C.c_void_p * 6)(*[_p(t) for t in g]), _stream()),
          "rec_bst_embed_bwd")
    return g


def bst_possum_fwd(z, bias, B):
    """y [B,1] = sum over the positions of z [B*P, 1] + bias [1] (rec_bst_possum_fwd)."""
    _chk(z, torch.float32, "z")
    _chk(bias, torch.float32, "bias", (1,))
    if B < 0 or (B and z.numel() % B):
        raise RecError("bst_possum_fwd: z must hold B * P logits")
    y = torch.empty(B, 1, dtype=torch.float32, device=z.device)
    check(lib().rec_bst_possum_fwd(B, z.numel() // max(B, 1), _p(z), _p(bias), _p(y), _stream()), "rec_bst_possum_fwd")
    return y


def bst_possum_bwd(dy, P, dbias):
    """-> dz [B*P, 1] = dy broadcast over the positions; dbias [1] = sum_b dy (rec_bst_possum_bwd)."""
    _chk(dy, torch.float32, "dy")
    _chk(dbias, torch.float32, "dbias", (1,))
    B = dy.numel()
    dz = torch.empty(B * P, 1, dtype=torch.float32, device=dy.device)
    check(lib().rec_bst_possum_bwd(B, int(P), _p(dy), _p(dz), _p(dbias), _stream()), "rec_bst_possum_bwd")
    return dz


# ------------------------------------------------------------------ multitask (mmoe, ple): expert-gate mixture, two-class head
class MtlMix:
    """The slot map of rec_mtl_mix_fwd / rec_mtl_mix_bwd (rec_mtl_mix_desc): expert_size S, n_slots column blocks of S
    floats in H, and per gate (first0, count0, first1, count1) — the gate mixes the slots [first0, first0 + count0) then
    [first1, first1 + count1).  n_logit: the columns of the logits / probabilities (the gates' expert counts, summed)."""

    def __init__(self, expert_size, n_slots, gates):
        self.expert_size, self.n_slots = int(expert_size), int(n_slots)
        self.gates = [tuple(int(x) for x in (tuple(g) + (0, 0))[:4]) for g in gates]
        self.n_gates = len(self.gates)
        self.n_logit = sum(g[1] + g[3] for g in self.gates)

    def desc(self, batch, ld_h=0, ld_logit=0, ld_prob=0, ld_out=0, ld_dh=0, ld_dlogit=0):
        d = MtlMixDesc(int(batch), self.expert_size, self.n_slots, self.n_gates, ld_h, ld_logit, ld_prob, ld_out, ld_dh,
                       ld_dlogit)
        for i, g in enumerate(self.gates[:_lib.REC_MTL_MAX_GATES]):
            d.first0[i], d.count0[i], d.first1[i], d.count1[i] = g
        return d


def _mtl_view(t, B, cols, name):
    """[B, cols] float32 device view with unit column stride -> its row stride (0 = packed where one row hides it)."""
    ld = _rows_view(t, name)
    if tuple(t.shape) != (B, cols):
        raise RecError("%s has shape %s, expected %s" % (name, tuple(t.shape), (B, cols)))
    return ld if B > 1 else 0


def mtl_mix_fwd(mix, H, logits, prob=None, out=None):
    """Gate softmax + gate-weighted sum of expert outputs (rec_mtl_mix_fwd).  H [B, n_slots*S] and logits [B, n_logit] are
    2-D views with a row stride (column ranges of the packed GEMM's output); prob [B, n_logit] and out [B, n_gates*S] are
    allocated when None.  -> (prob, out)."""
    B = H.shape[0]
    f32 = dict(dtype=torch.float32, device=H.device)
    if prob is None:
        prob = torch.empty(B, mix.n_logit, **f32)
    if out is None:
        out = torch.empty(B, mix.n_gates * mix.expert_size, **f32)
    d = mix.desc(B, _mtl_view(H, B, mix.n_slots * mix.expert_size, "H"), _mtl_view(logits, B, mix.n_logit, "logits"),
                 _mtl_view(prob, B, mix.n_logit, "prob"), _mtl_view(out, B, mix.n_gates * mix.expert_size, "out"))
    check(lib().rec_mtl_mix_fwd(C.byref(d), _p(H), _p(logits), _p(prob), _p(out), _stream()), "rec_mtl_mix_fwd")
    return prob, out


def mtl_mix_bwd(mix, H, prob, dmix, relu=True, dH=None, dlogits=None):
    """Backward of mtl_mix_fwd (rec_mtl_mix_bwd): dH [B, n_slots*S] (masked by H > 0 when relu) and dlogits [B, n_logit],
    views with a row stride — the two column ranges of the packed image's output gradient.  -> (dH, dlogits)."""
    B = H.shape[0]
    f32 = dict(dtype=torch.float32, device=H.device)
    if dH is None:
        dH = torch.empty(B, mix.n_slots * mix.expert_size, **f32)
    if dlogits is None:
        dlogits = torch.empty(B, mix.n_logit, **f32)
    d = mix.desc(B, _mtl_view(H, B, mix.n_slots * mix.expert_size, "H"), 0, _mtl_view(prob, B, mix.n_logit, "prob"),
                 _mtl_view(dmix, B, mix.n_gates * mix.expert_size, "dmix"),
                 _mtl_view(dH, B, mix.n_slots * mix.expert_size, "dH"), _mtl_view(dlogits, B, mix.n_logit, "dlogits"))
    check(lib().rec_mtl_mix_bwd(C.byref(d), _p(H), _p(prob), _p(dmix), int(bool(relu)), _p(dH), _p(dlogits), _stream()),
          "rec_mtl_mix_bwd")
    return dH, dlogits


def mtl_head(logits, label, grad_scale=1.0, want_grad=True):
    """The head of the multitask nets (rec_mtl_head): logits [B, 2T] and label [B, T] float32 views with a row stride.
    -> (pred [B, 2T] clipped softmax, cost [B, T] log loss of column 1, dlogits [B, 2T] = d(grad_scale * cost) or None)."""
    B, T = label.shape
    f32 = dict(dtype=torch.float32, device=logits.device)
    ld, ldl = _mtl_view(logits, B, 2 * T, "logits"), _mtl_view(label, B, T, "label")
    pred, cost = torch.empty(B, 2 * T, **f32), torch.empty(B, T, **f32)
    dl = torch.empty(B, 2 * T, **f32) if want_grad else None
    check(lib().rec_mtl_head(B, T, _p(logits), ld, _p(label), ldl, float(grad_scale), _p(pred), _p(cost), _p(dl), _stream()),
          "rec_mtl_head")
    return pred, cost, dl


# ------------------------------------------------------------------ entire-space multitask (esmm, escm2): field pool, head
ESM_MODES = {"ESMM": _lib.REC_ESM_ESMM, "IPW": _lib.REC_ESM_IPW, "DR": _lib.REC_ESM_DR}


def field_sumpool_fwd(ids, W, padding_idx, out=None, status=None):
    """Padded multi-field sum-pool (rec_field_sumpool_fwd): ids [B, F, L] int64, W [N, D] -> out [B, F*D] with
    out[b, f*D:(f+1)*D] = sum_l W[ids[b, f, l]], ids equal to padding_idx (None: no padding id) skipped; an id outside
    [0, N) is flagged in status, skipped and never read.  out: a [B, F*D] view with a row stride (allocated packed when
    None).  -> (out, status)."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 3:
        raise RecError("ids must be [B, F, L], got %s" % (tuple(ids.shape),))
    B, F, L = ids.shape
    D, rs = _chk_table(W, "W")
    if W.dim() != 2:
        raise RecError("W must be [N, D]")
    if out is None:
        out = torch.empty(B, F * D, dtype=torch.float32, device=W.device)
    ld = _mtl_view(out, B, F * D, "out")
    if status is None:
        status = new_status(W.device)
    check(lib().rec_field_sumpool_fwd(B, F, L, D, rs, W.shape[0], -1 if padding_idx is None else int(padding_idx), _p(ids),
                                      _p(W), _p(out), ld, _p(status), _stream()), "rec_field_sumpool_fwd")
    return out, status


def esm_head(logits, click, buy, mode, global_w=1.0, counterfactual_w=0.0, grad_scale=1.0, want_grad=True, click_count=None):
    """The entire-space head (rec_esm_head).  logits [B, 2G] float32 view with a row stride (G = 3 in mode "DR", else 2),
    click / buy [B] int64, mode "ESMM" | "IPW" | "DR".  -> (pred [B, 2G+2], cost [B, 3], dlogits [B, 2G] = d(grad_scale *
    (cost0 + counterfactual_w cost1 + global_w cost2)) or None).  click_count: int64 [1] that receives sum(click); when None
    it is allocated here in the IPW mode, the only one that reads it, and the other modes skip the count."""
    if mode not in ESM_MODES:
        raise RecError("esm_head: unknown mode %r (ESMM, IPW, DR)" % (mode,))
    G = 3 if mode == "DR" else 2
    B = logits.shape[0]
    ld = _mtl_view(logits, B, 2 * G, "logits")
    _chk(click, torch.int64, "click", (B,))
    _chk(buy, torch.int64, "buy", (B,))
    dev = logits.device
    if click_count is None and mode == "IPW":
        click_count = torch.empty(1, dtype=torch.int64, device=dev)
    _chk(click_count, torch.int64, "click_count", (1,))
    pred = torch.empty(B, 2 * G + 2, dtype=torch.float32, device=dev)
    cost = torch.empty(B, 3, dtype=torch.float32, device=dev)
    dl = torch.empty(B, 2 * G, dtype=torch.float32, device=dev) if want_grad else None
    d = EsmHeadDesc(B, ESM_MODES[mode], ld, float(global_w), float(counterfactual_w), float(grad_scale))
    check(lib().rec_esm_head(C.byref(d), _p(logits), _p(click), _p(buy), _p(click_count), _p(pred), _p(cost), _p(dl), _stream()),
          "rec_esm_head")
    return pred, cost, dl


# ------------------------------------------------------------------ AITM: per-field gather, AIT block, head, wide AUC buckets
def field_gather_fwd(ids, W, field_begin, out=None, rows_out=None, status=None):
    """One lookup per field over tables of unequal size kept in one buffer (rec_field_gather_fwd): ids [B, F] int64, W
    [sum vocab, D], field_begin [F + 1] int64 on the device -> out [B, F*D] with out[b, f*D:(f+1)*D] = W[field_begin[f] +
    ids[b, f]].  There is no padding id.  An id outside ITS field's [0, vocab_f) is flagged in status, never read, gives a
    zero row and -1 in rows_out; otherwise rows_out [B*F] int64 holds the global row (allocated here when None: it is what
    ids_group(rows_out, sum vocab, None, ...) groups for the backward).  out: a [B, F*D] view with a row stride (allocated
    packed when None).  -> (out, rows_out, status)."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2:
        raise RecError("ids must be [B, F], got %s" % (tuple(ids.shape),))
    B, F = ids.shape
    D, rs = _chk_table(W, "W")
    if W.dim() != 2:
        raise RecError("W must be [N, D]")
    _chk(field_begin, torch.int64, "field_begin", (F + 1,))
    if out is None:
        out = torch.empty(B, F * D, dtype=torch.float32, device=W.device)
    ld = _mtl_view(out, B, F * D, "out")
    if rows_out is None:
        rows_out = torch.empty(B * F, dtype=torch.int64, device=W.device)
    _chk(rows_out, torch.int64, "rows_out", (B * F,))
    if status is None:
        status = new_status(W.device)
    check(lib().rec_field_gather_fwd(B, F, D, rs, _p(field_begin), _p(ids), _p(W), _p(out), ld, _p(rows_out), _p(status),
                                     _stream()), "rec_field_gather_fwd")
    return out, rows_out, status


def _ait_args(QKV, tokens, what):
    T = int(tokens)
    if QKV.dim() != 2 or QKV.shape[1] % 3 or QKV.shape[0] % max(T, 1):
        raise RecError("%s: QKV must be [B * tokens, 3 * dim], got %s with tokens %d" % (what, tuple(QKV.shape), T))
    B, d = QKV.shape[0] // max(T, 1), QKV.shape[1] // 3
    return B, T, d, _mtl_view(QKV, B * T, 3 * d, "QKV")


def ait_fwd(QKV, tokens, out=None, prob=None):
    """The adaptive information transfer block (rec_ait_fwd): QKV [B * tokens, 3 dim], a float32 view with a row stride whose
    row b * tokens + t is Q_t | K_t | V_t of sample b.  a = softmax_t(<Q_t, K_t> / sqrt(dim)), out[b] = sum_t a_t V_t.
    -> (out [B, dim] (a view with a row stride when given), prob [B, tokens])."""
    B, T, d, ld = _ait_args(QKV, tokens, "ait_fwd")
    f32 = dict(dtype=torch.float32, device=QKV.device)
    if out is None:
        out = torch.empty(B, d, **f32)
    if prob is None:
        prob = torch.empty(B, T, **f32)
    _chk(prob, torch.float32, "prob", (B, T))
    check(lib().rec_ait_fwd(B, T, d, _p(QKV), ld, _p(out), _mtl_view(out, B, d, "out"), _p(prob), _stream()), "rec_ait_fwd")
    return out, prob


def ait_bwd(QKV, prob, d_out, tokens, out=None):
    """Backward of ait_fwd (rec_ait_bwd): d_out [B, dim] -> dQKV [B * tokens, 3 dim] in QKV's column layout (a view with a
    row stride when given).  With one token, dQ and dK are exactly zero."""
    B, T, d, ld = _ait_args(QKV, tokens, "ait_bwd")
    _chk(prob, torch.float32, "prob", (B, T))
    if out is None:
        out = torch.empty(B * T, 3 * d, dtype=torch.float32, device=QKV.device)
    check(lib().rec_ait_bwd(B, T, d, _p(QKV), ld, _p(prob), _p(d_out), _mtl_view(d_out, B, d, "d_out"), _p(out),
                            _mtl_view(out, B * T, 3 * d, "dQKV"), _stream()), "rec_ait_bwd")
    return out


def aitm_head(tower_click, ait, w_click, b_click, w_conv, b_conv, click, buy, constraint_w=0.6, grad_scale=1.0, want_grad=True):
    """AITM's coupled head (rec_aitm_head): tower_click, ait [B, dim] float32 views with a row stride; w_click, w_conv [dim]
    (or [dim, 1]) and b_click, b_conv [1] contiguous; click, buy [B] int64.  -> (pred [B, 2] = pCTR | pCVR, cost [B, 3] =
    BCE(pCTR, click) | BCE(pCVR, buy) | max(pCVR - pCTR, 0), dz [B, 2] = d(grad_scale (cost0 + cost1) + constraint_w cost2) by
    the two logits, or None)."""
    B, d = tower_click.shape
    ldc, lda = _mtl_view(tower_click, B, d, "tower_click"), _mtl_view(ait, B, d, "ait")
    for t, n in ((w_click, "w_click"), (w_conv, "w_conv")):
        _chk(t, torch.float32, n)
        if t.numel() != d:
            raise RecError("%s has %d elements, expected %d" % (n, t.numel(), d))
    for t, n in ((b_click, "b_click"), (b_conv, "b_conv")):
        _chk(t, torch.float32, n)
        if t.numel() != 1:
            raise RecError("%s must hold one element" % n)
    _chk(click, torch.int64, "click", (B,))
    _chk(buy, torch.int64, "buy", (B,))
    f32 = dict(dtype=torch.float32, device=tower_click.device)
    pred, cost = torch.empty(B, 2, **f32), torch.empty(B, 3, **f32)
    dz = torch.empty(B, 2, **f32) if want_grad else None
    desc = AitmHeadDesc(B, d, ldc, lda, float(constraint_w), float(grad_scale))
    check(lib().rec_aitm_head(C.byref(desc), _p(tower_click), _p(ait), _p(w_click), _p(b_click), _p(w_conv), _p(b_conv),
                              _p(click), _p(buy), _p(pred), _p(cost), _p(dz), _stream()), "rec_aitm_head")
    return pred, cost, dz


def auc_histogram_wide(pred, label, stat_pos, stat_neg, num_thresholds=100000):
    """auc_histogram's buckets for any 1 <= num_thresholds <= 2^24 (rec_auc_histogram_wide: integer global atomics instead of
    LDS histograms).  pred: float32 [B], or a column of a 2-D tensor (its element stride is passed on: no copy)."""
    _dev(pred, torch.float32, "pred")
    if pred.dim() != 1:
        raise RecError("pred must be [B] (a column view is fine), got %s" % (tuple(pred.shape),))
    B = pred.shape[0]
    ld = pred.stride(0) if B > 1 else 1
    if ld < 1:
        raise RecError("pred must have a positive stride")
    _chk(label, torch.int64, "label", (B,))
    _chk(stat_pos, torch.int64, "stat_pos", (num_thresholds + 1,))
    _chk(stat_neg, torch.int64, "stat_neg", (num_thresholds + 1,))
    check(lib().rec_auc_histogram_wide(B, _p(pred), ld, _p(label), int(num_thresholds), _p(stat_pos), _p(stat_neg),
                                       _stream()), "rec_auc_histogram_wide")


# ------------------------------------------------------------------ MIND: capsule routing, label-aware attention, sampled softmax
def mind_routing_fwd(low, seq_len, routing_logits, iters):
    """MIND's dynamic routing in one launch (rec_mind_routing_fwd).  low [B * T, H]: a float32 view with a row stride, row
    b * T + t the mapped history item t of sample b; seq_len [B] int64; routing_logits [K, T] (or [1, K, T]) contiguous.
    -> (W [B, K, T] the final coupling weights, Z [B, K, H] the capsules before squash, caps [B, K, H] = squash(Z))."""
    _chk(routing_logits, torch.float32, "routing_logits")
    K, T = routing_logits.shape[-2:]
    if routing_logits.numel() != K * T or low.dim() != 2 or low.shape[0] % T:
        raise RecError("mind_routing_fwd: low must be [B * %d, H] and routing_logits [K, T], got %s and %s"
                       % (T, tuple(low.shape), tuple(routing_logits.shape)))
    B, H = low.shape[0] // T, low.shape[1]
    ld = _mtl_view(low, B * T, H, "low")
    _chk(seq_len, torch.int64, "seq_len", (B,))
    f32 = dict(dtype=torch.float32, device=low.device)
    W, Z, caps = torch.empty(B, K, T, **f32), torch.empty(B, K, H, **f32), torch.empty(B, K, H, **f32)
    check(lib().rec_mind_routing_fwd(B, T, K, H, int(iters), _p(low), ld, _p(seq_len), _p(routing_logits), _p(W), _p(Z),
                                     _p(caps), _stream()), "rec_mind_routing_fwd")
    return W, Z, caps


def mind_routing_bwd(d_caps, Z, W, out=None):
    """Backward of the routing's last product (rec_mind_routing_bwd): d_caps, Z [B, K, H] and W [B, K, T] contiguous ->
    d_low [B * T, H] (a view with a row stride when given).  W is a constant of the backward."""
    _chk(Z, torch.float32, "Z")
    B, K, H = Z.shape
    _chk(d_caps, torch.float32, "d_caps", (B, K, H))
    _chk(W, torch.float32, "W")
    T = W.shape[2]
    if tuple(W.shape) != (B, K, T):
        raise RecError("mind_routing_bwd: W must be [B, K, T], got %s" % (tuple(W.shape),))
    if out is None:
        out = torch.empty(B * T, H, dtype=torch.float32, device=Z.device)
    check(lib().rec_mind_routing_bwd(B, T, K, H, _p(d_caps), _p(Z), _p(W), _p(out), _mtl_view(out, B * T, H, "d_low"),
                                     _stream()), "rec_mind_routing_bwd")
    return out


def mind_label_attn_fwd(caps2, target, k_max, pow_p=1.0):
    """MIND's label-aware attention (rec_mind_label_attn_fwd): caps2 [B * K, H] and target [B, H], float32 views with a row
    stride.  attn = softmax_k(pow(<caps2_k, target>, pow_p)), user = sum_k attn_k caps2_k.  -> (user [B, H], attn [B, K])."""
    K = int(k_max)
    if caps2.dim() != 2 or caps2.shape[0] % max(K, 1):
        raise RecError("mind_label_attn_fwd: caps2 must be [B * k_max, H], got %s with k_max %d" % (tuple(caps2.shape), K))
    B, H = caps2.shape[0] // max(K, 1), caps2.shape[1]
    f32 = dict(dtype=torch.float32, device=caps2.device)
    user, attn = torch.empty(B, H, **f32), torch.empty(B, K, **f32)
    check(lib().rec_mind_label_attn_fwd(B, K, H, float(pow_p), _p(caps2), _mtl_view(caps2, B * K, H, "caps2"), _p(target),
                                        _mtl_view(target, B, H, "target"), _p(user), 0, _p(attn), _stream()),
          "rec_mind_label_attn_fwd")
    return user, attn


def mind_label_attn_bwd(caps2, target, attn, d_user, pow_p=1.0, d_target=None):
    """Backward of mind_label_attn_fwd (rec_mind_label_attn_bwd): d_user [B, H] -> (d_caps2 [B * K, H], d_target [B, H]: a
    view with a row stride when given)."""
    _chk(attn, torch.float32, "attn")
    B, K = attn.shape
    H = caps2.shape[1]
    f32 = dict(dtype=torch.float32, device=caps2.device)
    d_caps2 = torch.empty(B * K, H, **f32)
    if d_target is None:
        d_target = torch.empty(B, H, **f32)
    check(lib().rec_mind_label_attn_bwd(B, K, H, float(pow_p), _p(caps2), _mtl_view(caps2, B * K, H, "caps2"), _p(target),
                                        _mtl_view(target, B, H, "target"), _p(attn), _p(d_user),
                                        _mtl_view(d_user, B, H, "d_user"), _p(d_caps2), 0, _p(d_target),
                                        _mtl_view(d_target, B, H, "d_target"), _stream()),
          "rec_mind_label_attn_bwd")
    return d_caps2, d_target


def mind_ssm_head(user, true_w, true_b, S, sample_b, labels, neg, logq_true, logq_neg, grad_scale=1.0, d_true_w=None,
                  d_user0=None):
    """MIND's sampled-softmax head in one launch (rec_mind_ssm_head).  user, true_w [B, H] and S [B, n] (= user x sample_w^T)
    float32 views with a row stride; true_b, logq_true [B], sample_b, logq_neg [n] float32 and labels [B], neg [n] int64
    contiguous.  S is OVERWRITTEN with d(sample logits) = grad_scale * softmax (exactly 0 where labels[b] == neg[j]).
    d_true_w, d_user0: [B, H] views with a row stride (or None) that receive d_true * user and d_true * true_w.
    -> (loss [B] = -log_softmax of the true column, d_true [B], S)."""
    B, H = user.shape
    n = S.shape[1]
    ldu, ldt, lds = _mtl_view(user, B, H, "user"), _mtl_view(true_w, B, H, "true_w"), _mtl_view(S, B, n, "S")
    for t, name, shape in ((true_b, "true_b", (B,)), (logq_true, "logq_true", (B,)), (sample_b, "sample_b", (n,)),
                           (logq_neg, "logq_neg", (n,))):
        _chk(t, torch.float32, name, shape)
    _chk(labels, torch.int64, "labels", (B,))
    _chk(neg, torch.int64, "neg", (n,))
    loss = torch.empty(B, dtype=torch.float32, device=user.device)
    d_true = torch.empty(B, dtype=torch.float32, device=user.device)
    check(lib().rec_mind_ssm_head(B, H, n, _p(user), ldu, _p(true_w), ldt, _p(true_b), _p(S), lds, _p(sample_b), _p(labels),
                                  _p(neg), _p(logq_true), _p(logq_neg), float(grad_scale), _p(loss), _p(d_true), _p(d_true_w),
                                  _mtl_view(d_true_w, B, H, "d_true_w") if d_true_w is not None else 0, _p(d_user0),
                                  _mtl_view(d_user0, B, H, "d_user0") if d_user0 is not None else 0, _stream()),
          "rec_mind_ssm_head")
    return loss, d_true, S


# ------------------------------------------------------------------ word2vec: skip-gram with negative sampling
def _w2v_tables(emb, emb_w, emb_b, what):
    """The three tables of Word2VecLayer -> (V, D, ld_emb, ld_w, ld_b); emb_b is [V, 1] (or [V])."""
    D, ld_e = _chk_table(emb, "emb")
    Dw, ld_w = _chk_table(emb_w, "emb_w")
    Db, ld_b = _chk_table(emb_b, "emb_b")
    V = emb.shape[0]
    if emb.dim() != 2 or tuple(emb_w.shape) != (V, D) or emb_b.shape[0] != V or Db != 1:
        raise RecError("%s: expected emb, emb_w [V, D] and emb_b [V, 1], got %s, %s, %s"
                       % (what, tuple(emb.shape), tuple(emb_w.shape), tuple(emb_b.shape)))
    return V, D, ld_e, ld_w, ld_b


def w2v_sgns_fwd_bwd(in_ids, target_ids, emb, emb_w, emb_b, grad_scale=1.0, status=None, d_in=None):
    """Skip-gram with negative sampling, forward and the gradient of the logits in one launch (rec_w2v_sgns_fwd_bwd).
    in_ids [B] and target_ids [B, 1 + neg] (the true word first) int64 contiguous; emb, emb_w [V, D] and emb_b [V, 1] float32
    tables with a row stride.  d_in: a [B, D] view with a row stride (or None).
    -> (true_logits [B], neg_logits [B, neg], g [B, 1 + neg] = d loss / d logit, d_in [B, D], loss [1], status)."""
    V, D, ld_e, ld_w, ld_b = _w2v_tables(emb, emb_w, emb_b, "w2v_sgns_fwd_bwd")
    _chk(in_ids, torch.int64, "in_ids")
    B = in_ids.numel()
    _chk(target_ids, torch.int64, "target_ids")
    if in_ids.dim() != 1 or target_ids.dim() != 2 or target_ids.shape[0] != B or target_ids.shape[1] < 2:
        raise RecError("w2v_sgns_fwd_bwd: expected in_ids [B] and target_ids [B, 1 + neg], got %s and %s"
                       % (tuple(in_ids.shape), tuple(target_ids.shape)))
    neg = target_ids.shape[1] - 1
    dev = emb.device
    if status is None:
        status = new_status(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    if d_in is None:
        d_in = torch.empty(B, D, **f32)
    true_logits, neg_logits, g = torch.empty(B, **f32), torch.empty(B, neg, **f32), torch.empty(B, 1 + neg, **f32)
    loss = torch.zeros(1, **f32)
    check(lib().rec_w2v_sgns_fwd_bwd(B, D, neg, V, _p(in_ids), _p(target_ids), _p(emb), ld_e, _p(emb_w), ld_w, _p(emb_b), ld_b,
                                     float(grad_scale), _p(true_logits), _p(neg_logits), _p(g), _p(d_in),
                                     _mtl_view(d_in, B, D, "d_in"), _p(loss), _p(status), _stream()), "rec_w2v_sgns_fwd_bwd")
    return true_logits, neg_logits, g, d_in, loss, status


def w2v_target_update(groups, g, in_ids, emb, emb_w, emb_b, lr, d_w_rows=None, d_b_rows=None):
    """The SGD step of emb_w / emb_b from g and the PRE-update input table (rec_w2v_target_update): groups is
    ids_group(target_ids.reshape(-1)); the merged gradient of unique row u goes to d_w_rows [n, D] / d_b_rows [n] when given.
    The [B, 1 + neg, D] gradient is never written.  emb may not overlap emb_w."""
    V, D, ld_e, ld_w, ld_b = _w2v_tables(emb, emb_w, emb_b, "w2v_target_update")
    _chk(g, torch.float32, "g")
    _chk(in_ids, torch.int64, "in_ids")
    B = in_ids.numel()
    if g.dim() != 2 or g.shape[0] != B or g.numel() != groups.n:
        raise RecError("w2v_target_update: g %s does not match in_ids [%d] and a grouping of %d ids" % (tuple(g.shape), B, groups.n))
    neg = g.shape[1] - 1
    ld_dw = 0
    if d_w_rows is not None:
        ld_dw = _mtl_view(d_w_rows, groups.n, D, "d_w_rows")
    _chk(d_b_rows, torch.float32, "d_b_rows", (groups.n,))
    check(lib().rec_w2v_target_update(B, D, neg, V, _p(groups.n_uniq), _p(groups.uniq_rows), _p(groups.seg_offset),
                                      _p(groups.sorted_pos), _p(g), _p(in_ids), _p(emb), ld_e, _p(emb_w), ld_w, _p(emb_b), ld_b,
                                      float(lr), _p(d_w_rows), ld_dw, _p(d_b_rows), _stream()), "rec_w2v_target_update")


def w2v_analogy_topk(a, b, c, W, k=4, status=None, cand=None):
    """The analogy search of Word2VecInferLayer without the [Q, V] scores (rec_w2v_analogy_topk): a, b, c int64 [Q]; W [V, D]
    with a row stride; score = <W[b] - W[a] + W[c], W[v]> / max(|W[v]|, 1e-12).  cand: (values, ids) candidate buffers
    [tiles, Q, k] float32 / int64 to reuse (allocated when None or of another shape).
    -> (values [Q, k] descending, ids [Q, k] int64; equal scores by the lower id)."""
    D, ld = _chk_table(W, "W")
    if W.dim() != 2:
        raise RecError("w2v_analogy_topk: W must be [V, D]")
    V, k = W.shape[0], int(k)
    Q = a.numel()
    for t, name in ((a, "a"), (b, "b"), (c, "c")):
        _chk(t, torch.int64, name, (Q,))
    tiles = (V + _lib.REC_W2V_TOPK_TILE_ROWS - 1) // _lib.REC_W2V_TOPK_TILE_ROWS
    dev = W.device
    if cand is None or tuple(cand[0].shape) != (tiles, Q, k) or tuple(cand[1].shape) != (tiles, Q, k):
        cand = (torch.empty(tiles, Q, max(k, 0), dtype=torch.float32, device=dev),
                torch.empty(tiles, Q, max(k, 0), dtype=torch.int64, device=dev))
    _chk(cand[0], torch.float32, "cand values")
    _chk(cand[1], torch.int64, "cand ids")
    values = torch.empty(Q, max(k, 0), dtype=torch.float32, device=dev)
    ids = torch.empty(Q, max(k, 0), dtype=torch.int64, device=dev)
    check(lib().rec_w2v_analogy_topk(Q, D, ld, V, k, _p(a), _p(b), _p(c), _p(W), _p(cand[0]), _p(cand[1]), tiles, _p(values),
                                     _p(ids), _p(status), _stream()), "rec_w2v_analogy_topk")
    return values, ids


# ------------------------------------------------------------------ TiSASRec: time-interval-aware self-attention
TISAS_SITES = ("att", "pos_k", "pos_v", "time_k", "time_v")      # order of the streams argument of rec_tisas_attn_*


def _tisas_attn_args(q, k, v, tables, tm, log_seqs, H, probs, streams, what):
    ldq, ldk, ldv = _rows_view(q, "q"), _rows_view(k, "k"), _rows_view(v, "v")
    _chk(tm, torch.int64, "tm")
    _chk(log_seqs, torch.int64, "log_seqs")
    if log_seqs.dim() != 2 or tm.dim() != 3:
        raise RecError("%s: log_seqs must be [B, L] and tm [B, L, L]" % what)
    B, L = log_seqs.shape
    D = q.shape[1]
    if tuple(tm.shape) != (B, L, L) or q.shape[0] != B * L or k.shape != q.shape or v.shape != q.shape or len(tables) != 4:
        raise RecError("%s: q, k, v must be [B*L, D] and tm [B, L, L] (B %d, L %d; got %s, %s, %s, %s)"
                       % (what, B, L, tuple(q.shape), tuple(k.shape), tuple(v.shape), tuple(tm.shape)))
    pos_k, pos_v, time_k, time_v = tables
    T = time_k.shape[0]
    for t, n, sh in ((pos_k, "pos_k", (L, D)), (pos_v, "pos_v", (L, D)), (time_k, "time_k", (T, D)), (time_v, "time_v", (T, D))):
        _chk(t, torch.float32, n, sh)
    if len(probs) != 3 or len(streams) != 5:
        raise RecError("%s: probs is (attention, position, time) and streams one per TISAS_SITES" % what)
    tp = (C.c_void_p * 4)(*[t.data_ptr() for t in tables])
    pr = (C.c_float * 3)(*[float(x) for x in probs])
    st = (C.c_uint64 * 5)(*[int(x) for x in streams])
    return B, L, D, T, ldq, ldk, ldv, tp, pr, st


def tisas_attn_fwd(q, k, v, tables, tm, log_seqs, H, scale, probs=(0.0, 0.0, 0.0), seed=0, streams=(0, 0, 0, 0, 0),
                   status=None, out=None):
    """TiSASRec's attention without the [B, L, L, D] relation tensors (rec_tisas_attn_fwd).  q, k, v [B*L, D] views with a
    row stride; tables = (pos_k, pos_v [L, D], time_k, time_v [T, D]); tm int64 [B, L, L]; log_seqs int64 [B, L]; probs =
    dropout on (weights, position rows, time rows); streams: one mask stream per TISAS_SITES.
    -> (out [B*L, D], lse [B, H, L])."""
    B, L, D, T, ldq, ldk, ldv, tp, pr, st = _tisas_attn_args(q, k, v, tables, tm, log_seqs, H, probs, streams, "tisas_attn_fwd")
    if out is None:
        out = torch.empty(B * L, D, dtype=torch.float32, device=q.device)
    ldo = _rows_view(out, "out")
    if tuple(out.shape) != (B * L, D):
        raise RecError("tisas_attn_fwd: out must be [B*L, D]")
    lse = torch.empty(B, int(H), L, dtype=torch.float32, device=q.device)
    check(lib().rec_tisas_attn_fwd(B, L, int(H), D, T, _p(q), ldq, _p(k), ldk, _p(v), ldv, tp, _p(tm), _p(log_seqs),
                                   float(scale), pr, int(seed), st, _p(out), ldo, _p(lse), _p(status), _stream()),
          "rec_tisas_attn_fwd")
    return out, lse


def tisas_attn_bwd(q, k, v, tables, tm, log_seqs, H, scale, lse, d_out, d_tables, probs=(0.0, 0.0, 0.0), seed=0,
                   streams=(0, 0, 0, 0, 0), grads=None, accumulate=False, scratch=None):
    """Backward of tisas_attn_fwd (rec_tisas_attn_bwd).  d_tables: four tensors shaped like tables that receive (accumulate:
    are added) d_pos_k, d_pos_v, d_time_k, d_time_v.  grads: (dq, dk, dv) views to write or None.  scratch: a dict that
    keeps the call's buffers (gs, ga [B*H*L*L], partials) between calls.  -> (dq, dk, dv)."""
    B, L, D, T, ldq, ldk, ldv, tp, pr, st = _tisas_attn_args(q, k, v, tables, tm, log_seqs, H, probs, streams, "tisas_attn_bwd")
    H = int(H)
    _chk(lse, torch.float32, "lse", (B, H, L))
    f32 = dict(dtype=torch.float32, device=q.device)
    if grads is None:
        grads = tuple(torch.empty(B * L, D, **f32) for _ in range(3))
    dq, dk, dv = grads
    for t, n in ((d_out, "d_out"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _rows_view(t, n)
        if tuple(t.shape) != (B * L, D):
            raise RecError("tisas_attn_bwd: %s must be [B*L, D], got %s" % (n, tuple(t.shape)))
    if len(d_tables) != 4:
        raise RecError("tisas_attn_bwd: d_tables must hold four tensors")
    for t, src in zip(d_tables, tables):
        _chk(t, torch.float32, "d_tables", tuple(src.shape))
    P = min(B, _lib.REC_TISAS_MAX_PARTIALS)
    need = (B * H * L * L, B * H * L * L, P * 2 * T * D)
    scratch = scratch if scratch is not None else {}
    bufs = scratch.get("bufs")
    if bufs is None or tuple(b.numel() for b in bufs) != need or bufs[0].device != q.device:
        bufs = scratch["bufs"] = tuple(torch.empty(max(n, 1), **f32)[:n] for n in need)
    gs, ga, partials = bufs
    dp = (C.c_void_p * 4)(*[t.data_ptr() for t in d_tables])
    check(lib().rec_tisas_attn_bwd(B, L, H, D, T, _p(q), ldq, _p(k), ldk, _p(v), ldv, tp, _p(tm), _p(log_seqs), float(scale), pr,
                                   int(seed), st, _p(d_out), _view_ld(d_out), _p(lse), _p(gs), _p(ga), _p(dq), _view_ld(dq),
                                   _p(dk), _view_ld(dk), _p(dv), _view_ld(dv), dp, _p(partials), int(bool(accumulate)),
                                   _stream()), "rec_tisas_attn_bwd")
    return dq, dk, dv


def affine_layer_norm_fwd(x, gamma, beta, eps, r=None, row_ids=None, sum_out=None, out=None):
    """y = LN((x + r) * (row_ids != 0)) * gamma + beta over the last axis (rec_affine_layer_norm_fwd).  x, r [m, n] views with
    a row stride; row_ids int64 [m] or None; sum_out: a [m, n] view (may be x) that receives the masked sum, or None.
    -> (y, mean [m], rstd [m])."""
    ldx = _rows_view(x, "x")
    m, n = x.shape
    _chk(gamma, torch.float32, "gamma", (n,))
    _chk(beta, torch.float32, "beta", (n,))
    _chk(row_ids, torch.int64, "row_ids")
    if row_ids is not None and row_ids.numel() != m:
        raise RecError("affine_layer_norm_fwd: row_ids must hold one id per row")
    for t, name in ((r, "r"), (sum_out, "sum_out"), (out, "out")):
        if t is not None and (_rows_view(t, name) < 0 or tuple(t.shape) != (m, n)):
            raise RecError("affine_layer_norm_fwd: %s must have x's shape" % name)
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    mean = torch.empty(m, dtype=torch.float32, device=x.device)
    rstd = torch.empty(m, dtype=torch.float32, device=x.device)
    check(lib().rec_affine_layer_norm_fwd(m, n, _p(x), ldx, _p(r), _view_ld(r) if r is not None else 0, _p(gamma), _p(beta),
                                          float(eps), _p(row_ids), _p(sum_out), _view_ld(sum_out) if sum_out is not None else 0,
                                          _p(out), _view_ld(out), _p(mean), _p(rstd), _stream()), "rec_affine_layer_norm_fwd")
    return out, mean, rstd


def affine_layer_norm_bwd(t, mean, rstd, gamma, dy, dgamma, dbeta, dy2=None, e1=None, e2=None, row_ids=None, out=None):
    """Backward of affine_layer_norm_fwd (rec_affine_layer_norm_bwd): t is the masked sum the forward normalised; the
    incoming gradient is dy + dy2; e1, e2 are further gradients of t.  dgamma, dbeta [n] are written.
    -> dx [m, n], the gradient of x and of r (out may be dy)."""
    ldt = _rows_view(t, "t")
    m, n = t.shape
    for v_, name in ((mean, "mean"), (rstd, "rstd")):
        _chk(v_, torch.float32, name, (m,))
    for v_, name in ((gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _chk(v_, torch.float32, name, (n,))
    _chk(row_ids, torch.int64, "row_ids")
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=t.device)
    for v_, name in ((dy, "dy"), (dy2, "dy2"), (e1, "e1"), (e2, "e2"), (out, "out")):
        if v_ is not None and (_rows_view(v_, name) < 0 or tuple(v_.shape) != (m, n)):
            raise RecError("affine_layer_norm_bwd: %s must have t's shape" % name)
    ld = lambda v_: _view_ld(v_) if v_ is not None else 0
    check(lib().rec_affine_layer_norm_bwd(m, n, _p(t), ldt, _p(mean), _p(rstd), _p(gamma), _p(dy), ld(dy), _p(dy2), ld(dy2),
                                          _p(e1), ld(e1), _p(e2), ld(e2), _p(row_ids), _p(out), ld(out), _p(dgamma), _p(dbeta),
                                          _stream()), "rec_affine_layer_norm_bwd")
    return out


def tisas_embed_fwd(ids, table, scale, p=0.0, seed=0, stream=0, status=None, out=None):
    """out[r] = dropout(table[ids[r]] * scale), a zero row for id 0 (rec_tisas_embed_fwd).  ids int64 (any shape, contiguous);
    table [N, D] with a row stride.  -> out [ids.numel(), D]."""
    _chk(ids, torch.int64, "ids")
    D, ld = _chk_table(table, "table")
    n = ids.numel()
    if out is None:
        out = torch.empty(n, D, dtype=torch.float32, device=table.device)
    if tuple(out.shape) != (n, D):
        raise RecError("tisas_embed_fwd: out must be [n, D]")
    check(lib().rec_tisas_embed_fwd(n, D, table.shape[0], _p(ids), _p(table), ld, float(scale), float(p), int(seed), int(stream),
                                    _p(out), _rows_view(out, "out"), _p(status), _stream()), "rec_tisas_embed_fwd")
    return out


def tisas_embed_bwd(ids, d_out, num_rows, scale, p=0.0, seed=0, stream=0, out=None):
    """The gradient rows of the table behind tisas_embed_fwd (rec_tisas_embed_bwd): out[r] = d_out[r] * scale through the
    same mask, zero for id 0.  out: a [n, D] view with a row stride (rows of the step's gradient buffer) or None."""
    _chk(ids, torch.int64, "ids")
    ldd = _rows_view(d_out, "d_out")
    n, D = d_out.shape
    if ids.numel() != n:
        raise RecError("tisas_embed_bwd: one id per row of d_out")
    if out is None:
        out = torch.empty(n, D, dtype=torch.float32, device=d_out.device)
    if tuple(out.shape) != (n, D):
        raise RecError("tisas_embed_bwd: out must be [n, D]")
    check(lib().rec_tisas_embed_bwd(n, D, int(num_rows), _p(ids), _p(d_out), ldd, float(scale), float(p), int(seed), int(stream),
                                    _p(out), _rows_view(out, "out"), _stream()), "rec_tisas_embed_bwd")
    return out


def tisas_head(feats, pos, neg, table, status=None, d_pos_rows=None, d_neg_rows=None):
    """TiSASRec's training head (rec_tisas_head): both dot products per position, the two masked BCE means with the selected
    count taken on the device, d(feats) and the gradient rows of the pos / neg lookups.  feats [n, D] view; pos, neg int64
    [n]; table [N, D].  -> (loss2 [2] = loss, selected count; d_feats [n, D]; coef_pos [n]; coef_neg [n]; row_loss [n];
    pos_logits [n]; neg_logits [n])."""
    ldf = _rows_view(feats, "feats")
    n, D = feats.shape
    Dt, ldt = _chk_table(table, "table")
    _chk(pos, torch.int64, "pos")
    _chk(neg, torch.int64, "neg")
    if Dt != D or pos.numel() != n or neg.numel() != n:
        raise RecError("tisas_head: feats [n, D], pos / neg [n] and table [N, D] do not fit")
    f32 = dict(dtype=torch.float32, device=feats.device)
    loss2, row_loss = torch.empty(2, **f32), torch.empty(n, **f32)
    cp, cn, d_feats = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, D, **f32)
    pl, nl = torch.empty(n, **f32), torch.empty(n, **f32)
    for t, name in ((d_pos_rows, "d_pos_rows"), (d_neg_rows, "d_neg_rows")):
        if t is not None and (_rows_view(t, name) < 0 or tuple(t.shape) != (n, D)):
            raise RecError("tisas_head: %s must be [n, D]" % name)
    ld = lambda t: _view_ld(t) if t is not None else 0
    check(lib().rec_tisas_head(n, D, table.shape[0], _p(feats), ldf, _p(pos), _p(neg), _p(table), ldt, _p(loss2), _p(row_loss),
                               _p(pl), _p(nl), _p(cp), _p(cn), _p(d_feats), D, _p(d_pos_rows), ld(d_pos_rows), _p(d_neg_rows), ld(d_neg_rows),
                               _p(status), _stream()), "rec_tisas_head")
    return loss2, d_feats, cp, cn, row_loss, pl, nl


# ------------------------------------------------------------------ xDeepFM CIN (the passes around the GEMM)
def _chk_f32(t, name):
    if not t.is_cuda:
        raise RecError("%s must be a device tensor (no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise RecError("%s must be float32, got %s" % (name, t.dtype))


def cin_view(t, kind):
    """rec_cin_view of a feature tensor: kind "bfd" = [B,F,D] (feat_embeddings, any strides), "xt" = (tensor [B*D, C],
    D): a CIN layer's d-major GEMM output (row stride allowed, unit column stride)."""
    if kind == "bfd":
        _chk_f32(t, "feature tensor")
        return CinView(t.stride(0), t.stride(1), t.stride(2))
    x, D = t
    return CinView(D * _chk_mat(x, "XT"), 1, _chk_mat(x, "XT"))


def cin_outer_fwd(B, D, F, S, X0, v0, Xk, vk, Z):
    """Z[(b,d), f*S+s] = X0[b,f,d] * Xk[b,s,d]   (xdeepfm/net.py:163-175).  Z [B*D, F*S] f32."""
    _chk_f32(X0, "X0")
    _chk_f32(Xk, "Xk")
    ldz = _chk_mat(Z, "Z")
    if tuple(Z.shape) != (B * D, F * S):
        raise RecError("Z must be [B*D, F*S]")
    check(lib().rec_cin_outer_fwd(B, D, F, S, _p(X0), C.byref(v0), _p(Xk), C.byref(vk), _p(Z), ldz, _stream()),
          "rec_cin_outer_fwd")
    return Z


def cin_outer_bwd(B, D, F, S, dZ, X0, v0, Xk, vk, dX0, dv0, acc0, dXk, dvk, acck, dpool=None):
    """dX0 (+)= dZ . Xk over s;  dXk (+)= dZ . X0 over f (+ dpool[b,s] on every d row)."""
    for t, n in ((X0, "X0"), (Xk, "Xk"), (dX0, "dX0"), (dXk, "dXk")):
        _chk_f32(t, n)
    ldz = _chk_mat(dZ, "dZ")
    if tuple(dZ.shape) != (B * D, F * S):
        raise RecError("dZ must be [B*D, F*S]")
    ldp = 0
    if dpool is not None:
        ldp = _chk_mat(dpool, "dpool")
        if tuple(dpool.shape) != (B, S):
            raise RecError("dpool must be [B, S]")
    check(lib().rec_cin_outer_bwd(B, D, F, S, _p(dZ), ldz, _p(X0), C.byref(v0), _p(Xk), C.byref(vk), _p(dX0),
                                  C.byref(dv0), int(acc0), _p(dXk), C.byref(dvk), int(acck), _p(dpool), ldp, _stream()),
          "rec_cin_outer_bwd")


def cin_contract_fwd(B, D, F, Y, X0, v0, XT):
    """XT[(b,d), c] = sum_f X0[b,f,d] * Y[(b,d), c*F+f]   (the C < S association of a CIN layer)."""
    _chk_f32(X0, "X0")
    ldy, ldx = _chk_mat(Y, "Y"), _chk_mat(XT, "XT")
    Cc = XT.shape[1]
    if tuple(Y.shape) != (B * D, Cc * F) or XT.shape[0] != B * D:
        raise RecError("Y must be [B*D, C*F] and XT [B*D, C]")
    check(lib().rec_cin_contract_fwd(B, D, F, Cc, _p(Y), ldy, _p(X0), C.byref(v0), _p(XT), ldx, _stream()),
          "rec_cin_contract_fwd")
    return XT


def cin_contract_bwd(B, D, F, Y, dXT, X0, v0, dY, dX0, dv0, acc0):
    """dY = dXT (x) X0;  dX0 (+)= sum_c dXT[.,c] * Y[., c*F+f]."""
    for t, n in ((X0, "X0"), (dX0, "dX0")):
        _chk_f32(t, n)
    ldy, ldx, lddy = _chk_mat(Y, "Y"), _chk_mat(dXT, "dXT"), _chk_mat(dY, "dY")
    Cc = dXT.shape[1]
    if tuple(Y.shape) != (B * D, Cc * F) or tuple(dY.shape) != (B * D, Cc * F) or dXT.shape[0] != B * D:
        raise RecError("Y / dY must be [B*D, C*F] and dXT [B*D, C]")
    check(lib().rec_cin_contract_bwd(B, D, F, Cc, _p(Y), ldy, _p(dXT), ldx, _p(X0), C.byref(v0), _p(dY), lddy,
                                     _p(dX0), C.byref(dv0), int(acc0), _stream()), "rec_cin_contract_bwd")


def cin_sumpool(B, D, XT, out):
    """out[b,c] = sum_d XT[(b,d), c]   (net.py:195-198); out may be a column window of the pooled-feature row."""
    ldx, ldo = _chk_mat(XT, "XT"), _chk_mat(out, "out")
    Cc = XT.shape[1]
    if XT.shape[0] != B * D or tuple(out.shape) != (B, Cc):
        raise RecError("XT must be [B*D, C] and out [B, C]")
    check(lib().rec_cin_sumpool(B, D, Cc, _p(XT), ldx, _p(out), ldo, _stream()), "rec_cin_sumpool")
    return out


def cin_sumpool_bwd(B, D, dpool, dXT):
    """dXT[(b,d), c] = dpool[b,c]."""
    ldp, ldx = _chk_mat(dpool, "dpool"), _chk_mat(dXT, "dXT")
    Cc = dpool.shape[1]
    if tuple(dXT.shape) != (B * D, Cc) or dpool.shape[0] != B:
        raise RecError("dXT must be [B*D, C] and dpool [B, C]")
    check(lib().rec_cin_sumpool_bwd(B, D, Cc, _p(dpool), ldp, _p(dXT), ldx, _stream()), "rec_cin_sumpool_bwd")
    return dXT


# ------------------------------------------------------------------ DLRM: BatchNorm1D, dot interaction, accuracy
def batchnorm_fwd(X, gamma, beta, running_mean, running_var, ws, training=True, momentum=0.9, eps=1e-5, out=None):
    """nn.BatchNorm1D on X [m, n] (dlrm/net.py:151-153).  -> (Y, save_mean [n], save_invstd [n]); the running
    statistics are updated in place when training."""
    ldx = _chk_mat(X, "X")
    m, n = X.shape
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, torch.float32, nm, (n,))
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=X.device)
    ldy = _chk_mat(out, "out")
    sm = torch.empty(n, dtype=torch.float32, device=X.device)
    si = torch.empty(n, dtype=torch.float32, device=X.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_batchnorm_workspace_bytes(m, n, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_batchnorm_fwd(m, n, _p(X), ldx, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                  float(momentum), float(eps), int(bool(training)), _p(out), ldy, _p(sm), _p(si), _p(w),
                                  C.c_size_t(w.numel()), _stream()), "rec_batchnorm_fwd")
    return out, sm, si


def batchnorm_bwd(X, dY, gamma, save_mean, save_invstd, ws, relu_mask=False, dgamma=None, dbeta=None, out=None):
    """-> (dX, dgamma, dbeta).  relu_mask: X was a ReLU output — dX is zeroed where X <= 0."""
    ldx, lddy = _chk_mat(X, "X"), _chk_mat(dY, "dY")
    m, n = X.shape
    dev = X.device
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=dev)
    if dgamma is None:
        dgamma = torch.empty(n, dtype=torch.float32, device=dev)
    if dbeta is None:
        dbeta = torch.empty(n, dtype=torch.float32, device=dev)
    for t, nm in ((gamma, "gamma"), (save_mean, "save_mean"), (save_invstd, "save_invstd"), (dgamma, "dgamma"),
                  (dbeta, "dbeta")):
        _chk(t, torch.float32, nm, (n,))
    nbytes = C.c_size_t(0)
    check(lib().rec_batchnorm_workspace_bytes(m, n, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_batchnorm_bwd(m, n, _p(X), ldx, _p(dY), lddy, _p(gamma), _p(save_mean), _p(save_invstd),
                                  int(bool(relu_mask)), _p(out), _chk_mat(out, "dX"), _p(dgamma), _p(dbeta), _p(w),
                                  C.c_size_t(w.numel()), _stream()), "rec_batchnorm_bwd")
    return out, dgamma, dbeta


def dot_interact_fwd(T, out=None):
    """T [B,F,D] = [emb_1 .. emb_{F-1}, x]  ->  R [B, D + F(F-1)/2] = [x | strictly-upper-triangle dots, row-major]
    (dlrm/net.py:96-123)."""
    _chk(T, torch.float32, "T")
    B, F, D = T.shape
    P = F * (F - 1) // 2
    if out is None:
        out = torch.empty(B, D + P, dtype=torch.float32, device=T.device)
    check(lib().rec_dot_interact_fwd(B, F, D, _p(T), F * D, _p(out), _chk_mat(out, "R"), _stream()),
          "rec_dot_interact_fwd")
    return out


def dot_interact_bwd(T, dR, out=None):
    _chk(T, torch.float32, "T")
    B, F, D = T.shape
    ldr = _chk_mat(dR, "dR")
    if out is None:
        out = torch.empty(B, F, D, dtype=torch.float32, device=T.device)
    _chk(out, torch.float32, "dT", (B, F, D))
    check(lib().rec_dot_interact_bwd(B, F, D, _p(T), F * D, _p(dR), ldr, _p(out), F * D, _stream()),
          "rec_dot_interact_bwd")
    return out


def accuracy_count(pred, label, counts):
    """counts [2] int64: += (#correct top-1 of two classes, n)   (paddle.metric.Accuracy)."""
    _chk(pred, torch.float32, "pred")
    _chk(label, torch.int64, "label")
    _chk(counts, torch.int64, "counts", (2,))
    check(lib().rec_accuracy_count(pred.numel(), _p(pred), _p(label), _p(counts), _stream()), "rec_accuracy_count")
    return counts


def sparse_sgd_rows(groups, grad, P, lr, grad_div=1, grad_group=0, grad_group_stride=0, partials=None):
    D, stride = _chk_table(P, "P")
    check(lib().rec_sparse_sgd_rows(groups.n, D, stride, _p(groups.n_uniq), _p(groups.uniq_rows),
                                    _p(groups.seg_offset), _p(groups.sorted_pos), _p(grad),
                                    C.byref(_gl(grad_div, grad_group, grad_group_stride, partials)),
                                    _p(P), float(lr), _stream()), "rec_sparse_sgd_rows")


SMALL_MERGE_MAX = 15360     # rec_sparse_sgd_small: lookups per call


def sparse_sgd_small(ids, grad, P, lr, padding_idx=None, status=None, grad_div=1, grad_group=0, grad_group_stride=0):
    """Merge + SGD row update of a small SelectedRows gradient in ONE launch (ids.numel() <= SMALL_MERGE_MAX,
    emb_dim <= 256): P[row] -= lr * (sum of the row's gradient rows, ascending position)."""
    _chk(ids, torch.int64, "ids")
    D, stride = _chk_table(P, "P")
    if status is None:
        status = new_status(ids.device)
    check(lib().rec_sparse_sgd_small(ids.numel(), D, stride, P.shape[0], -1 if padding_idx is None else padding_idx,
                                     _p(ids), _p(grad), C.byref(_gl(grad_div, grad_group, grad_group_stride)), _p(P),
                                     float(lr), _p(status), _stream()), "rec_sparse_sgd_small")
    return status


def sparse_sgd_small_multi(jobs, lr, status):
    """Up to 8 sparse_sgd_small jobs in ONE launch: jobs = [(ids, grad, P, grad_group, grad_group_stride), ...] (tables
    independent of each other: rec_sparse_sgd_small_multi)."""
    arr = (_lib.SmallSgdJob * len(jobs))()
    for a, (ids, grad, P, group, gstride) in zip(arr, jobs):
        _chk(ids, torch.int64, "ids")
        D, stride = _chk_table(P, "P")
        a.n, a.emb_dim, a.row_stride, a.num_rows, a.padding_idx = ids.numel(), D, stride, P.shape[0], -1
        a.ids, a.grad, a.P = ids.data_ptr(), grad.data_ptr(), P.data_ptr()
        a.grad_layout = _gl(1, group, gstride)
        if _recorder is not None:
            _recorder.note_field(a, "ids", ids)
            _recorder.keep.extend((ids, grad, P))
    check(lib().rec_sparse_sgd_small_multi(len(jobs), arr, float(lr), _p(status), _stream()),
          "rec_sparse_sgd_small_multi")
    return status


_SMALL_SCRATCH = {}


def sparse_adam_record_small(ids, slot_offset, padding_idx, grad, grad1, grad1_div, rec, mv, D, step, lr=1e-3,
                             beta1=0.9, beta2=0.999, eps=1e-8, v_offset=None, grad_scale=None, status=None):
    """sparse_adam_record with the SelectedRows merge done inside the launch (ids.numel() <= SMALL_MERGE_MAX): ids
    [B,S] (or flat [B*S]), row = id + slot_offset[s]; grad [B*S, D] row gradients; grad1 = dz with layout {grad1_div}."""
    _chk(ids, torch.int64, "ids")
    _chk(grad, torch.float32, "grad")
    _chk(grad1, torch.float32, "grad1")
    S = ids.shape[-1] if ids.dim() > 1 else 1
    if v_offset is None:
        v_offset = (D + 3) // 4 * 4
    if status is None:
        status = new_status(ids.device)
    h = _hyper(lr, beta1, beta2, eps, step)
    # one int per (device, stream): the launch's "every id stays in its slot's span" decision — written by one kernel
    # of the call and read by the next on the SAME stream, so calls on different streams must not share it
    key = (ids.device, _stream().value if ids.device.type == "cuda" else None)
    scratch = _SMALL_SCRATCH.get(key)
    if scratch is None:
        if len(_SMALL_SCRATCH) > 256:
            _SMALL_SCRATCH.clear()
        scratch = _SMALL_SCRATCH[key] = torch.zeros(1, dtype=torch.int32, device=ids.device)
    check(lib().rec_sparse_adam_record_small(ids.numel(), S, int(D), rec.stride(0), mv.stride(0), int(v_offset),
                                             rec.shape[0], -1 if padding_idx is None else int(padding_idx), _p(ids),
                                             _p(slot_offset), _p(grad), C.byref(_gl(1, 0, 0)), _p(grad1),
                                             C.byref(_gl(grad1_div, 0, 0)), _p(grad_scale), _p(rec), _p(mv),
                                             C.byref(h), _p(status), _p(scratch), _stream()),
          "rec_sparse_adam_record_small")
    return status


def sgd_dense(p, g, lr):
    _chk(p, torch.float32, "p")
    _chk(g, torch.float32, "g")
    if g.numel() != p.numel():
        raise RecError("sgd_dense: %d gradients for %d parameters" % (g.numel(), p.numel()))
    check(lib().rec_sgd_dense(p.numel(), _p(p), _p(g), float(lr), _stream()), "rec_sgd_dense")


def bce_with_logits(logit, label, ws, mean_over=0):
    """-> pred [B,1], dz [B,1], loss [1]   (label float32 [B,1])"""
    B = logit.numel()
    _chk(logit, torch.float32, "logit")
    _chk(label, torch.float32, "label")
    if label.numel() != B:
        raise RecError("bce_with_logits: %d labels for %d logits" % (label.numel(), B))
    dev = logit.device
    pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
    dz = torch.empty(B, 1, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    nbytes = C.c_size_t(0)
    check(lib().rec_logloss_workspace_bytes(B, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_bce_with_logits(B, int(mean_over), _p(logit), _p(label), _p(pred), _p(dz), _p(loss), _p(w),
                                    C.c_size_t(w.numel()), _stream()), "rec_bce_with_logits")
    return pred, dz, loss


def softmax_rows(x, out=None):
    ldx = _chk_mat(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().rec_softmax_rows(x.shape[0], x.shape[1], _p(x), ldx, _p(out), _chk_mat(out, "out"),
                                 _stream()), "rec_softmax_rows")
    return out


def moe_bwd_prep(dX, X0, U, prob_e, dU, dX0_acc, accumulate, dp_e):
    """CrossNetMix backward glue for one expert: dU = dX*X0*p_e; dX0_acc (+)= dX*p_e*U; dp_e = rowsum(dX*X0*U)."""
    M, N = dX.shape
    lds = [_chk_mat(t, n) for t, n in ((dX, "dX"), (X0, "X0"), (U, "U"), (dU, "dU"), (dX0_acc, "dX0_acc"))]
    check(lib().rec_moe_bwd_prep(M, N, _p(dX), lds[0], _p(X0), lds[1], _p(U), lds[2], _p(prob_e),
                                 prob_e.stride(0) if M > 1 else 1, _p(dU), lds[3], _p(dX0_acc), lds[4],
                                 int(accumulate), _p(dp_e), dp_e.stride(0) if M > 1 else 1, _stream()),
          "rec_moe_bwd_prep")


def softmax_rows_bwd(p, dp, out=None):
    if out is None:
        out = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    check(lib().rec_softmax_rows_bwd(p.shape[0], p.shape[1], _p(p), _chk_mat(p, "p"), _p(dp), _chk_mat(dp, "dp"),
                                     _p(out), _chk_mat(out, "out"), _stream()), "rec_softmax_rows_bwd")
    return out


def cross_bwd_prep(dX, X0, U, dU, dX0_acc, accumulate):
    """dU = dX*X0; dX0_acc (+)= dX*U  (CrossNetV2 backward glue)."""
    M, N = dX.shape
    lds = [_chk_mat(t, n) for t, n in ((dX, "dX"), (X0, "X0"), (U, "U"), (dU, "dU"), (dX0_acc, "dX0_acc"))]
    check(lib().rec_cross_bwd_prep(M, N, _p(dX), lds[0], _p(X0), lds[1], _p(U), lds[2], _p(dU), lds[3],
                                   _p(dX0_acc), lds[4], int(accumulate), _stream()), "rec_cross_bwd_prep")


# ------------------------------------------------------------------ CrossNet layers (one C-ABI call per layer)
def _ld(t, name):
    return _chk_mat(t, name)


def crossnet_v2_layer_fwd(x0, xl, W, bias, ws, out=None, u=None):
    """x_{l+1} = x_l + x_0 * (x_l W + b) (dcn_v2/net.py:222-226) -> out; u (optional) receives x_l W + b."""
    B, d = xl.shape
    if out is None:
        out = torch.empty(B, d, dtype=torch.float32, device=xl.device)
    desc = _lib.CrossV2Desc(B, d, _ld(x0, "x0"), _ld(xl, "xl"), _ld(out, "out"), _ld(u, "u") if u is not None else d)
    nb = C.c_size_t(0)
    check(lib().rec_crossnet_v2_layer_workspace_bytes(C.byref(desc), C.byref(nb), None))
    w = ws.get(nb.value)
    check(lib().rec_crossnet_v2_layer_fwd(C.byref(desc), _p(x0), _p(xl), _p(W), _p(bias), _p(out), _p(u), _p(w),
                                          C.c_size_t(w.numel()), _stream()), "rec_crossnet_v2_layer_fwd")
    return out


def crossnet_v2_layer_bwd(x0, xl, W, u, dxnext, dx0_acc, accumulate_dx0, fold_dx0, dW, db, ws, out=None):
    """-> d x_l ([B,d]); dW, db written; dx0_acc (+)= dxnext * u."""
    B, d = xl.shape
    if out is None:
        out = torch.empty(B, d, dtype=torch.float32, device=xl.device)
    # ld_out: the widest gradient row stride of this call, so that the workspace query covers the split-K partials of
    # the GEMM that writes `out` (include/recengine.h: the backward reads ld_out for nothing else)
    desc = _lib.CrossV2Desc(B, d, _ld(x0, "x0"), _ld(xl, "xl"),
                            max(d, _ld(dxnext, "dxnext"), _ld(dx0_acc, "dx0_acc"), _ld(out, "out")), _ld(u, "u"))
    nb = C.c_size_t(0)
    check(lib().rec_crossnet_v2_layer_workspace_bytes(C.byref(desc), None, C.byref(nb)))
    w = ws.get(nb.value)
    check(lib().rec_crossnet_v2_layer_bwd(C.byref(desc), _p(x0), _p(xl), _p(W), _p(u), _p(dxnext), _ld(dxnext, "dxnext"),
                                          _p(dx0_acc), _ld(dx0_acc, "dx0_acc"), int(accumulate_dx0), int(fold_dx0),
                                          _p(out), _ld(out, "out"), _p(dW), _p(db), _p(w), C.c_size_t(w.numel()),
                                          _stream()), "rec_crossnet_v2_layer_bwd")
    return out


def crossnet_mix_layer_fwd(x0, xl, U, V, Cm, bias, gate_w, gate_b, ws, out=None):
    """One CrossNetMix layer (dcn_v2/net.py:278-320) -> (x_next, t1, t2, prob); t1 / t2 / prob are what the backward
    needs."""
    B, d = xl.shape
    E, _, r = U.shape
    dev = xl.device
    if out is None:
        out = torch.empty(B, d, dtype=torch.float32, device=dev)
    t1 = torch.empty(B, E * r, dtype=torch.float32, device=dev)
    t2 = torch.empty(B, E * r, dtype=torch.float32, device=dev)
    prob = torch.empty(B, E, dtype=torch.float32, device=dev)
    desc = _lib.CrossMixDesc(B, d, r, E, _ld(x0, "x0"), _ld(xl, "xl"), _ld(out, "out"))
    nb = C.c_size_t(0)
    check(lib().rec_crossnet_mix_layer_workspace_bytes(C.byref(desc), C.byref(nb), None))
    w = ws.get(nb.value)
    check(lib().rec_crossnet_mix_layer_fwd(C.byref(desc), _p(x0), _p(xl), _p(U), _p(V), _p(Cm), _p(bias), _p(gate_w),
                                           _p(gate_b), _p(out), _p(t1), _p(t2), _p(prob), _p(w),
                                           C.c_size_t(w.numel()), _stream()), "rec_crossnet_mix_layer_fwd")
    return out, t1, t2, prob


def crossnet_mix_layer_bwd(x0, xl, U, V, Cm, bias, gate_w, t1, t2, prob, dxnext, dx0_acc, accumulate_dx0, fold_dx0,
                           gU, gV, gC, gbias, g_gate_w, g_gate_b, accumulate_gate, ws, out=None):
    """-> d x_l; gU / gV / gC / gbias written, the shared gating gradients written or accumulated."""
    B, d = xl.shape
    E, _, r = U.shape
    if out is None:
        out = torch.empty(B, d, dtype=torch.float32, device=xl.device)
    desc = _lib.CrossMixDesc(B, d, r, E, _ld(x0, "x0"), _ld(xl, "xl"),          # ld_out: as crossnet_v2_layer_bwd
                             max(d, _ld(dxnext, "dxnext"), _ld(dx0_acc, "dx0_acc"), _ld(out, "out")))
    nb = C.c_size_t(0)
    check(lib().rec_crossnet_mix_layer_workspace_bytes(C.byref(desc), None, C.byref(nb)))
    w = ws.get(nb.value)
    check(lib().rec_crossnet_mix_layer_bwd(C.byref(desc), _p(x0), _p(xl), _p(U), _p(V), _p(Cm), _p(bias), _p(gate_w),
                                           _p(t1), _p(t2), _p(prob), _p(dxnext), _ld(dxnext, "dxnext"), _p(dx0_acc),
                                           _ld(dx0_acc, "dx0_acc"), int(accumulate_dx0), int(fold_dx0), _p(out),
                                           _ld(out, "out"), _p(gU), _p(gV), _p(gC), _p(gbias), _p(g_gate_w),
                                           _p(g_gate_b), int(accumulate_gate), _p(w), C.c_size_t(w.numel()),
                                           _stream()), "rec_crossnet_mix_layer_bwd")
    return out


# ------------------------------------------------------------------ row-sharded tables
class ShardRoute:
    """Result buffers of rec_shard_route (device)."""

    def __init__(self, n, num_shards, device):
        self.n, self.num_shards = n, num_shards
        i64 = dict(dtype=torch.int64, device=device)
        self.send_local_row = torch.empty(max(n, 1), **i64)
        self.send_pos = torch.empty(max(n, 1), **i64)
        self.send_sample = torch.empty(max(n, 1), **i64)
        self.slot_of_pos = torch.empty(max(n, 1), **i64)
        self.send_counts = torch.zeros(num_shards + 1, **i64)


class DedupPlan:
    """One deduplicated lookup of a row-sharded table (paddlerec_amd/sharded.py, REC_SHARD_DEDUP): the DISTINCT rows this
    rank needs of every owner, in fixed-capacity send slots (owner o owns slots [o * cap, (o + 1) * cap)), and the maps
    between lookup positions, distinct rows and slots.  Everything lives on the device; nothing here reads it back."""

    def __init__(self, n, num_shards, cap, device):
        self.n, self.num_shards, self.cap = n, num_shards, cap
        self.groups = IdGroups(n, device)                  # grouping of the lookups by (owner, local row)
        i64 = dict(dtype=torch.int64, device=device)
        self.send_rows = torch.empty(num_shards * cap, **i64)       # local row per slot; empty slots hold `sentinel`
        self.slot_of_pos = torch.empty(max(n, 1), **i64)            # 1 + slot of the position's row; 0: padding / dropped
        self.slot_of_uniq = torch.empty(max(n, 1), **i64)           # slot of distinct row u; num_shards * cap: none
        self.counts = torch.zeros(num_shards, **i64)                # distinct rows per owner (before the capacity cut)
        self.sentinel = None


def dedup_plan(ids, num_rows, padding_idx, num_shards, local_rows, cap, ws, slot_offset=None, status=None, plan=None):
    """Distinct (owner, local row) pairs of a batch of lookups, owner-major and ascending — HeterPS dedups a pass's keys
    before it builds the per-GPU tables (tools/static_gpubox_trainer.py:237-246).  ids [B,S] int64; row = id +
    slot_offset[s]; owner = row % num_shards, local row = row // num_shards.  rec_dedup_plan: device only, no host read:
    sizes are the fixed capacity `cap` rows per owner; a rank that needs more of one owner sets REC_FLAG_EXCHANGE_OVERFLOW
    and loses the rows behind the capacity."""
    _chk(ids, torch.int64, "ids")
    n, G, dev = ids.numel(), int(num_shards), ids.device
    if plan is None or plan.n != n or plan.cap != cap or plan.num_shards != G:
        plan = DedupPlan(n, G, cap, dev)
    if status is None:
        status = new_status(dev)
    S = ids.shape[-1] if ids.dim() > 1 else 1
    nbytes = C.c_size_t(0)
    check(lib().rec_dedup_plan_workspace_bytes(n, G, int(local_rows), C.byref(nbytes)), "rec_dedup_plan_workspace_bytes")
    w = ws.get(nbytes.value)
    g = plan.groups
    plan.sentinel = int(local_rows)
    check(lib().rec_dedup_plan(n, S, int(num_rows), -1 if padding_idx is None else int(padding_idx), G, int(local_rows),
                               int(cap), _p(ids), _p(slot_offset), _p(g.sorted_pos), _p(g.uniq_rows), _p(g.seg_offset),
                               _p(g.n_uniq), _p(plan.send_rows), _p(plan.slot_of_pos), _p(plan.slot_of_uniq),
                               _p(plan.counts), _p(status), _p(w), C.c_size_t(w.numel()), _stream()), "rec_dedup_plan")
    return plan, status


def dedup_merge(plan, grad, emb_dim, grad_div=1, out=None):
    """The gradient rows of a deduplicated lookup merged per distinct row (duplicates summed in ascending position
    order, as every merge of the engine) and laid into the plan's send slots: out [num_shards * cap, emb_dim], zeros in
    the empty slots.  grad: [n / grad_div, emb_dim] (grad_div = S: one row per sample serving its S lookups)."""
    G, cap, D = plan.num_shards, plan.cap, int(emb_dim)
    none = G * cap
    if out is None or out.shape[0] != none + 1:
        out = torch.empty(none + 1, D, dtype=torch.float32, device=grad.device)      # + one row the unplaced rows land in
    out.zero_()

    class _G:                                   # the plan's grouping with the send slot in the place of the table row
        pass
    g, f = plan.groups, _G()
    f.n, f.n_uniq, f.seg_offset, f.sorted_pos, f.uniq_rows = g.n, g.n_uniq, g.seg_offset, g.sorted_pos, plan.slot_of_uniq
    sparse_sgd_rows(f, grad, out, -1.0, grad_div=grad_div)          # 0 - (-1) * sum = sum, exactly
    return out


def shard_route(ids, num_rows, padding_idx, num_shards, ws, slot_offset=None, status=None,
                route=None):
    """Partition the lookups by owner shard (row % num_shards).  -> (ShardRoute, status)"""
    _chk(ids, torch.int64, "ids")
    n = ids.numel()
    S = ids.shape[-1] if ids.dim() > 1 else 1
    dev = ids.device
    if route is None:
        route = ShardRoute(n, num_shards, dev)
    if status is None:
        status = new_status(dev)
    nbytes = C.c_size_t(0)
    check(lib().rec_shard_route_workspace_bytes(n, num_shards, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_shard_route(n, S, num_rows, -1 if padding_idx is None else padding_idx,
                                num_shards, _p(ids), _p(slot_offset), _p(route.send_local_row),
                                _p(route.send_pos), _p(route.send_sample), _p(route.slot_of_pos),
                                _p(route.send_counts), _p(status), _p(w), C.c_size_t(w.numel()),
                                _stream()), "rec_shard_route")
    return route, status


# ------------------------------------------------------------------ f32 MFMA GEMM
def _chk_mat(t, name):
    if not t.is_cuda:
        raise RecError("%s must be a device tensor (no CPU fallback)" % name)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise RecError("%s must be a 2-D float32 tensor" % name)
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise RecError("%s must have unit column stride" % name)
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


_gemm_ws_cache = {}


class GemmImages:
    """bf16 x 3 images of a set of GEMM weights, made in ONE launch (rec_gemm_b_images) ahead of the GEMMs that consume
    them: entries (B, trans_b) in the orientation the consuming call passes.  get(i) -> the image tensor (or None where
    the shape has no image form: the call then splits for itself, or runs the exact-f32 kernel)."""

    def __init__(self, specs, device):
        self.specs, self.images = list(specs), []
        for B, trans_b in self.specs:
            n, k = (B.shape if trans_b else B.shape[::-1])
            ok, nb = C.c_int32(0), C.c_size_t(0)
            check(lib().rec_gemm_b_image_bytes(int(k), int(n), C.byref(ok), C.byref(nb)), "rec_gemm_b_image_bytes")
            self.images.append(torch.empty(nb.value, dtype=torch.uint8, device=device) if ok.value else None)
        live = [(B, t, img) for (B, t), img in zip(self.specs, self.images) if img is not None]
        self._items = (GemmBImage * max(1, len(live)))()
        self._n = len(live)
        for it, (B, t, img) in zip(self._items, live):
            n, k = (B.shape if t else B.shape[::-1])
            it.B, it.ldb, it.k, it.n, it.trans_b, it.image = B.data_ptr(), _chk_mat(B, "B"), int(k), int(n), int(t), img.data_ptr()

    def refresh(self):
        """Re-split every weight from its current values on the current stream."""
        if self._n:
            check(lib().rec_gemm_b_images(self._n, self._items, _stream()), "rec_gemm_b_images")

    def get(self, i):
        return self.images[i]


def gemm(A, B, ws, trans_a=False, trans_b=False, epilogue="none", bias=None, aux0=None, aux1=None,
         out=None, split_k=0, b_colsum=None, row_scale=None, out2=None, num_cus=0, b_image=None, relu_bits=None):
    """out[M,N] = epi(op(A) @ op(B)); A/B/out row-major (row strides allowed).
    trans_a: A is given as [K,M]; trans_b: B is given as [N,K] (a torch Linear.weight, or W for dX).
    num_cus > 0: the current stream is confined to that many compute units (cu_range_stream) — size the
    split-K for them instead of the whole chip.
    b_image: op(B)'s bf16 x 3 image from GemmImages (current values of B): the call skips its own split launch.
    relu_bits: the ReLU mask as bits (rec_gemm_epilogue_args.relu_bits).  epilogue "bias_relu": a LIST — the call appends
    the mask tensor it wrote beside `out` (or None when this call has no bit form); "relu_mask": such a tensor (or None):
    read instead of aux0 when this call has the bit form."""
    d, x, out, need = _gemm_prepare(A, B, trans_a, trans_b, epilogue, bias, aux0, aux1, out, split_k, b_colsum, row_scale,
                                    out2, num_cus, b_image)
    if relu_bits is not None:
        nb = _relu_bits_bytes(d)
        if epilogue == "bias_relu":
            t = torch.empty(nb // 8, dtype=torch.int64, device=A.device) if nb else None
            relu_bits.append(t)
            relu_bits = t
        elif nb == 0 or relu_bits.numel() * 8 < nb:
            relu_bits = None
        if relu_bits is not None:
            x.relu_bits = relu_bits.data_ptr()
            if _recorder is not None:
                _recorder.keep.append(relu_bits)
    w = ws.get(need)
    check(lib().rec_gemm_f32(C.byref(d), _p(A), _p(B), _p(out), C.byref(x), _p(w),
                             C.c_size_t(w.numel()), _stream()), "rec_gemm_f32")
    return out


def linear_backward(X, G, W, ws, dW, db, relu_src=None, b_image=None, epilogue=None, aux0=None, relu_bits=None, out=None):
    """The backward of one Linear in ONE call (rec_gemm_f32_pair): dW = X^T G, db = colsum(G) and
    dX = G W^T (masked by relu_src > 0 — the layer's own input — when given; or any dX epilogue of gemm(): epilogue=
    "dsigmoid", aux0=the layer's input).  -> dX.  At launch-bound sizes the two GEMMs are one launch; otherwise exactly the
    two gemm() calls of mlp_backward, dW first.  out: the buffer (view) dX is written to."""
    if epilogue is None:
        epilogue, aux0 = ("relu_mask", relu_src) if relu_src is not None else ("none", None)
    d0, x0, _, need0 = _gemm_prepare(X, G, True, False, "none", None, None, None, dW, 0, db, None, None, 0, None)
    d1, x1, dX, need1 = _gemm_prepare(G, W, False, True, epilogue, None, aux0, None, out, 0, None, None, None, 0, b_image)
    if relu_bits is not None and epilogue == "relu_mask":      # relu_src's mask as bits (mlp_forward), where dX has the bit form
        nb = _relu_bits_bytes(d1)
        if nb and relu_bits.numel() * 8 >= nb:
            x1.relu_bits = relu_bits.data_ptr()
            if _recorder is not None:
                _recorder.keep.append(relu_bits)
    w = ws.get(max(need0, need1))
    check(lib().rec_gemm_f32_pair(C.byref(d0), _p(X), _p(G), _p(dW), C.byref(x0), C.byref(d1), _p(G), _p(W), _p(dX),
                                  C.byref(x1), _p(w), C.c_size_t(w.numel()), _stream()), "rec_gemm_f32_pair")
    return dX


GemmRouteInfo = collections.namedtuple("GemmRouteInfo", "family cfg splits flags")


def gemm_last_route():
    """Which kernel this thread's last gemm() / linear_backward() call launched (rec_gemm_last_route): family as a
    string (_lib.GEMM_ROUTE_FAMILIES; None before the first call), cfg = the tiled kernels' tile config ("128x80", ...;
    None elsewhere), splits = K slices (> 1: the split-K reduce applied the epilogue), flags = the names of the set
    _lib.GEMM_ROUTE_FLAGS bits as a frozenset."""
    r = _lib.GemmRoute()
    check(lib().rec_gemm_last_route(C.byref(r)), "rec_gemm_last_route")
    return GemmRouteInfo(_lib.GEMM_ROUTE_FAMILIES[r.family] if r.family >= 0 else None,
                         _lib.GEMM_CFGS[r.cfg] if r.cfg >= 0 else None, r.splits,
                         frozenset(n for n, b in _lib.GEMM_ROUTE_FLAGS.items() if r.flags & b))


@contextlib.contextmanager
def route_log():
    """Which kernels this thread's calls launch inside the block (rec_route_log_begin / rec_route_log_end): yields a
    list that holds, once the block is left, one note per launch of a host-routed entry point, in call order
    ("rows<4,16>", "ms_lane<9>", "din_fwd:ct:nopf2:split", ... — include/recengine.h names them all).  The log is off
    outside such a block; blocks do not nest."""
    notes = []
    check(_lib.lib().rec_route_log_begin(), "rec_route_log_begin")
    try:
        yield notes
    finally:
        buf, need = C.create_string_buffer(1 << 15), C.c_size_t(0)
        check(_lib.lib().rec_route_log_end(buf, C.c_size_t(len(buf)), C.byref(need)), "rec_route_log_end")
        notes.extend(buf.value.decode().splitlines())


_relu_bits_cache = {}


def _relu_bits_bytes(d):
    """Bytes of the ReLU bit mask of this call, 0 when it has no bit form (or REC_RELU_BITS=0)."""
    if os.environ.get("REC_RELU_BITS") == "0":
        return 0
    key = (d.m, d.n, d.k, d.lda, d.ldb, d.ldc, d.trans_a, d.trans_b, d.epilogue, d.split_k, os.environ.get("REC_GEMM_BF16X3"))
    nb = _relu_bits_cache.get(key)
    if nb is None:
        ok, nbytes = C.c_int32(0), C.c_size_t(0)
        check(lib().rec_gemm_relu_bits_bytes(C.byref(d), C.byref(ok), C.byref(nbytes)), "rec_gemm_relu_bits_bytes")
        nb = _relu_bits_cache[key] = nbytes.value if ok.value else 0
    return nb


def _gemm_prepare(A, B, trans_a, trans_b, epilogue, bias, aux0, aux1, out, split_k, b_colsum, row_scale, out2, num_cus,
                  b_image):
    """Checks of one rec_gemm_f32 call -> (descriptor, epilogue arguments, out, workspace bytes)."""
    lda, ldb = _chk_mat(A, "A"), _chk_mat(B, "B")
    K, M = (A.shape if trans_a else A.shape[::-1])
    N, K2 = (B.shape if trans_b else B.shape[::-1])
    if K != K2:
        raise RecError("inner dimensions differ: %d vs %d" % (K, K2))
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    ldc = _chk_mat(out, "out")
    if tuple(out.shape) != (M, N):
        raise RecError("out has shape %s, expected %s" % (tuple(out.shape), (M, N)))
    ld0 = ld1 = 0
    if aux0 is not None:
        ld0 = _chk_mat(aux0, "aux0")
    if aux1 is not None:
        ld1 = _chk_mat(aux1, "aux1")
    if bias is not None:
        _chk(bias, torch.float32, "bias")
        if bias.numel() != N:
            raise RecError("bias must have N elements")
    if b_colsum is not None:
        _chk(b_colsum, torch.float32, "b_colsum")
        if b_colsum.numel() != N:
            raise RecError("b_colsum must have N elements")
    rs_stride = 0
    if row_scale is not None:
        if not row_scale.is_cuda or row_scale.dtype != torch.float32 or row_scale.shape[0] != M:
            raise RecError("row_scale must be a float32 device tensor with M rows")
        rs_stride = row_scale.stride(0) if M > 1 else 1
    ld2 = 0
    if out2 is not None:
        ld2 = _chk_mat(out2, "out2")
        if tuple(out2.shape) != (M, N):
            raise RecError("out2 must have the shape of out")
    d = GemmDesc(M, N, K, lda, ldb, ldc, int(trans_a), int(trans_b), EPI[epilogue], int(split_k), int(max(num_cus, 0)))
    if num_cus > 0 and split_k <= 0:
        sp = C.c_int32(0)
        check(lib().rec_gemm_plan_splits(C.byref(d), int(num_cus), C.byref(sp)), "rec_gemm_plan_splits")
        d.split_k = sp.value
    pv = lambda t: None if t is None else t.data_ptr()
    x = GemmEpilogueArgs(pv(bias), pv(aux0), ld0, pv(aux1), ld1, pv(row_scale), rs_stride, pv(out2),
                         ld2, pv(b_colsum), pv(b_image))
    if _recorder is not None:      # a recorded step holds these addresses too
        _recorder.keep.extend(t for t in (bias, aux0, aux1, row_scale, out2, b_colsum, b_image) if t is not None)
    key = (M, N, K, lda, ldb, ldc, d.trans_a, d.trans_b, d.epilogue, d.split_k, d.num_cus,
           os.environ.get("REC_GEMM_BF16X3"), os.environ.get("REC_GEMM_BF16X3_DW"))
    need = _gemm_ws_cache.get(key)
    if need is None:       # a pure function of the descriptor: one C call per distinct GEMM, not per launch
        nbytes = C.c_size_t(0)
        check(lib().rec_gemm_f32_workspace_bytes(C.byref(d), C.byref(nbytes)))
        need = _gemm_ws_cache[key] = nbytes.value
    return d, x, out, need


def colsum(G, ws, out=None):
    ld = _chk_mat(G, "G")
    M, N = G.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=G.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_colsum_workspace_bytes(M, N, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    check(lib().rec_colsum(M, N, ld, _p(G), _p(out), _p(w), C.c_size_t(w.numel()), _stream()),
          "rec_colsum")
    return out


# ------------------------------------------------------------------ top MLP on the GEMM above
class _Acts(list):
    """mlp_forward's list of layer inputs; relu_bits[j] = the ReLU mask of acts[j] as bits, for mlp_backward's dX GEMMs."""
    relu_bits = None


def mlp_forward(x, weights, biases, ws, relu_last=False, out_last=None, images=None):
    """Linear(+bias)->ReLU ... ->Linear (deepfm/net.py:142-174) with Paddle-layout weights [in,out];
    bias and ReLU run in the GEMM epilogue.  relu_last: ReLU after the last layer too (the DNN tower of
    dcn_v2/net.py:161-184); out_last: buffer (view) for the last layer's output.
    images[i]: the bf16 x 3 image of weights[i] (GemmImages, current values) or None.
    Returns (y, acts): acts[i] = input of layer i."""
    acts = _Acts()
    bits = [None]                      # bits[j]: the ReLU mask of acts[j] as bits (gemm(relu_bits=)), or None
    n = len(weights)
    for i in range(n):
        acts.append(x)
        last = i == n - 1
        relu = not last or relu_last
        x = gemm(x, weights[i], ws, epilogue="bias_relu" if relu else "bias",
                 bias=biases[i], out=out_last if last else None, b_image=images[i] if images is not None else None,
                 relu_bits=bits if relu else None)
        if not relu:
            bits.append(None)
    acts.append(x)
    acts.relu_bits = bits
    return x, acts


def mlp_head_bwd(act, dz, w, ws, dw, db, relu=True, out=None):
    """Backward of a one-logit head Linear(n -> 1) behind a ReLU in ONE pass over act [B, n]: -> dx [B, n]; dw [n] (or
    [n,1]) and db [1] are written.  (rec_mlp_head_bwd)"""
    B, n = act.shape
    if out is None:
        out = torch.empty(B, n, dtype=torch.float32, device=act.device)
    nbytes = C.c_size_t(0)
    check(lib().rec_mlp_head_bwd_workspace_bytes(B, n, C.byref(nbytes)))
    wk = ws.get(nbytes.value)
    check(lib().rec_mlp_head_bwd(B, n, _p(act), act.stride(0), _p(dz), _p(w), 1 if relu else 0, _p(out), out.stride(0),
                                 _p(dw), _p(db), _p(wk), C.c_size_t(wk.numel()), _stream()), "rec_mlp_head_bwd")
    return out


def ctr_head_ok(w, dw):
    """The fused CTR head (rec_ctr_head_fwd_bwd) takes Linear(n -> 1) with n % 4 == 0, n <= 512 and an aligned contiguous
    weight (its input is the previous GEMM's own output buffer: contiguous, aligned)."""
    return (os.environ.get("REC_CTR_HEAD_FUSED", "1") != "0" and w.dim() == 2 and w.shape[1] == 1 and
            w.shape[0] % 4 == 0 and w.shape[0] <= 512 and w.is_contiguous() and w.data_ptr() % 16 == 0 and
            dw.is_contiguous())


def ctr_head(act, w, bias, y1, y2, label, ws, dw, db, eps=1e-4, clip=None, mean_over=0, relu=True, out=None):
    """Last Linear(n -> 1) + sigmoid + log_loss + mean AND their backward in one pass over act [B, n]
    (rec_ctr_head_fwd_bwd).  -> (pred [B,1], dz [B,1], loss [1], dx [B,n]); dw [n(,1)] and db [1] are written."""
    B, n = act.shape
    dev = act.device
    _chk(label, torch.int64, "label")
    for t, nm in ((y1, "y1"), (y2, "y2"), (bias, "bias")):
        _chk(t, torch.float32, nm)
    if label.numel() != B or (y1 is not None and y1.numel() != B) or (y2 is not None and y2.numel() != B):
        raise RecError("ctr_head: y1 / y2 / label must have one entry per row of act")
    if clip is not None and not clip[0] < clip[1]:
        raise RecError("clip must be (lo, hi) with lo < hi")
    if out is None:
        pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
        dz = torch.empty(B, 1, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dx = torch.empty(B, n, dtype=torch.float32, device=dev)
    else:
        pred, dz, loss, dx = out
    nbytes = C.c_size_t(0)
    check(lib().rec_ctr_head_workspace_bytes(B, n, C.byref(nbytes)))
    wk = ws.get(nbytes.value)
    lo, hi = (float(clip[0]), float(clip[1])) if clip is not None else (0.0, 0.0)
    check(lib().rec_ctr_head_fwd_bwd(B, n, int(mean_over), _p(act), act.stride(0), _p(w), _p(bias), _p(y1), _p(y2),
                                     _p(label), float(eps), lo, hi, 1 if relu else 0, None, _p(pred), _p(dz), _p(loss),
                                     _p(dx), dx.stride(0), _p(dw), _p(db), _p(wk), C.c_size_t(wk.numel()), _stream()),
          "rec_ctr_head_fwd_bwd")
    return pred, dz, loss, dx


def _head_ok(act, w, dw, db, dy):
    """A one-logit head the fused backward takes: Linear(n -> 1), n % 4 == 0, n <= 512, aligned contiguous operands."""
    return (os.environ.get("REC_MLP_HEAD_FUSED", "1") != "0" and w.dim() == 2 and w.shape[1] == 1 and
            w.shape[0] % 4 == 0 and w.shape[0] <= 512 and act.dim() == 2 and act.stride(1) == 1 and
            act.stride(0) % 4 == 0 and act.data_ptr() % 16 == 0 and w.is_contiguous() and w.data_ptr() % 16 == 0 and
            dw.is_contiguous() and dy.is_contiguous() and dy.shape[-1] == 1 and act.shape[0] >= 64)


def mlp_backward(dy, acts, weights, dws, dbs, ws, defer_first=False, defer_all=False, dw_stream=None, dw_ws=None,
                 defer_split=0, images_t=None, defer_cus=0):
    """Backward of mlp_forward: dW_i -> dws[i], db_i -> dbs[i] (preallocated views); returns d(input).
    ReLU' is applied in the epilogue of the dX GEMM (mask = layer input > 0).
    defer_first: compute d(input) BEFORE dW_0 and return (d_input, finish) where finish() launches the
    dW_0 / db_0 GEMM — lets the caller start the HBM-bound consumers of d(input) on another stream
    underneath that MFMA-bound GEMM.
    defer_all: run the whole dX chain first and return (d_input, finish) with EVERY dW / db GEMM in finish()
    — the row-sharded step hides its gradient exchange, sparse optimizer and the next batch's lookup under them."""
    n = len(weights)
    g = dy
    imt = (lambda i: images_t[i]) if images_t is not None else (lambda i: None)   # images of weights[i]^T (the dX GEMMs)
    rbl = getattr(acts, "relu_bits", None)
    rb = (lambda i: rbl[i]) if rbl is not None else (lambda i: None)              # ReLU mask of acts[i] as bits
    head = n > 1 and _head_ok(acts[n - 1], weights[n - 1], dws[n - 1], dbs[n - 1], dy)
    if head:
        # the one-logit head: dX (with the ReLU mask of the layer in front), dW and db in ONE pass over its input
        g = mlp_head_bwd(acts[n - 1], dy, weights[n - 1], ws, dws[n - 1], dbs[n - 1], relu=True)
        n_run = n - 1
    else:
        n_run = n
    if defer_all:
        gs = [None] * n_run
        for i in reversed(range(n_run)):
            gs[i] = g
            g = gemm(g, weights[i], ws, trans_b=True, b_image=imt(i),
                     **(dict(epilogue="relu_mask", aux0=acts[i], relu_bits=rb(i)) if i > 0 else {}))

        def finish(num_cus=0):
            for i in reversed(range(n_run)):
                gemm(acts[i], gs[i], ws, trans_a=True, out=dws[i], b_colsum=dbs[i], num_cus=num_cus)
        return g, finish
    cur = torch.cuda.current_stream() if dw_stream is not None else None
    keep = []          # dw_stream: tensors the other stream still reads (the caching allocator must not recycle them)

    def join():
        if dw_stream is not None:
            cur.wait_stream(dw_stream)
            keep.clear()
    for i in reversed(range(n_run)):
        if i == 0 and defer_first:
            g0 = g
            d_in = gemm(g0, weights[0], ws, trans_b=True, b_image=imt(0))
            join()
            # defer_cus: the deferred dW_0's grid sized for that many CUs (the bf16 x 3 kernel: one block per CU)
            # defer_split: K split of the deferred dW_0 GEMM (0 = the planner's: one resident round of blocks) — the
            # caller that runs an HBM-bound kernel beside it asks for fewer, longer blocks, which leave it wave slots
            return d_in, (lambda: gemm(acts[0], g0, ws, trans_a=True, out=dws[0], b_colsum=dbs[0], split_k=defer_split,
                                    num_cus=defer_cus))
        if dw_stream is not None:
            # dW_i and dX_i both consume g_i and nothing of each other: two streams, so that the half-empty last
            # round of blocks of one GEMM is filled by the other
            dw_stream.wait_stream(cur)
            keep.append(g)
            with torch.cuda.stream(dw_stream):
                gemm(acts[i], g, dw_ws if dw_ws is not None else ws, trans_a=True, out=dws[i], b_colsum=dbs[i])
        else:
            # dW = X^T G, db = colsum(G) and dX = G W^T (+ ReLU') in one call: one launch at launch-bound sizes
            g = linear_backward(acts[i], g, weights[i], ws, dws[i], dbs[i], relu_src=acts[i] if i > 0 else None,
                                b_image=imt(i), relu_bits=rb(i) if i > 0 else None)
            continue
        if i > 0:
            g = gemm(g, weights[i], ws, trans_b=True, epilogue="relu_mask", aux0=acts[i], b_image=imt(i), relu_bits=rb(i))
        else:
            g = gemm(g, weights[i], ws, trans_b=True, b_image=imt(i))
    join()
    return g


# ------------------------------------------------------------------ loss head / metric
def sigmoid_logloss(y1, y2, y_dnn, label, ws, eps=1e-4, want_dz=True, out=None, mean_over=0, clip=None):
    """-> pred [B,1], dz [B,1] (or None), loss [1].  mean_over: denominator of the mean (0 -> B).
    clip = (lo, hi): paddle.clip on the logit in front of the sigmoid (slot_dnn/net.py:84)."""
    B = y1.numel()
    dev = y1.device
    _chk(y1, torch.float32, "y1")
    _chk(y2, torch.float32, "y2")
    _chk(y_dnn, torch.float32, "y_dnn")
    _chk(label, torch.int64, "label")
    if clip is not None and not clip[0] < clip[1]:
        raise RecError("clip must be (lo, hi) with lo < hi")
    if out is None:
        pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
        dz = torch.empty(B, 1, dtype=torch.float32, device=dev) if want_dz else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    else:
        pred, dz, loss = out
    nbytes = C.c_size_t(0)
    check(lib().rec_logloss_workspace_bytes(B, C.byref(nbytes)))
    w = ws.get(nbytes.value)
    lo, hi = (float(clip[0]), float(clip[1])) if clip is not None else (0.0, 0.0)
    check(lib().rec_sigmoid_logloss(B, int(mean_over), _p(y1), _p(y2), _p(y_dnn), _p(label), float(eps), lo, hi,
                                    _p(pred), _p(dz), _p(loss), _p(w), C.c_size_t(w.numel()), _stream()),
          "rec_sigmoid_logloss")
    return pred, dz, loss


def auc_histogram(pred, label, stat_pos, stat_neg, num_thresholds=4095):
    _chk(pred, torch.float32, "pred")
    _chk(label, torch.int64, "label")
    _chk(stat_pos, torch.int64, "stat_pos", (num_thresholds + 1,))
    _chk(stat_neg, torch.int64, "stat_neg", (num_thresholds + 1,))
    check(lib().rec_auc_histogram(pred.numel(), _p(pred), _p(label), num_thresholds, _p(stat_pos),
                                  _p(stat_neg), _stream()), "rec_auc_histogram")


def fill_uniform(buf, lo, hi, seed):
    _chk(buf, torch.float32, "buf")
    check(lib().rec_fill_uniform(buf.numel(), _p(buf), float(lo), float(hi), int(seed), _stream()),
          "rec_fill_uniform")
    return buf


_SIDE_STREAMS = {}


def concurrent_stream(device, tries=8, micros=200, priority=None, index=0):
    """A side stream whose kernels really run CONCURRENTLY with the current stream's.  HIP multiplexes streams
    onto a few hardware queues (4 by default, shared with the streams RCCL and rocPRIM create); two streams on
    one queue execute strictly in submission order, which silently turns 'sparse optimizer underneath the dW
    GEMM' into 'after it'.  Probe: spin `micros` on a candidate, then on the current stream, and accept the
    candidate if the second spin did not have to wait for the first (events).  Cached per (device, main stream).
    index > 0: a further stream that also overlaps with the side streams of the lower indices (its own hardware queue)."""
    device = torch.device(device)
    main = torch.cuda.current_stream(device)
    if priority is None:
        priority = int(os.environ.get("REC_SIDE_PRIORITY", "0"))      # -1 = high priority queue (measured: no effect)
    key = (device.index, main.cuda_stream, priority, int(index))
    if key in _SIDE_STREAMS:
        return _SIDE_STREAMS[key]
    others = [main] + [concurrent_stream(device, tries, micros, priority, j) for j in range(int(index))]

    def overlaps(s, o):
        for st in (s, o):                                         # first use of a stream binds its queue
            check(lib().rec_stream_spin(1, C.c_void_p(st.cuda_stream)), "rec_stream_spin")
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(o)
        check(lib().rec_stream_spin(micros, C.c_void_p(s.cuda_stream)), "rec_stream_spin")
        check(lib().rec_stream_spin(micros, C.c_void_p(o.cuda_stream)), "rec_stream_spin")
        e1.record(o)
        torch.cuda.synchronize(device)
        return e0.elapsed_time(e1) * 1e3 < 1.5 * micros
    s, keep = None, []
    with torch.cuda.device(device):
        for _ in range(tries):
            s = torch.cuda.Stream(device=device, priority=priority)
            keep.append(s)          # rejected candidates stay alive until the search ends: a freed stream's queue slot
            if all(overlaps(s, o) for o in others):               # would be handed to the next candidate again
                break
    _SIDE_STREAMS[key] = s
    return s


_CU_STREAMS = {}


def cu_range_stream(device, cu_begin, cu_end):
    """torch stream (ExternalStream over rec_stream_create_cu_range) whose kernels only run on compute units
    [cu_begin, cu_end).  Cached for the life of the process."""
    device = torch.device(device)
    key = (device.index, int(cu_begin), int(cu_end))
    if key not in _CU_STREAMS:
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(lib().rec_stream_create_cu_range(int(cu_begin), int(cu_end), C.byref(h)),
                  "rec_stream_create_cu_range")
        _CU_STREAMS[key] = torch.cuda.ExternalStream(h.value, device=device)
    return _CU_STREAMS[key]


def cu_stride_stream(device, first, stride, cu_total=256):
    """torch stream whose kernels only run on every `stride`-th compute unit (rec_stream_create_cu_stride)."""
    device = torch.device(device)
    key = (device.index, "stride", int(first), int(stride), int(cu_total))
    if key not in _CU_STREAMS:
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(lib().rec_stream_create_cu_stride(int(first), int(stride), int(cu_total), C.byref(h)),
                  "rec_stream_create_cu_stride")
        _CU_STREAMS[key] = torch.cuda.ExternalStream(h.value, device=device)
    return _CU_STREAMS[key]


# ------------------------------------------------------------------ host: feature hash
def xxh32(data: bytes, seed: int = 0) -> int:
    return int(lib().rec_xxh32(data, len(data), seed))


def hash_features(field_idx, values, hash_dim=1000001):
    """xxh32(str(idx)+value) % hash_dim for each (idx, value) — dnn/benchmark_reader.py:52."""
    n = len(values)
    arr = (C.c_char_p * n)(*[v.encode("utf-8") for v in values])
    idx = (C.c_int32 * n)(*[int(i) for i in field_idx])
    out = (C.c_int64 * n)()
    check(lib().rec_xxh32_hash_mod(arr, idx, n, hash_dim, out), "rec_xxh32_hash_mod")
    return list(out)


# ------------------------------------------------------------------ ENSFM (csrc/ensfm_ops.hip)
def _ensfm_buf(scratch, key, numel, device):
    """A float32 buffer of the step's, kept in `scratch` (a dict of the caller's, or None) while it is large enough."""
    t = None if scratch is None else scratch.get(key)
    if t is None or t.numel() < numel:
        t = torch.empty(max(int(numel), 1), dtype=torch.float32, device=device)
        if scratch is not None:
            scratch[key] = t
    return t


def ensfm_tower_fwd(ids, table, bias_table, H_s, bias=None, item_layout=False, status=None, out=None):
    """One side of net.py:65-83 (rec_ensfm_tower_fwd): ids int64 [n, F]; table [rows, D]; bias_table [bias_rows] or
    [bias_rows, 1]; H_s [D] or [D, 1]; bias [1] or None.  -> out [n, D + 2] = [s, score, 1] (user) or [s, 1, score] (item)."""
    _chk(ids, torch.int64, "ids")
    if ids.dim() != 2:
        raise RecError("ensfm_tower_fwd: ids must be [n, F]")
    D, ld = _chk_table(table, "table")
    _chk(bias_table, torch.float32, "bias_table")
    _chk(H_s, torch.float32, "H_s")
    _chk(bias, torch.float32, "bias")
    if H_s.numel() != D:
        raise RecError("ensfm_tower_fwd: H_s must hold D = %d floats" % D)
    n, F = ids.shape
    if out is None:
        out = torch.empty(n, D + 2, dtype=torch.float32, device=table.device)
    if tuple(out.shape) != (n, D + 2):
        raise RecError("ensfm_tower_fwd: out must be [n, D + 2]")
    check(lib().rec_ensfm_tower_fwd(n, F, D, table.shape[0], bias_table.numel(), _p(ids), _p(table), ld, _p(bias_table), _p(H_s),
                                    _p(bias), int(bool(item_layout)), _p(out), _rows_view(out, "out"), _p(status), _stream()),
          "rec_ensfm_tower_fwd")
    return out


def ensfm_tower_partials(n, D):
    """Floats of rec_ensfm_tower_bwd's partials for n rows."""
    return max(1, min(-(-n // 4), _lib.REC_ENSFM_MAX_PARTIALS)) * (D + 1)


def ensfm_tower_bwd(ids, table, H_s, d_out, dH_s, dbias=None, item_layout=False, accumulate=False, scratch=None, rows=None,
                    dscore=None):
    """rec_ensfm_tower_bwd -> (rows [n F, D]: the gradient row of every lookup; dscore [n]: the gradient of every bias lookup
    of a row).  dH_s [D] and dbias [1] (or None) are written, or added to with accumulate."""
    _chk(ids, torch.int64, "ids")
    D, ld = _chk_table(table, "table")
    n, F = ids.shape
    ldd = _rows_view(d_out, "d_out")
    if tuple(d_out.shape) != (n, D + 2):
        raise RecError("ensfm_tower_bwd: d_out must be [n, D + 2]")
    _chk(H_s, torch.float32, "H_s")
    _chk(dH_s, torch.float32, "dH_s")
    _chk(dbias, torch.float32, "dbias")
    if H_s.numel() != D or dH_s.numel() != D:
        raise RecError("ensfm_tower_bwd: H_s and dH_s must hold D = %d floats" % D)
    dev = table.device
    if rows is None:
        rows = torch.empty(n * F, D, dtype=torch.float32, device=dev)
    if dscore is None:
        dscore = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    if tuple(rows.shape) != (n * F, D) or dscore.numel() < n:
        raise RecError("ensfm_tower_bwd: rows must be [n F, D] and dscore [n]")
    part = _ensfm_buf(scratch, "tower_partials", ensfm_tower_partials(n, D), dev)
    check(lib().rec_ensfm_tower_bwd(n, F, D, table.shape[0], _p(ids), _p(table), ld, _p(H_s), _p(d_out), ldd,
                                    int(bool(item_layout)), _p(rows), _rows_view(rows, "rows"), _p(dscore), _p(part), _p(dH_s),
                                    _p(dbias), int(bool(accumulate)), _stream()), "rec_ensfm_tower_bwd")
    return rows, dscore


def ensfm_gram(X, scratch=None, out=None):
    """G = X^T X (rec_ensfm_gram) for a [n, C] view X -> [C, C]."""
    ldx = _rows_view(X, "X")
    n, Cc = X.shape
    if out is None:
        out = torch.empty(Cc, Cc, dtype=torch.float32, device=X.device)
    _chk(out, torch.float32, "out", (Cc, Cc))
    if n == 0:
        return out.zero_()                               # nothing is launched for an empty X
    part = _ensfm_buf(scratch, "gram_partials", min(-(-n // 64), _lib.REC_ENSFM_GRAM_MAX_BLOCKS) * Cc * Cc, X.device)
    check(lib().rec_ensfm_gram(n, Cc, _p(X), ldx, _p(part), _p(out), _stream()), "rec_ensfm_gram")
    return out


def _ensfm_pq(p, q, H_i, what):
    ldp, ldq = _rows_view(p, "p"), _rows_view(q, "q")
    _chk(H_i, torch.float32, "H_i")
    D = H_i.numel()
    if p.shape[1] != D + 2 or q.shape[1] != D + 2:
        raise RecError("%s: p and q must have D + 2 = %d columns" % (what, D + 2))
    return D, ldp, ldq


def ensfm_pos_user(ur, p, q, H_i, G_q, neg_weight, status=None, want_pos_r=False):
    """The positives, user-owned (rec_ensfm_pos_user): ur int64 [B, P] padded with I = q.shape[0] - 1.
    -> (g [B, P], dP [B, C], loss_part [B], dHi_part [B, D], pos_r [B, P] or None)."""
    _chk(ur, torch.int64, "ur")
    D, ldp, ldq = _ensfm_pq(p, q, H_i, "ensfm_pos_user")
    _chk(G_q, torch.float32, "G_q", (D + 2, D + 2))
    if ur.dim() != 2 or ur.shape[0] != p.shape[0]:
        raise RecError("ensfm_pos_user: ur must be [B, P] with one row per row of p")
    B, P = ur.shape
    f32 = dict(dtype=torch.float32, device=p.device)
    g, dP = torch.empty(B, P, **f32), torch.empty(B, D + 2, **f32)
    loss_part, dHi_part = torch.empty(max(B, 1), **f32), torch.empty(max(B, 1), D, **f32)
    pos_r = torch.empty(B, P, **f32) if want_pos_r else None
    check(lib().rec_ensfm_pos_user(B, P, D, q.shape[0] - 1, float(neg_weight), _p(ur), _p(p), ldp, _p(q), ldq, _p(H_i), _p(G_q),
                                   _p(g), _p(pos_r), _p(dP), D + 2, _p(loss_part), _p(dHi_part), _p(status), _stream()),
          "rec_ensfm_pos_user")
    return g, dP, loss_part, dHi_part, pos_r


def ensfm_pos_item(groups, g, p, q, H_i, G_p, neg_weight, out=None):
    """The positives, item-owned (rec_ensfm_pos_item): groups = ids_group(ur.view(-1), I + 1, I, ...); g [B, P] of
    ensfm_pos_user.  -> dQ [I + 1, C] for all rows."""
    D, ldp, ldq = _ensfm_pq(p, q, H_i, "ensfm_pos_item")
    _chk(G_p, torch.float32, "G_p", (D + 2, D + 2))
    _chk(g, torch.float32, "g")
    B = p.shape[0]
    if g.dim() != 2 or g.shape[0] != B or groups.n != g.numel():
        raise RecError("ensfm_pos_item: g must be [B, P] and groups the grouping of its B P positions")
    if out is None:
        out = torch.empty(q.shape[0], D + 2, dtype=torch.float32, device=q.device)
    if tuple(out.shape) != (q.shape[0], D + 2):
        raise RecError("ensfm_pos_item: out must be [I + 1, D + 2]")
    check(lib().rec_ensfm_pos_item(B, g.shape[1], D, q.shape[0] - 1, float(neg_weight), _p(groups.n_uniq), _p(groups.uniq_rows),
                                   _p(groups.seg_offset), _p(groups.sorted_pos), _p(g), _p(p), ldp, _p(q), ldq, _p(H_i), _p(G_p),
                                   _p(out), _rows_view(out, "out"), _stream()), "rec_ensfm_pos_item")
    return out


def ensfm_loss(G_p, G_q, H_i, loss_part, dHi_part, neg_weight, B, loss=None, dH_i=None):
    """rec_ensfm_loss -> (loss [1], dH_i [D])."""
    for t, name in ((G_p, "G_p"), (G_q, "G_q"), (H_i, "H_i"), (loss_part, "loss_part"), (dHi_part, "dHi_part")):
        _chk(t, torch.float32, name)
    D = H_i.numel()
    if G_p.numel() != (D + 2) ** 2 or G_q.numel() != (D + 2) ** 2 or loss_part.numel() < B or dHi_part.numel() < B * D:
        raise RecError("ensfm_loss: G_p, G_q [D + 2, D + 2], loss_part [B] and dHi_part [B, D] do not fit")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=H_i.device)
    if dH_i is None:
        dH_i = torch.empty(D, dtype=torch.float32, device=H_i.device)
    _chk(loss, torch.float32, "loss")
    _chk(dH_i, torch.float32, "dH_i")
    if dH_i.numel() != D:
        raise RecError("ensfm_loss: dH_i must hold D floats")
    check(lib().rec_ensfm_loss(int(B), D, float(neg_weight), _p(G_p), _p(G_q), _p(H_i), _p(loss_part), _p(dHi_part), _p(loss),
                               _p(dH_i), _stream()), "rec_ensfm_loss")
    return loss, dH_i


def ensfm_score(p, q, H_i, out=None):
    """pre [B, I + 1] = (p o h) q^T (rec_ensfm_score): the model's output for --infer; `dot` is never formed."""
    D, ldp, ldq = _ensfm_pq(p, q, H_i, "ensfm_score")
    B, rows = p.shape[0], q.shape[0]
    if out is None:
        out = torch.empty(B, rows, dtype=torch.float32, device=p.device)
    if tuple(out.shape) != (B, rows):
        raise RecError("ensfm_score: out must be [B, I + 1]")
    check(lib().rec_ensfm_score(B, rows, D, _p(p), ldp, _p(q), ldq, _p(H_i), _p(out), _rows_view(out, "out"), _stream()),
          "rec_ensfm_score")
    return out


# ------------------------------------------------------------------ NCF (models/recall/ncf, csrc/ncf_ops.hip)
class NcfDesc:
    """The five arguments that name the net to every rec_ncf_* entry: mf_dim, n_fc, widths (host int32 [n_fc + 1]), num_users,
    num_items."""

    def __init__(self, num_users, num_items, mf_dim, widths):
        widths = [int(w) for w in widths]
        self.mf_dim, self.n_fc, self.num_users, self.num_items = int(mf_dim), max(len(widths) - 1, 0), int(num_users), int(num_items)
        self.widths = (C.c_int32 * max(len(widths), 1))(*widths)

    def args(self):
        return self.mf_dim, self.n_fc, self.widths if self.n_fc > 0 else None, self.num_users, self.num_items


def ncf_desc(num_users, num_items, mf_dim, widths):
    """widths = [fc_layers[0], the outputs of the tower's Linears...] ([] in GMF mode); mf_dim 0 in MLP mode."""
    return NcfDesc(num_users, num_items, mf_dim, widths)


def ncf_dense_layout(mf_dim, widths):
    """The dense buffer of include/recengine.h -> ([(name, offset, shape)], P): layer_i.weight [in, out], layer_i.bias,
    prediction.weight [width, 1], prediction.bias; every tensor starts at a multiple of 4 floats."""
    out, off = [], 0
    for i in range(1, len(widths)):
        out.append(("layer_%d.weight" % i, off, (widths[i - 1], widths[i])))
        off += -(-widths[i - 1] * widths[i] // 4) * 4
        out.append(("layer_%d.bias" % i, off, (widths[i],)))
        off += -(-widths[i] // 4) * 4
    pw = int(mf_dim) + (widths[-1] if len(widths) > 1 else 0)
    out.append(("prediction.weight", off, (pw, 1)))
    off += -(-pw // 4) * 4
    out.append(("prediction.bias", off, (1,)))
    return out, off + 4


def ncf_dense_numel(desc):
    n = C.c_int64(0)
    check(lib().rec_ncf_dense_numel(*desc.args(), C.byref(n)), "rec_ncf_dense_numel")
    return n.value


def ncf_fused_eligible(desc):
    """True when rec_ncf_step / rec_ncf_score take the net (host query, no device needed)."""
    ok = C.c_int32(0)
    check(lib().rec_ncf_fused_eligible(*desc.args(), C.byref(ok)), "rec_ncf_fused_eligible")
    return bool(ok.value)


def _ncf_ids(users, items, labels=None):
    for t, n in ((users, "users"), (items, "items"), (labels, "labels")):
        _chk(t, torch.int64, n)
    B = users.numel()
    if items.numel() != B or (labels is not None and labels.numel() != B):
        raise RecError("ncf: users, items and labels must have one entry per sample")
    return B


def _ncf_out(t, B, cols, dev, name):
    if t is None:
        return torch.empty(B, cols, dtype=torch.float32, device=dev)
    if t.dim() != 2 or tuple(t.shape) != (B, cols):
        raise RecError("%s must be [%d, %d]" % (name, B, cols))
    return t


def ncf_partials_numel(B, P):
    return max(1, min(-(-B // _lib.REC_NCF_TILE), _lib.REC_NCF_MAX_BLOCKS)) * (P + 1)


def ncf_step(desc, users, items, labels, user_table, item_table, dense, g_dense, mean_over=0, status=None, pred=None,
             g_user=None, g_item=None, loss=None, scratch=None):
    """rec_ncf_step: forward, loss and backward of the whole net in one launch -> (pred [B], g_user [B, Cu], g_item [B, Ci],
    loss [1]); g_dense [P] is written."""
    B = _ncf_ids(users, items, labels)
    Cu, ldu = _chk_table(user_table, "user_table")
    Ci, ldi = _chk_table(item_table, "item_table")
    _chk(dense, torch.float32, "dense")
    _chk(g_dense, torch.float32, "g_dense")
    P = ncf_dense_numel(desc)
    if dense.numel() != P or g_dense.numel() != P:
        raise RecError("ncf_step: dense and g_dense must hold P = %d floats" % P)
    dev = dense.device
    if pred is None:
        pred = torch.empty(B, dtype=torch.float32, device=dev)
    _chk(pred, torch.float32, "pred")
    g_user, g_item = _ncf_out(g_user, B, Cu, dev, "g_user"), _ncf_out(g_item, B, Ci, dev, "g_item")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    _chk(loss, torch.float32, "loss")
    part = _ensfm_buf(scratch, "ncf_partials", ncf_partials_numel(B, P), dev)
    check(lib().rec_ncf_step(*desc.args(), B, int(mean_over), _p(users), _p(items), _p(labels), _p(user_table), ldu,
                             _p(item_table), ldi, _p(dense), _p(pred), _p(g_user), _rows_view(g_user, "g_user"), _p(g_item),
                             _rows_view(g_item, "g_item"), _p(part), _p(g_dense), _p(loss), _p(status), _stream()),
          "rec_ncf_step")
    return pred, g_user, g_item, loss


def ncf_score(desc, users, items, user_table, item_table, dense, status=None, pred=None):
    """rec_ncf_score: the fused forward alone -> pred [B]."""
    B = _ncf_ids(users, items)
    ldu, ldi = _chk_table(user_table, "user_table")[1], _chk_table(item_table, "item_table")[1]
    _chk(dense, torch.float32, "dense")
    if dense.numel() != ncf_dense_numel(desc):
        raise RecError("ncf_score: dense must hold P floats")
    if pred is None:
        pred = torch.empty(B, dtype=torch.float32, device=dense.device)
    _chk(pred, torch.float32, "pred")
    check(lib().rec_ncf_score(*desc.args(), B, _p(users), _p(items), _p(user_table), ldu, _p(item_table), ldi, _p(dense),
                              _p(pred), _p(status), _stream()), "rec_ncf_score")
    return pred


def ncf_gather_fwd(desc, users, items, user_table, item_table, pred_in, mlp_in, status=None):
    """rec_ncf_gather_fwd: mf_u o mf_i -> pred_in[:, :mf_dim]; [mlp_u, mlp_i] -> mlp_in (either may be None in the mode
    without it).  Both are [B, .] float32 views with any row stride."""
    B = _ncf_ids(users, items)
    ldu, ldi = _chk_table(user_table, "user_table")[1], _chk_table(item_table, "item_table")[1]
    ldp = _rows_view(pred_in, "pred_in") if pred_in is not None else 0
    ldm = _rows_view(mlp_in, "mlp_in") if mlp_in is not None else 0
    check(lib().rec_ncf_gather_fwd(*desc.args(), B, _p(users), _p(items), _p(user_table), ldu, _p(item_table), ldi,
                                   _p(pred_in), ldp, _p(mlp_in), ldm, _p(status), _stream()), "rec_ncf_gather_fwd")


def ncf_gather_bwd(desc, users, items, user_table, item_table, d_pred_in, d_mlp_in, g_user=None, g_item=None):
    """rec_ncf_gather_bwd -> (g_user [B, Cu], g_item [B, Ci]) as ncf_step writes them."""
    B = _ncf_ids(users, items)
    Cu, ldu = _chk_table(user_table, "user_table")
    Ci, ldi = _chk_table(item_table, "item_table")
    ldp = _rows_view(d_pred_in, "d_pred_in") if d_pred_in is not None else 0
    ldm = _rows_view(d_mlp_in, "d_mlp_in") if d_mlp_in is not None else 0
    dev = user_table.device
    g_user, g_item = _ncf_out(g_user, B, Cu, dev, "g_user"), _ncf_out(g_item, B, Ci, dev, "g_item")
    check(lib().rec_ncf_gather_bwd(*desc.args(), B, _p(users), _p(items), _p(user_table), ldu, _p(item_table), ldi,
                                   _p(d_pred_in), ldp, _p(d_mlp_in), ldm, _p(g_user), _rows_view(g_user, "g_user"), _p(g_item),
                                   _rows_view(g_item, "g_item"), _stream()), "rec_ncf_gather_bwd")
    return g_user, g_item


# ------------------------------------------------------------------ DSSM (models/match/dssm, csrc/dssm_ops.hip)
DSSM_MAX_DOCS, DSSM_MAX_WIDTH = _lib.REC_DSSM_MAX_DOCS, _lib.REC_DSSM_MAX_WIDTH


def _dssm_csr(cols, vals, lod, what):
    """A tower input in CSR (include/recengine.h): cols int64 [nnz], vals float32 [nnz], lod int64 [rows + 1] -> (rows, nnz)."""
    _chk(cols, torch.int64, "cols")
    _chk(vals, torch.float32, "vals")
    _chk(lod, torch.int64, "lod")
    if cols.dim() != 1 or vals.dim() != 1 or lod.dim() != 1 or cols.numel() != vals.numel() or lod.numel() < 1:
        raise RecError("%s: cols and vals must be [nnz] and lod [rows + 1]" % what)
    return lod.numel() - 1, cols.numel()


def dssm_lod_rows(lod, nnz, out=None):
    """rec_dssm_lod_rows: row_of [nnz] int32, the row of every CSR entry."""
    _chk(lod, torch.int64, "lod")
    if lod.dim() != 1 or lod.numel() < 1:
        raise RecError("dssm_lod_rows: lod must be [rows + 1]")
    if out is None:
        out = torch.empty(max(int(nnz), 1), dtype=torch.int32, device=lod.device)
    _chk(out, torch.int32, "row_of")
    if out.numel() < nnz:
        raise RecError("dssm_lod_rows: row_of shorter than nnz")
    check(lib().rec_dssm_lod_rows(lod.numel() - 1, int(nnz), _p(lod), _p(out), _stream()), "rec_dssm_lod_rows")
    return out


def dssm_sparse_linear_fwd(cols, vals, lod, W, bias, relu=False, status=None, out=None):
    """rec_dssm_sparse_linear_fwd: Y [rows, n] = act(bias + sum_j vals[j] W[cols[j], :]); W [in_dim, n] (row stride allowed)."""
    R, nnz = _dssm_csr(cols, vals, lod, "dssm_sparse_linear_fwd")
    ldw = _chk_mat(W, "W")
    T, N = W.shape
    _chk(bias, torch.float32, "bias")
    if bias.numel() != N:
        raise RecError("dssm_sparse_linear_fwd: bias must have n = %d elements" % N)
    if out is None:
        out = torch.empty(R, N, dtype=torch.float32, device=W.device)
    ldy = _chk_mat(out, "out")
    if tuple(out.shape) != (R, N):
        raise RecError("dssm_sparse_linear_fwd: out has shape %s, expected %s" % (tuple(out.shape), (R, N)))
    check(lib().rec_dssm_sparse_linear_fwd(R, nnz, T, N, int(bool(relu)), _p(cols), _p(vals), _p(lod), _p(W), ldw, _p(bias), _p(out),
                                           ldy, _p(status), _stream()), "rec_dssm_sparse_linear_fwd")
    return out


def dssm_sparse_linear_bwd(vals, row_of, groups, dY, dW):
    """rec_dssm_sparse_linear_bwd: dW [in_dim, n] (every row written) from the entries grouped by column — groups: the
    IdGroups of ids_group(cols, in_dim, None, ...) — vals [nnz], row_of [nnz] int32 and dY [rows, n]."""
    _chk(vals, torch.float32, "vals")
    _chk(row_of, torch.int32, "row_of")
    nnz = vals.numel()
    if groups.n != nnz or row_of.numel() < nnz:
        raise RecError("dssm_sparse_linear_bwd: groups and row_of must cover the nnz = %d entries" % nnz)
    lddy, lddw = _chk_mat(dY, "dY"), _chk_mat(dW, "dW")
    R, N = dY.shape
    T = dW.shape[0]
    if dW.shape[1] != N:
        raise RecError("dssm_sparse_linear_bwd: dW must be [in_dim, %d]" % N)
    U = min(nnz, T)                                            # the kernel reads at most that many groups, whatever n_uniq says
    for t, dt, need, name in ((groups.sorted_pos, torch.int32, nnz, "sorted_pos"), (groups.uniq_rows, torch.int64, U, "uniq_rows"),
                              (groups.seg_offset, torch.int32, U + 1, "seg_offset"), (groups.n_uniq, torch.int32, 1, "n_uniq")):
        _chk(t, dt, name)
        if t is None or t.numel() < need:
            raise RecError("dssm_sparse_linear_bwd: groups.%s must hold at least %d entries" % (name, need))
    check(lib().rec_dssm_sparse_linear_bwd(R, nnz, T, N, _p(vals), _p(row_of), _p(groups.sorted_pos), _p(groups.uniq_rows),
                                           _p(groups.seg_offset), _p(groups.n_uniq), _p(dY), lddy, _p(dW), lddw, _stream()),
          "rec_dssm_sparse_linear_bwd")
    return dW


def dssm_head_step(q, d, slice_end, relu_mask=False, out=None):
    """rec_dssm_head_step: q [B, n], d [(1 + neg) B, n] field-major -> dict(cos [B, 1 + neg], hit_prob [B], loss_terms [B],
    loss [1], dq [B, n], dd [(1 + neg) B, n]).  out: such a dict from an earlier call of the same shapes, reused."""
    ldq, ldd = _chk_mat(q, "q"), _chk_mat(d, "d")
    B, N = q.shape
    if d.shape[1] != N or (d.shape[0] % B if B else d.shape[0]):
        raise RecError("dssm_head_step: d must be [(1 + neg) * %d, %d], got %s" % (B, N, tuple(d.shape)))
    docs = d.shape[0] // B if B else 1
    if docs < 1:
        raise RecError("dssm_head_step: d holds no positive rows")
    if out is None:
        f32 = dict(dtype=torch.float32, device=q.device)
        out = dict(cos=torch.empty(B, docs, **f32), hit_prob=torch.empty(B, **f32), loss_terms=torch.empty(B, **f32),
                   loss=torch.zeros(1, **f32), dq=torch.empty(B, N, **f32), dd=torch.empty(docs * B, N, **f32))
    for key, shape in (("cos", (B, docs)), ("hit_prob", (B,)), ("loss_terms", (B,)), ("loss", (1,))):
        _chk(out[key], torch.float32, key, shape)
    lddq, lddd = _chk_mat(out["dq"], "dq"), _chk_mat(out["dd"], "dd")
    if tuple(out["dq"].shape) != (B, N) or tuple(out["dd"].shape) != (docs * B, N):
        raise RecError("dssm_head_step: dq / dd must have the shapes of q / d")
    check(lib().rec_dssm_head_step(B, docs - 1, N, int(slice_end), int(bool(relu_mask)), _p(q), ldq, _p(d), ldd, _p(out["cos"]),
                                   _p(out["hit_prob"]), _p(out["loss_terms"]), _p(out["loss"]), _p(out["dq"]), lddq,
                                   _p(out["dd"]), lddd, _stream()), "rec_dssm_head_step")
    return out


def dssm_cos(q, d, out=None):
    """rec_dssm_cos: Paddle's cosine_similarity of q [B, n] against d [B, n] -> [B]."""
    ldq, ldd = _chk_mat(q, "q"), _chk_mat(d, "d")
    B, N = q.shape
    if tuple(d.shape) != (B, N):
        raise RecError("dssm_cos: q and d must have one shape")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=q.device)
    _chk(out, torch.float32, "out", (B,))
    check(lib().rec_dssm_cos(B, N, _p(q), ldq, _p(d), ldd, _p(out), _stream()), "rec_dssm_cos")
    return out


# ------------------------------------------------------------------ MatchPyramid (models/match/match-pyramid, csrc/match_pyramid_ops.hip)
MPYR_MAX_LEFT, MPYR_MAX_RIGHT, MPYR_MAX_EMB = _lib.REC_MPYR_MAX_LEFT, _lib.REC_MPYR_MAX_RIGHT, _lib.REC_MPYR_MAX_EMB
MPYR_MAX_WEIGHTS, MPYR_MAX_POOLED, MPYR_MAX_BAND = _lib.REC_MPYR_MAX_WEIGHTS, _lib.REC_MPYR_MAX_POOLED, _lib.REC_MPYR_MAX_BAND

MpyrShape = collections.namedtuple("MpyrShape", "left_len right_len emb_dim channels filter_h filter_w pool_h pool_w stride_h "
                                                "stride_w relu")


def mpyr_pooled_shape(shape):
    """(PH, PW) of the VALID pool of an MpyrShape."""
    return (shape.left_len - shape.pool_h) // shape.stride_h + 1, (shape.right_len - shape.pool_w) // shape.stride_w + 1


def mpyr_shape_error(shape):
    """None, or why the kernels' LDS staging refuses this MpyrShape (the REC_MPYR_* limits of include/recengine.h)."""
    s = shape
    if min(s[:10]) < 1:
        return "every size must be positive"
    if s.filter_h > s.left_len or s.filter_w > s.right_len or s.pool_h > s.left_len or s.pool_w > s.right_len:
        return "filter and pool must fit the [%d, %d] image" % (s.left_len, s.right_len)
    PH, PW = mpyr_pooled_shape(s)
    for value, limit, name in ((s.left_len, MPYR_MAX_LEFT, "sentence_left_size"), (s.right_len, MPYR_MAX_RIGHT, "sentence_right_size"),
                               (s.emb_dim, MPYR_MAX_EMB, "emb_size"),
                               (s.filter_h * s.filter_w * ((s.channels + 7) // 8 * 8), MPYR_MAX_WEIGHTS, "filter area * kernel_num"),
                               (s.channels * PH * PW, MPYR_MAX_POOLED, "kernel_num * PH * PW"),
                               ((s.pool_h + s.filter_h - 1) * (s.right_len + s.filter_w - 1), MPYR_MAX_BAND,
                                "(pool_h + filter_h - 1) * (sentence_right_size + filter_w - 1)")):
        if value > limit:
            return "%s = %d above the kernels' %d" % (name, value, limit)
    return None


def _mpyr_args(shape, left, right, table, conv_w, conv_b, what):
    _chk(left, torch.int64, "left")
    _chk(right, torch.int64, "right")
    _chk(conv_w, torch.float32, "conv_w")
    _chk(conv_b, torch.float32, "conv_b")
    E, ldt = _chk_table(table, "table")
    B = left.shape[0]
    if tuple(left.shape) != (B, shape.left_len) or tuple(right.shape) != (B, shape.right_len) or E != shape.emb_dim:
        raise RecError("%s: left / right / table must be [B, %d] / [B, %d] / [V, %d]" % (what, shape.left_len, shape.right_len,
                                                                                         shape.emb_dim))
    if conv_w.numel() != shape.channels * shape.filter_h * shape.filter_w or conv_b.numel() != shape.channels:
        raise RecError("%s: conv_w / conv_b must hold K * kh * kw / K values" % what)
    return B, ldt, (C.c_int32 * _lib.REC_MPYR_SHAPE_LEN)(*[int(x) for x in shape])


def mpyr_fwd(shape, left, right, table, conv_w, conv_b, padding_idx=None, status=None, out=None):
    """rec_mpyr_fwd: left [B, Ll], right [B, Lr] int64, table [V, E] (row stride allowed) -> (pooled [B, K * PH * PW] float32,
    argmax int32 of that shape).  out: such a pair (row strides allowed), reused."""
    B, ldt, arr = _mpyr_args(shape, left, right, table, conv_w, conv_b, "mpyr_fwd")
    PH, PW = mpyr_pooled_shape(shape)
    N = shape.channels * max(PH, 0) * max(PW, 0)
    if out is None:
        out = (torch.empty(B, N, dtype=torch.float32, device=left.device), torch.empty(B, N, dtype=torch.int32, device=left.device))
    pooled, argmax = out
    ldp = _chk_mat(pooled, "pooled")
    if argmax.dtype != torch.int32 or argmax.dim() != 2 or (argmax.shape[1] > 1 and argmax.stride(1) != 1) \
            or tuple(pooled.shape) != (B, N) or tuple(argmax.shape) != (B, N):
        raise RecError("mpyr_fwd: pooled / argmax must be float32 / int32 [%d, %d]" % (B, N))
    lda = argmax.stride(0) if B > 1 else max(N, 1)
    check(lib().rec_mpyr_fwd(B, arr, table.shape[0], ldt, -1 if padding_idx is None else int(padding_idx), _p(left), _p(right),
                             _p(table), _p(conv_w), _p(conv_b), _p(pooled), ldp, _p(argmax), lda, _p(status), _stream()),
          "rec_mpyr_fwd")
    return pooled, argmax


def mpyr_bwd(shape, left, right, table, conv_w, conv_b, d_pooled, argmax, dL, dR, d_conv_w, d_conv_b, padding_idx=None,
             scratch=None):
    """rec_mpyr_bwd -> (dL [B * Ll, E], dR [B * Lr, E], d_conv_w, d_conv_b), all written in place (dL / dR may be row-strided
    views).  scratch: the dict of the two named intermediates (gated, partials) of an earlier call of this shape, reused."""
    B, ldt, arr = _mpyr_args(shape, left, right, table, conv_w, conv_b, "mpyr_bwd")
    PH, PW = mpyr_pooled_shape(shape)
    N, T = shape.channels * PH * PW, shape.channels * shape.filter_h * shape.filter_w
    lddp, lddl, lddr = _chk_mat(d_pooled, "d_pooled"), _chk_mat(dL, "dL"), _chk_mat(dR, "dR")
    _chk(d_conv_w, torch.float32, "d_conv_w")
    _chk(d_conv_b, torch.float32, "d_conv_b")
    if tuple(d_pooled.shape) != (B, N) or tuple(argmax.shape) != (B, N) or argmax.dtype != torch.int32:
        raise RecError("mpyr_bwd: d_pooled / argmax must be float32 / int32 [%d, %d]" % (B, N))
    if tuple(dL.shape) != (B * shape.left_len, shape.emb_dim) or tuple(dR.shape) != (B * shape.right_len, shape.emb_dim):
        raise RecError("mpyr_bwd: dL / dR must be [B * Ll, E] / [B * Lr, E]")
    if d_conv_w.numel() != T or d_conv_b.numel() != shape.channels:
        raise RecError("mpyr_bwd: d_conv_w / d_conv_b must hold K * kh * kw / K values")
    lda = argmax.stride(0) if B > 1 else max(N, 1)
    if scratch is None:
        scratch = {}
    if "gated" not in scratch or scratch["gated"].numel() < B * N or scratch["partials"].numel() < B * PH * (T + shape.channels):
        scratch["gated"] = torch.empty(max(B * N, 1), dtype=torch.float32, device=left.device)
        scratch["partials"] = torch.empty(max(B * PH * (T + shape.channels), 1), dtype=torch.float32, device=left.device)
    check(lib().rec_mpyr_bwd(B, arr, table.shape[0], ldt, -1 if padding_idx is None else int(padding_idx), _p(left), _p(right),
                             _p(table), _p(conv_w), _p(conv_b), _p(d_pooled), lddp, _p(argmax), lda, _p(scratch["gated"]),
                             _p(scratch["partials"]), _p(dL), lddl, _p(dR), lddr, _p(d_conv_w), _p(d_conv_b), _stream()),
          "rec_mpyr_bwd")
    return dL, dR, d_conv_w, d_conv_b


def mpyr_hinge(pred, pairs, out=None):
    """rec_mpyr_hinge: pred [B, 1] or [B] -> (loss [1], d_pred [B]); out: such a pair, reused."""
    _chk(pred, torch.float32, "pred")
    B = pred.numel()
    if out is None:
        out = (torch.empty(1, dtype=torch.float32, device=pred.device), torch.empty(B, dtype=torch.float32, device=pred.device))
    loss, d_pred = out
    _chk(loss, torch.float32, "loss", (1,))
    _chk(d_pred, torch.float32, "d_pred", (B,))
    check(lib().rec_mpyr_hinge(B, int(pairs), _p(pred), _p(loss), _p(d_pred), _stream()), "rec_mpyr_hinge")
    return loss, d_pred
