"""Stand-in for paddlerec_amd.ops on CPU tensors for the host logic of paddlerec_amd/aitm.py — TEST INFRASTRUCTURE ONLY.

Everything tests/mtl_cpu_kernels.py has, Dropout, the L2 term and the non-lazy row Adam with L2 of tests/cpu_kernels.py and
tests/deepfefm_cpu_kernels.py, and the new ops: rec_field_gather_fwd, rec_ait_fwd / _bwd, rec_aitm_head and
rec_auc_histogram_wide evaluate the formulas of tests/aitm_ref.py in float32, writing through the same strided views the
device kernels write through.  The id grouping drops a row outside [0, num_rows) as rec_ids_group does (the gather's -1 for
a refused id), which tests/cpu_kernels.py's does not.  The product never imports this module."""
import numpy as np
import torch

import aitm_ref as A
from cpu_kernels import IdGroups, dropout, l2_decay_grad, segment_partials  # noqa: F401
from deepfefm_cpu_kernels import adam_rows_all  # noqa: F401
from mtl_cpu_kernels import *  # noqa: F401,F403
from mtl_cpu_kernels import _n, _t
from oracle import deepfm_ref as R

F32 = np.float32


def ids_group(ids, num_rows, padding_idx, ws, slot_offset=None, status=None, groups=None, payload=None):
    rows = _n(ids).reshape(-1)
    valid = (rows >= 0) & (rows < num_rows)
    if padding_idx is not None:
        valid &= rows != padding_idx
    if status is not None and ((rows < 0) | (rows >= num_rows)).any():
        status |= 1
    groups.spos, groups.uniq, groups.offs = R.group_ids(rows, valid)
    return groups, status


def field_gather_fwd(ids, W, field_begin, out=None, rows_out=None, status=None):
    o, rows, flagged = A.gather(_n(W), _n(field_begin), _n(ids), dtype=F32)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32)
    if flagged:
        status |= 1
    o, rows = _t(o), torch.from_numpy(rows.astype(np.int64))
    return (o if out is None else out.copy_(o)), (rows if rows_out is None else rows_out.copy_(rows)), status


def ait_fwd(QKV, tokens, out=None, prob=None):
    o, p = A.ait_fwd(_n(QKV), tokens, dtype=F32)
    o, p = _t(o), _t(p)
    return (o if out is None else out.copy_(o)), (p if prob is None else prob.copy_(p))


def ait_bwd(QKV, prob, d_out, tokens, out=None):
    r = _t(A.ait_bwd(_n(QKV), _n(prob), _n(d_out), tokens, dtype=F32))
    return r if out is None else out.copy_(r)


def aitm_head(tower_click, ait, w_click, b_click, w_conv, b_conv, click, buy, constraint_w=0.6, grad_scale=1.0, want_grad=True):
    pred, cost, dz = A.head(_n(tower_click), _n(ait), _n(w_click), _n(b_click), _n(w_conv), _n(b_conv), click.numpy(),
                            buy.numpy(), F32(constraint_w), F32(grad_scale), dtype=F32)
    return _t(pred), _t(cost), (_t(dz) if want_grad else None)


def auc_histogram_wide(pred, label, stat_pos, stat_neg, num_thresholds=100000):
    pos, neg = A.auc_histogram(pred.numpy(), label.numpy(), num_thresholds)
    stat_pos += torch.from_numpy(pos)
    stat_neg += torch.from_numpy(neg)
