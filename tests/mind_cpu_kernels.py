"""Stand-in for paddlerec_amd.ops on CPU tensors for the host logic of paddlerec_amd/mind.py — TEST INFRASTRUCTURE ONLY.

Everything tests/aitm_cpu_kernels.py has (GEMM and its epilogues, the gather, the id grouping that drops a row outside
[0, num_rows), the segment partials, the non-lazy row Adam, the dense Adam), the ReLU mask, and the new ops:
rec_mind_routing_fwd / _bwd, rec_mind_label_attn_fwd / _bwd and rec_mind_ssm_head evaluate the formulas of tests/mind_ref.py
in float32, writing through the same strided views the device kernels write through.  The product never imports this
module."""
import numpy as np
import torch

import mind_ref as M
from aitm_cpu_kernels import *  # noqa: F401,F403
from cpu_kernels import emb_gather  # noqa: F401
from gatenet_cpu_kernels import relu_mask_  # noqa: F401
from mtl_cpu_kernels import _n, _t

F32 = np.float32


def mind_routing_fwd(low, seq_len, routing_logits, iters):
    K, T = routing_logits.shape[-2:]
    x = _n(low)
    W, Z, caps = M.routing_fwd(x.reshape(-1, T, x.shape[1]), seq_len.numpy(), _n(routing_logits).reshape(K, T), iters, F32)
    return _t(W), _t(Z), _t(caps)


def mind_routing_bwd(d_caps, Z, W, out=None):
    B, K, H = Z.shape
    r = _t(M.routing_bwd(_n(d_caps).reshape(B, K, H), _n(Z), _n(W), F32).reshape(-1, H))
    return r if out is None else out.copy_(r)


def mind_label_attn_fwd(caps2, target, k_max, pow_p=1.0):
    x = _n(caps2)
    user, attn = M.label_attn_fwd(x.reshape(-1, k_max, x.shape[1]), _n(target), pow_p, F32)
    return _t(user), _t(attn)


def mind_label_attn_bwd(caps2, target, attn, d_user, pow_p=1.0, d_target=None):
    x = _n(caps2)
    K = attn.shape[1]
    dx, dq = M.label_attn_bwd(x.reshape(-1, K, x.shape[1]), _n(target), _n(attn), _n(d_user), pow_p, F32)
    dq = _t(dq)
    return _t(dx.reshape(x.shape)), (dq if d_target is None else d_target.copy_(dq))


def mind_ssm_head(user, true_w, true_b, S, sample_b, labels, neg, logq_true, logq_neg, grad_scale=1.0, d_true_w=None,
                  d_user0=None):
    with np.errstate(invalid="ignore", over="ignore"):
        loss, dS, d_true = M.ssm_head(_n(user), _n(true_w), _n(true_b), _n(S), _n(sample_b), labels.numpy(), neg.numpy(),
                                      _n(logq_true), _n(logq_neg), F32(grad_scale), F32)
    S.copy_(_t(dS))
    if d_true_w is not None:
        d_true_w.copy_(_t(d_true[:, None] * _n(user)))
    if d_user0 is not None:
        d_user0.copy_(_t(d_true[:, None] * _n(true_w)))
    return _t(loss), _t(d_true), S
