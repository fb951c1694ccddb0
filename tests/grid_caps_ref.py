"""Plain numpy restatements for tests/test_grid_caps_gpu.py — TEST INFRASTRUCTURE ONLY.  Written from the comments of the
kernels in paddlerec_amd/csrc and the docstrings of ops.py; imports nothing from paddlerec_amd.  Where tests/*_ref.py or
oracle/ already states an operation (Adam, batch norm, the AUC buckets, the dropout mask, the dot interaction, CIN) the test
uses that statement; what is here had none.

Every function takes `dtype` (float64: the reference; float32: the restatement whose own error sets the tolerance).  Inputs
are the float32 arrays the kernel is given; a scalar the C entry point takes as `float` is rounded to float32 first."""
import numpy as np

from glue_ref import relerr, _a, _s                     # noqa: F401  (relerr is re-exported)


def ramped(rng, *shape, scale=1.0):
    """N(0, 1) scale plus a slow ramp over the FLAT index from 0.5 to 1.5: position-dependent, so a shifted or repeated index
    cannot cancel."""
    n = int(np.prod(shape))
    x = rng.standard_normal(n) * scale + np.linspace(0.5, 1.5, n)
    return x.astype(np.float32).reshape(shape)


def adagrad_dense(p, acc, g, lr, eps, dtype=np.float64):
    p, acc, g = _a(p, dtype), _a(acc, dtype), _a(g, dtype)
    acc = acc + g * g
    return p - _s(lr, dtype) * g / (np.sqrt(acc) + _s(eps, dtype)), acc


def l2_decay_grad(grad, w, coeff, grad_scale=None, dtype=np.float64):
    c = _s(coeff, dtype)
    if grad_scale is not None:
        c = c / _s(grad_scale, dtype)
    return _a(grad, dtype) + c * _a(w, dtype)


def softmax_rows(x, dtype=np.float64):
    x = _a(x, dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e * (dtype(1) / e.sum(axis=1, keepdims=True, dtype=dtype))


def softmax_rows_bwd(p, dp, dtype=np.float64):
    p, dp = _a(p, dtype), _a(dp, dtype)
    return p * (dp - (p * dp).sum(axis=1, keepdims=True, dtype=dtype))


def cross_bwd_prep(dX, X0, U, acc0, dtype=np.float64):
    """-> dU = dX X0, acc = (acc0 or 0) + dX U."""
    dX, X0, U = _a(dX, dtype), _a(X0, dtype), _a(U, dtype)
    a = dX * U
    return dX * X0, a if acc0 is None else _a(acc0, dtype) + a


def moe_bwd_prep(dX, X0, U, prob, acc0, dtype=np.float64):
    """-> dU = dX X0 p_e, acc = (acc0 or 0) + dX p_e U, dp = rowsum(dX X0 U)."""
    dX, X0, U, pe = _a(dX, dtype), _a(X0, dtype), _a(U, dtype), _a(prob, dtype).reshape(-1, 1)
    a = dX * pe * U
    return dX * X0 * pe, a if acc0 is None else _a(acc0, dtype) + a, (dX * X0 * U).sum(axis=1, dtype=dtype)


def sumsq(x, out0=None, dtype=np.float64):
    x = _a(x, dtype)
    s = (x * x).sum(dtype=dtype)
    return np.asarray([s if out0 is None else dtype(np.float32(out0)) + s])


def sigmoid_logloss(y1, y2, y3, label, eps, mean_over=0, dtype=np.float64):
    """-> pred, dz, loss of head_ops.hip's sigmoid_logloss_kernel (no clip): cost = -t log(p + eps) - (1 - t) log(1 - p + eps),
    dz = (-t / (p + eps) + (1 - t) / (1 - p + eps)) p (1 - p) / n."""
    z = _a(y1, dtype).reshape(-1) + _a(y2, dtype).reshape(-1) + _a(y3, dtype).reshape(-1)
    t, e, one = _a(label, dtype).reshape(-1), _s(eps, dtype), dtype(1)
    inv = one / dtype(mean_over if mean_over > 0 else z.size)
    p = one / (one + np.exp(-z))
    cost = -t * np.log(p + e) - (one - t) * np.log(one - p + e)
    dz = (-t / (p + e) + (one - t) / (one - p + e)) * inv * (p * (one - p))
    return p, dz, np.asarray([cost.sum(dtype=dtype) * inv])


def llrintf(x):
    """(int64) llrintf(x): round half to even; x float32 inside the int64 range."""
    return np.rint(np.asarray(x, np.float32).astype(np.float64)).astype(np.int64)
