"""NumPy restatement of the reference's rank/ffm net (models/rank/ffm/net.py, ffm/dygraph_model.py) — TEST ORACLE.

Everything is computed in float64; callers cast.  p = {"W" [N, >= R], "W1" [N,1], "dense_w" [1,Dn,R] | [Dn,R],
"dense_w_one" [Dn], "bias" [1]} with R = F * D, F = S + Dn (dygraph_model.py:31-32).  W may be wider than R (the
engine's padded table): only its first R columns are read.
"""
import numpy as np

LOG_EPS = 1e-4                       # paddle.nn.functional.log_loss default epsilon


def cube(ids, dense, W, dense_w, D):
    """feat_embeddings reshaped to [B, F, F, D]                                        net.py:110-120"""
    B, S = ids.shape
    Dn = dense.shape[1]
    R = (S + Dn) * D
    sparse = np.asarray(W, np.float64)[:, :R][ids]                                   # net.py:111
    dense_e = np.asarray(dense, np.float64)[:, :, None] * np.asarray(dense_w, np.float64).reshape(1, Dn, R)  # :112-113
    E = np.concatenate([sparse, dense_e], axis=1)                                    # net.py:114-115 [B, F, R]
    return E.reshape(B, S + Dn, S + Dn, D)                                           # net.py:117-120


def forward(ids, dense, p, D):
    """-> (y1 [B,1], y2 [B,1])."""
    B, S = ids.shape
    y1 = np.asarray(p["W1"], np.float64)[ids, 0].sum(1, keepdims=True) + \
        (np.asarray(dense, np.float64) * np.asarray(p["dense_w_one"], np.float64)).sum(1, keepdims=True)  # :101-108
    E = cube(ids, dense, p["W"], p["dense_w"], D)
    F = E.shape[1]
    prod = np.einsum("bijd,bjid->bij", E, E)                                         # <E[i,j,:], E[j,i,:]>
    iu = np.triu_indices(F, 1)
    y2 = prod[:, iu[0], iu[1]].sum(1, keepdims=True)                                 # net.py:121-132 (i < j)
    return y1, y2


def backward(ids, dense, p, D, dz, grad_stride=None):
    """dz [B] = dloss / dlogit -> (row_grad [B*S, grad_stride or R] in position order, d_dense_w [Dn,R],
    d_dense_w_one [Dn]).  dE[i,j,:] = dz * E[j,i,:] (j != i), dE[i,i,:] = 0."""
    B, S = ids.shape
    Dn = dense.shape[1]
    E = cube(ids, dense, p["W"], p["dense_w"], D)
    F = E.shape[1]
    R = F * D
    dz = np.asarray(dz, np.float64).reshape(B)
    dE = np.swapaxes(E, 1, 2) * dz[:, None, None, None]
    dE[:, np.arange(F), np.arange(F), :] = 0.0
    dE = dE.reshape(B, F, R)
    gs = grad_stride or R
    row_grad = np.zeros((B * S, gs))
    row_grad[:, :R] = dE[:, :S].reshape(B * S, R)
    dd = np.asarray(dense, np.float64)
    d_dense_w = np.einsum("bk,bkc->kc", dd, dE[:, S:])
    d_dense_w_one = (dz[:, None] * dd).sum(0)
    return row_grad, d_dense_w, d_dense_w_one


def loss_and_grads(ids, dense, label, p, D):
    """Forward + mean log_loss (dygraph_model.py:50-55) + backward.  rows / row_valid are the flattened lookups
    (every id is a trained row: no padding_idx, net.py:59-75)."""
    B, S = ids.shape
    y1, y2 = forward(ids, dense, p, D)
    z = y1 + y2 + np.asarray(p["bias"], np.float64).reshape(1, 1)
    pred = 1.0 / (1.0 + np.exp(-z))
    t = np.asarray(label, np.float64).reshape(B, 1)
    cost = -t * np.log(pred + LOG_EPS) - (1 - t) * np.log(1 - pred + LOG_EPS)
    dz = ((-t / (pred + LOG_EPS) + (1 - t) / (1 - pred + LOG_EPS)) / B) * (pred * (1 - pred))
    row_grad, d_dense_w, d_dense_w_one = backward(ids, dense, p, D, dz)
    return dict(y1=y1, y2=y2, pred=pred, loss=cost.mean(), dz=dz.reshape(B),
                rows=ids.reshape(-1), row_valid=np.ones(B * S, bool), row_grad=row_grad,
                row_grad1=np.repeat(dz.reshape(B), S).reshape(B * S, 1),
                d_dense_w=d_dense_w, d_dense_w_one=d_dense_w_one, d_bias=dz.sum(keepdims=True).reshape(1))
