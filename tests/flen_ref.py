"""NumPy restatement of the reference's rank/flen net (models/rank/flen/net.py, flen/dygraph_model.py) — TEST ORACLE.
Float64 by default (`dtype`): the field-wise bi-interaction forward / backward (what rec_flen_fwd / rec_flen_bwd compute),
paddle.optimizer.Adagrad (duplicates merged first) and the whole net with a hand-written backward.  p = the reference's
state_dict (keys below); ids [B, 23] are the reference's "sparse inputs", column 0 unused (net.py:67-69).

    E[b,s]  = table[ids[b, 1 + s]], s < S = 22;  X0 = [E_0 | .. | E_{S-1}]                                  net.py:67-79
    FW[b,g] = sum of E[b,s] over the slots of group g;  h_mf = sum_{i<j} kernel_mf[p] * FW_i * FW_j          net.py:205-229
    fwbi    = drop(BN(relu(h_mf @ Wf + bf)))                                                                 net.py:84-87
    dnn     = per layer: Linear, drop, ReLU, drop, BN, drop  (Dropout follows EVERY element)                 net.py:157-164
    pred    = sigmoid([fwbi | dnn] @ Wl + bl);  loss = mean binary_cross_entropy           net.py:89-95, dygraph_model.py:53-60
Train-mode dropout takes its keep-masks as inputs: `keeps` is a list of 3n + 1 boolean arrays in stream order — for DNN
layer i the two masks of the Linear/ReLU output (relu(drop(z)) = drop(relu(z)): applied together, scale 1/(1-p)^2) and the
mask behind its BN, then the mask of fwbi_drop.  keeps None = no dropout.
"""
import itertools

import numpy as np

EMB = "_EmbeddingLayer.embedding.weight"
KMF, KFM = "_FieldWiseBiInteraction.kernel_mf", "_FieldWiseBiInteraction.kernel_fm"
LIN, NORM = "_DNNLayer.linear_%d", "_DNNLayer.norm_%d"
FC, FBN, HEAD, HEAD_ALIAS = "fwbi_fc_32", "fwbi_bn", "linear", "linear_out"
BN_MOMENTUM, BN_EPS = 0.9, 1e-5
ADAGRAD_EPS, ADAGRAD_INIT = 1e-6, 1e-3
FIELD_SIZES = (13, 3, 6)


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def group_begin(field_sizes):
    return [0] + list(itertools.accumulate(int(x) for x in field_sizes))


def pairs(G):
    return list(itertools.combinations(range(G), 2))


# ---------------------------------------------------------------- the two operators
def lookup(ids, W, dtype=np.float64):
    """ids [B,S], W [N,>=D] -> (E [B,S,D] with zero rows for ids outside [0,N), live [B,S] bool)."""
    ids, W = np.asarray(ids), np.asarray(W, dtype)
    live = (ids >= 0) & (ids < W.shape[0])
    return W[np.where(live, ids, 0)] * live[..., None], live


def flen_forward(E, gb, kmf, dtype=np.float64):
    """E [B,S,D] -> (FW [B,G,D], h_mf [B,D])."""
    E, kmf = np.asarray(E, dtype), np.asarray(kmf, dtype).reshape(-1)
    G = len(gb) - 1
    FW = np.stack([E[:, gb[g]:gb[g + 1]].sum(axis=1, dtype=dtype) for g in range(G)], axis=1)
    h = np.zeros((E.shape[0], E.shape[2]), dtype)
    for p, (i, j) in enumerate(pairs(G)):
        h += kmf[p] * FW[:, i] * FW[:, j]
    return FW, h


def flen_backward(FW, gb, kmf, dH, dX0, live=None, dtype=np.float64):
    """dX0 [B,S,D] = d loss / d X0, dH [B,D] -> (row gradient [B,S,D], d kernel_mf [P])."""
    FW, dH, dX0 = np.asarray(FW, dtype), np.asarray(dH, dtype), np.asarray(dX0, dtype)
    kmf = np.asarray(kmf, dtype).reshape(-1)
    G = len(gb) - 1
    T = np.zeros_like(FW)
    dk = np.zeros(len(kmf), dtype)
    for p, (i, j) in enumerate(pairs(G)):
        T[:, i] += kmf[p] * FW[:, j]
        T[:, j] += kmf[p] * FW[:, i]
        dk[p] = (dH * FW[:, i] * FW[:, j]).sum(dtype=dtype)
    rg = dX0.copy()
    for g in range(G):
        rg[:, gb[g]:gb[g + 1]] += (dH * T[:, g])[:, None, :]
    if live is not None:
        rg = rg * np.asarray(live)[..., None]
    return rg, dk


def adagrad(p, acc, g, lr, eps=ADAGRAD_EPS):
    """paddle.optimizer.Adagrad in place on arrays of one dtype: acc += g*g; p -= lr * g / (sqrt(acc) + eps)."""
    acc += g * g
    p -= lr * g / (np.sqrt(acc) + eps)


def merged_rows(ids, row_grad, N):
    """SelectedRows merge: (unique live rows, the sum of their duplicate gradients [U,D])."""
    ids = np.asarray(ids).reshape(-1)
    g = np.asarray(row_grad).reshape(len(ids), -1)
    live = (ids >= 0) & (ids < N)
    uniq = np.unique(ids[live])
    out = np.zeros((len(uniq), g.shape[1]), g.dtype)
    np.add.at(out, np.searchsorted(uniq, ids[live]), g[live])
    return uniq, out


def adagrad_rows(P, A, ids, row_grad, lr, eps=ADAGRAD_EPS):
    """The rule on the MERGED gradient of the touched rows of P / A (in place): (sum g)^2, not sum g^2."""
    uniq, g = merged_rows(ids, row_grad, P.shape[0])
    D = g.shape[1]
    a, p = A[uniq, :D].copy(), P[uniq, :D].copy()
    adagrad(p, a, g.astype(P.dtype), lr, eps)
    A[uniq, :D], P[uniq, :D] = a, p


# ---------------------------------------------------------------- BatchNorm1D (Paddle: momentum 0.9, biased variance)
def bn_forward(x, gamma, beta, rmean, rvar, training):
    """-> (y, xhat, invstd, new running mean, new running variance)."""
    if training:
        mu, var = x.mean(axis=0), x.var(axis=0)
        rmean = BN_MOMENTUM * rmean + (1 - BN_MOMENTUM) * mu
        rvar = BN_MOMENTUM * rvar + (1 - BN_MOMENTUM) * var
    else:
        mu, var = rmean, rvar
    invstd = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (x - mu) * invstd
    return xhat * gamma + beta, xhat, invstd, rmean, rvar


def bn_backward(dy, xhat, invstd, gamma):
    """Train-mode backward -> (dx, dgamma, dbeta)."""
    dg, db = (dy * xhat).sum(axis=0), dy.sum(axis=0)
    m = dy.shape[0]
    return gamma * invstd * (dy - db / m - xhat * dg / m), dg, db


# ---------------------------------------------------------------- the whole net
def n_layers(p):
    return sum(1 for k in p if k.startswith("_DNNLayer.linear_") and k.endswith(".weight"))


def run(p, ids, label=None, field_sizes=FIELD_SIZES, training=False, keeps=None, rate=0.0, dtype=np.float64):
    """-> dict(pred [B,1], stats {key: new running statistic}) and, with a label [B,1], loss and grads {state_dict key:
    gradient} (the table's densified [N,D]; kernel_fm zeros; both aliases of the head)."""
    f = lambda k: np.asarray(p[k], dtype)
    ids = np.asarray(ids)[:, 1:]                                        # net.py:67-69: column 0 is never used
    B, S = ids.shape
    gb = group_begin(field_sizes)
    assert gb[-1] == S, "field_sizes must sum to the %d lookups" % S
    W = f(EMB)
    N, D = W.shape
    n = n_layers(p)
    sc = 1.0 / (1.0 - rate) if keeps is not None else 1.0
    keep = (lambda j: np.asarray(keeps[j], dtype)) if keeps is not None else (lambda j: 1.0)
    stats = {}

    def bn(name, x):
        y, xhat, invstd, rm, rv = bn_forward(x, f(name + ".weight"), f(name + ".bias"), f(name + "._mean"),
                                             f(name + "._variance"), training)
        stats[name + "._mean"], stats[name + "._variance"] = rm, rv
        return y, xhat, invstd

    E, _ = lookup(ids, W, dtype)
    FW, h = flen_forward(E, gb, f(KMF), dtype)
    x = E.reshape(B, S * D)
    cache = []
    for i in range(n):
        z = np.maximum(x @ f(LIN % i + ".weight") + f(LIN % i + ".bias"), 0.0)
        m1 = keep(3 * i) * keep(3 * i + 1) * sc * sc
        u = z * m1
        y, xhat, invstd = bn(NORM % i, u)
        m2 = keep(3 * i + 2) * sc
        cache.append((x, z, m1, xhat, invstd, m2))
        x = y * m2
    fz = np.maximum(h @ f(FC + ".weight") + f(FC + ".bias"), 0.0)
    fy, fxhat, finvstd = bn(FBN, fz)
    mf = keep(3 * n) * sc
    cat = np.concatenate([fy * mf, x], axis=1)
    logit = cat @ f(HEAD + ".weight") + f(HEAD + ".bias")
    out = dict(pred=sigmoid(logit), stats=stats, X0=E.reshape(B, S * D), h_mf=h, FW=FW)
    if label is None:
        return out
    t = np.asarray(label, dtype).reshape(B, 1)
    out["loss"] = (np.maximum(logit, 0) - logit * t + np.log1p(np.exp(-np.abs(logit)))).mean()
    g = {}
    dlogit = (out["pred"] - t) / B
    g[HEAD + ".weight"], g[HEAD + ".bias"] = cat.T @ dlogit, dlogit.sum(axis=0)
    g[HEAD_ALIAS + ".weight"], g[HEAD_ALIAS + ".bias"] = g[HEAD + ".weight"], g[HEAD + ".bias"]
    dcat = dlogit @ f(HEAD + ".weight").T
    dfz, g[FBN + ".weight"], g[FBN + ".bias"] = bn_backward(dcat[:, :D] * mf, fxhat, finvstd, f(FBN + ".weight"))
    dfz = dfz * (fz > 0)
    g[FC + ".weight"], g[FC + ".bias"] = h.T @ dfz, dfz.sum(axis=0)
    dH = dfz @ f(FC + ".weight").T
    dx = dcat[:, D:]
    for i in reversed(range(n)):
        xin, z, m1, xhat, invstd, m2 = cache[i]
        du, g[NORM % i + ".weight"], g[NORM % i + ".bias"] = bn_backward(dx * m2, xhat, invstd, f(NORM % i + ".weight"))
        dz = du * m1 * (z > 0)
        g[LIN % i + ".weight"], g[LIN % i + ".bias"] = xin.T @ dz, dz.sum(axis=0)
        dx = dz @ f(LIN % i + ".weight").T
    rg, g[KMF] = flen_backward(FW, gb, f(KMF), dH, dx.reshape(B, S, D), dtype=dtype)
    g[KMF] = g[KMF].reshape(np.asarray(p[KMF]).shape)
    g[KFM] = np.zeros(np.asarray(p[KFM]).shape, dtype)                  # net.py:234-257: dead code
    dW = np.zeros((N, D), dtype)
    np.add.at(dW, ids.reshape(-1), rg.reshape(B * S, D))
    g[EMB] = dW
    out.update(grads=g, row_grad=rg, dH=dH, dX0=dx)
    return out


def trainable(p):
    """The keys the optimizer walks: every parameter once (the running statistics are buffers, linear_out an alias)."""
    return [k for k in p if not (k.endswith("._mean") or k.endswith("._variance") or k.startswith(HEAD_ALIAS + "."))]


def train_step(p, acc, ids, label, lr, field_sizes=FIELD_SIZES, keeps=None, rate=0.0, dtype=np.float64):
    """One step in place on p (arrays of `dtype`) and the Adagrad accumulators acc {key: array}.  -> run()'s dict."""
    out = run(p, ids, label, field_sizes, True, keeps, rate, dtype)
    for k, v in out["stats"].items():
        p[k][...] = v
    for k in trainable(p):
        if k == EMB:
            adagrad_rows(p[k], acc[k], np.asarray(ids)[:, 1:], out["row_grad"], lr)
        else:
            adagrad(p[k], acc[k], out["grads"][k].reshape(p[k].shape), lr)
    for nm in (".weight", ".bias"):
        if HEAD_ALIAS + nm in p:
            p[HEAD_ALIAS + nm] = p[HEAD + nm]
    return out


def new_accumulators(p, dtype=np.float64):
    return {k: np.full(np.asarray(p[k]).shape, ADAGRAD_INIT, dtype) for k in trainable(p)}
