"""NumPy restatement of the reference's rank/autofis net (models/rank/autofis/net.py, optimizer.py, dygraph_model.py) —
TEST ORACLE.  Float64 by default (`dtype`): the gated pair term forward / backward (what rec_autofis_fwd / rec_autofis_bwd
compute), BatchNorm -> ReLU, SimpleGrda, non-lazy Adam, and the whole net with a hand-written backward.  p = the
reference's state_dict (keys below); ids [B, S].

    xw = w_embeddings(ids) [B,S];  xv = v_embeddings(ids) [B,S,D]                                      net.py:78-80
    h  = xv.flatten(1) through depth x (Linear, BatchNorm, ReLU), then Linear(width -> 1)             net.py:82-89
    L[b,p] = <xv[b,c_p], xv[b,r_p]> over the pairs (c_p < r_p) kept by comb_mask                       net.py:91-96
    fm = (bn2(L) * mask).sum(-1);  pred = sigmoid(xw.sum(1) + fm + h)                                  net.py:97-101
    loss = mean binary_cross_entropy(pred, label)                                            dygraph_model.py:46-48
"""
import itertools
import math

import numpy as np

MASK, WEMB, VEMB = "mask", "w_embeddings.weight", "v_embeddings.weight"
LIN, BN, BN2 = "linear.%d", "bn.%d", "bn2"
BN_MOMENTUM, BN_EPS = 0.9, 1e-5


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def all_pairs(S):
    return list(itertools.combinations(range(S), 2))


def generate_pairs(S, comb_mask=None):
    """net.py:29-38 -> (cols, rows) of the pairs kept by comb_mask (None: all of them), in combinations order."""
    kept = [pr for i, pr in enumerate(all_pairs(S)) if comb_mask is None or int(comb_mask[i]) == 1]
    return [a for a, _ in kept], [b for _, b in kept]


def lookup(ids, W, dtype=np.float64):
    """ids [B,S], W [N,D] -> (E [B,S,D] with zero rows for ids outside [0,N), live [B,S] bool)."""
    ids, W = np.asarray(ids), np.asarray(W, dtype)
    live = (ids >= 0) & (ids < W.shape[0])
    return W[np.where(live, ids, 0)] * live[..., None], live


# ---------------------------------------------------------------- BatchNorm (Paddle: biased variance everywhere)
def bn_stats(X, eps=BN_EPS):
    mean = X.mean(axis=0)
    var = ((X - mean) ** 2).mean(axis=0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def bn_relu_forward(X, gamma, beta, dtype=np.float64):
    X = np.asarray(X, dtype)
    mean, var, invstd = bn_stats(X)
    return np.maximum((X - mean) * invstd * np.asarray(gamma, dtype) + np.asarray(beta, dtype), 0), mean, var, invstd


def bn_relu_backward(X, Y, dY, gamma, mean, invstd, dtype=np.float64):
    """-> (dX, dgamma, dbeta) of Y = relu(BN(X))."""
    X, dY, gamma = np.asarray(X, dtype), np.asarray(dY, dtype), np.asarray(gamma, dtype)
    dY = dY * (np.asarray(Y) > 0)
    xhat = (X - mean) * invstd
    dbeta, dgamma = dY.sum(axis=0), (dY * xhat).sum(axis=0)
    m = X.shape[0]
    return gamma * invstd * (dY - dbeta / m - xhat * dgamma / m), dgamma, dbeta


# ---------------------------------------------------------------- the pair term
def pair_forward(xv, xw, cols, rows, gamma, beta, mask, mean=None, var=None, dtype=np.float64):
    """xv [B,S,D], xw [B,S] -> (s [B] = sum_s xw + sum_p mask_p BN_p(L), L [B,P], mean, var, invstd).
    mean / var given: eval mode on those statistics; None: batch statistics."""
    xv, xw = np.asarray(xv, dtype), np.asarray(xw, dtype)
    gamma, beta, mask = (np.asarray(t, dtype).reshape(-1) for t in (gamma, beta, mask))
    L = (xv[:, cols] * xv[:, rows]).sum(axis=-1)
    if mean is None:
        mean, var, invstd = bn_stats(L)
    else:
        mean, var = np.asarray(mean, dtype), np.asarray(var, dtype)
        invstd = 1.0 / np.sqrt(var + BN_EPS)
    y = (L - mean) * invstd * gamma + beta
    return xw.sum(axis=1) + (y * mask).sum(axis=1), L, mean, var, invstd


def pair_backward(xv, L, dz, cols, rows, gamma, beta, mask, mean, invstd, dtype=np.float64):
    """dz [B] = dloss / d s -> (dxv [B,S,D] (the pair term's part), d_mask, d_gamma, d_beta [P])."""
    xv, L, dz = np.asarray(xv, dtype), np.asarray(L, dtype), np.asarray(dz, dtype).reshape(-1)
    gamma, beta, mask = (np.asarray(t, dtype).reshape(-1) for t in (gamma, beta, mask))
    B = max(len(dz), 1)
    xhat = (L - mean) * invstd
    S0 = dz.sum()
    S1 = (dz[:, None] * xhat).sum(axis=0)
    d_mask, d_gamma, d_beta = gamma * S1 + beta * S0, mask * S1, mask * S0
    dL = gamma * invstd * mask * (dz[:, None] - S0 / B - xhat * S1 / B)
    dxv = np.zeros_like(xv)
    for p, (c, r) in enumerate(zip(cols, rows)):
        dxv[:, c] += dL[:, p:p + 1] * xv[:, r]
        dxv[:, r] += dL[:, p:p + 1] * xv[:, c]
    return dxv, d_mask, d_gamma, d_beta


def pair_forward_f32_sequential(xv, xw, cols, rows, gamma, beta, mask):
    """The training pair_forward in strictly sequential float32 (every sum a left-to-right loop in float32): the rounding
    any float32 implementation is allowed.  -> (s, L, mean, invstd)."""
    f = np.float32
    xv, xw = np.asarray(xv, f), np.asarray(xw, f)
    B, _, D = xv.shape
    P = len(cols)
    L = np.zeros((B, P), f)
    for d in range(D):
        L = (L + xv[:, cols, d] * xv[:, rows, d]).astype(f)
    mean = np.zeros(P, f)
    for b in range(B):
        mean = (mean + L[b]).astype(f)
    mean = (mean / f(B)).astype(f)
    var = np.zeros(P, f)
    for b in range(B):
        var = (var + (L[b] - mean) * (L[b] - mean)).astype(f)
    var = (var / f(B)).astype(f)
    invstd = (f(1) / np.sqrt(var + f(BN_EPS))).astype(f)
    y = ((L - mean) * invstd * np.asarray(gamma, f) + np.asarray(beta, f)).astype(f) * np.asarray(mask, f)
    s = np.zeros(B, f)
    for t in range(xw.shape[1]):
        s = (s + xw[:, t]).astype(f)
    for p in range(P):
        s = (s + y[:, p]).astype(f)
    return s, L, mean, invstd


# ---------------------------------------------------------------- optimizers
class Grda:
    """optimizer.py:19-60 on one parameter.  acc: the accumulator (the reference draws it U(-0.1, 0.1))."""

    def __init__(self, acc, lr=1.0, c=0.0, mu=0.7):
        self.acc, self.lr, self.c, self.mu = np.array(acc, copy=True), lr, c, mu
        self.iterations, self.l1_accumulation = 0, 0.0

    def step(self, p, g):
        """-> the new p."""
        c, mu, lr = self.c, self.mu, self.lr
        self.l1_accumulation += c * math.pow(lr, 0.5 + mu) * math.pow(self.iterations + 1.0, mu) \
            - c * math.pow(lr, 0.5 + mu) * math.pow(self.iterations + 0.0, mu)
        first_iter = max(1 - self.iterations, 0)
        self.acc = self.acc + first_iter * p - lr * g
        self.iterations += 1
        return np.sign(self.acc) * np.clip(np.abs(self.acc) - self.l1_accumulation, 0, None)


def adam(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """paddle.optimizer.Adam on EVERY element (lazy_mode=False: rows without a gradient move with g = 0), in place."""
    m[...] = beta1 * m + (1 - beta1) * g
    v[...] = beta2 * v + (1 - beta2) * g * g
    lr_t = lr * math.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    p[...] = p - lr_t * m / (np.sqrt(v) + eps * math.sqrt(1 - beta2 ** t))


# ---------------------------------------------------------------- the whole net
def depth_of(p):
    return sum(1 for k in p if k.startswith("bn.") and k.endswith(".weight"))


def forward(p, ids, comb_mask=None, training=True, dtype=np.float64):
    """-> (pred [B], cache).  training: batch statistics (cache["rs"] = the running statistics after the step)."""
    P = {k: np.asarray(v, dtype) for k, v in p.items()}
    ids = np.asarray(ids)
    S = ids.shape[1]
    cols, rows = generate_pairs(S, comb_mask)
    xv, live = lookup(ids, P[VEMB], dtype)
    xw, _ = lookup(ids, P[WEMB], dtype)
    xw = xw[..., 0]
    n = depth_of(p)
    h, layers, rs = xv.reshape(len(ids), -1), [], {}
    for i in range(n):
        z = h @ P[LIN % i + ".weight"] + P[LIN % i + ".bias"]
        if training:
            y, mean, var, invstd = bn_relu_forward(z, P[BN % i + ".weight"], P[BN % i + ".bias"], dtype)
            rs[BN % i + "._mean"] = BN_MOMENTUM * P[BN % i + "._mean"] + (1 - BN_MOMENTUM) * mean
            rs[BN % i + "._variance"] = BN_MOMENTUM * P[BN % i + "._variance"] + (1 - BN_MOMENTUM) * var
        else:
            mean, invstd = P[BN % i + "._mean"], 1.0 / np.sqrt(P[BN % i + "._variance"] + BN_EPS)
            y = np.maximum((z - mean) * invstd * P[BN % i + ".weight"] + P[BN % i + ".bias"], 0)
        layers.append((h, z, y, mean, invstd))
        h = y
    hd = (h @ P[LIN % n + ".weight"] + P[LIN % n + ".bias"])[:, 0]
    if training:
        s, L, mean, var, invstd = pair_forward(xv, xw, cols, rows, P[BN2 + ".weight"], P[BN2 + ".bias"], P[MASK],
                                               dtype=dtype)
        rs[BN2 + "._mean"] = BN_MOMENTUM * P[BN2 + "._mean"] + (1 - BN_MOMENTUM) * mean
        rs[BN2 + "._variance"] = BN_MOMENTUM * P[BN2 + "._variance"] + (1 - BN_MOMENTUM) * var
    else:
        s, L, mean, var, invstd = pair_forward(xv, xw, cols, rows, P[BN2 + ".weight"], P[BN2 + ".bias"], P[MASK],
                                               P[BN2 + "._mean"], P[BN2 + "._variance"], dtype=dtype)
    pred = sigmoid(s + hd)
    return pred, dict(P=P, ids=ids, cols=cols, rows=rows, xv=xv, live=live, layers=layers, h=h, L=L, mean=mean,
                      invstd=invstd, rs=rs, n=n)


def loss_of(pred, label):
    y = np.asarray(label, pred.dtype).reshape(-1)
    return -(y * np.maximum(np.log(pred), -100.0) + (1 - y) * np.maximum(np.log(1 - pred), -100.0)).mean()


def log_loss(pred, label, eps=1e-4):
    """paddle.nn.functional.log_loss(pred, label).mean() (metrics.py:26)."""
    y = np.asarray(label, pred.dtype).reshape(-1)
    return (-y * np.log(pred + eps) - (1 - y) * np.log(1 - pred + eps)).mean()


def backward(pred, label, c):
    """-> {name: gradient} of the mean BCE for every parameter (the tables' densified) plus "dz" and "dX0"."""
    P, n, ids = c["P"], c["n"], c["ids"]
    B, S = ids.shape
    y = np.asarray(label, pred.dtype).reshape(-1)
    dz = (pred - y) / B
    g = {}
    g[LIN % n + ".weight"] = c["h"].T @ dz[:, None]
    g[LIN % n + ".bias"] = dz.sum(keepdims=True)
    dh = dz[:, None] @ P[LIN % n + ".weight"].T
    for i in reversed(range(n)):
        x, z, yv, mean, invstd = c["layers"][i]
        dzi, g[BN % i + ".weight"], g[BN % i + ".bias"] = bn_relu_backward(z, yv, dh, P[BN % i + ".weight"], mean, invstd,
                                                                          pred.dtype)
        g[LIN % i + ".weight"] = x.T @ dzi
        g[LIN % i + ".bias"] = dzi.sum(axis=0)
        dh = dzi @ P[LIN % i + ".weight"].T
    dxv, d_mask, g[BN2 + ".weight"], g[BN2 + ".bias"] = pair_backward(
        c["xv"], c["L"], dz, c["cols"], c["rows"], P[BN2 + ".weight"], P[BN2 + ".bias"], P[MASK], c["mean"], c["invstd"],
        pred.dtype)
    g[MASK] = d_mask.reshape(P[MASK].shape)
    dX0 = dh.reshape(c["xv"].shape) + dxv
    gv, gw = np.zeros_like(P[VEMB]), np.zeros_like(P[WEMB])
    np.add.at(gv, ids[c["live"]], dX0[c["live"]])
    np.add.at(gw, ids[c["live"]], np.broadcast_to(dz[:, None, None], (B, S, 1))[c["live"]])
    g[VEMB], g[WEMB], g["dz"], g["dX0"] = gv, gw, dz, dX0
    return g
