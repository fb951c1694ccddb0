"""NumPy restatement of the reference's word2vec (models/recall/word2vec/net.py:57-110, dygraph_model.py:53-76) in float64 or
float32 — TEST INFRASTRUCTURE ONLY.  The formulas are the reference's; an id outside the table follows the engine's rule
(include/recengine.h: the pair has logit 0, g 0 and no loss term)."""
import numpy as np

KEYS = ("embedding.weight", "embedding_w.weight", "embedding_b.weight")


def relerr(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-300) if ref.size else 0.0


def sgns(emb, emb_w, emb_b, in_ids, target_ids, grad_scale=1.0, dtype=np.float64):
    """-> dict(true_logits [B], neg_logits [B, neg], g [B, 1 + neg], d_in [B, D], loss [1]).  Sigmoid, THEN BCE on the
    probability: the log clamped at -100, the backward's denominator at 1e-12 (Paddle, as torch's binary_cross_entropy)."""
    f = dtype
    emb, emb_w, emb_b = (np.asarray(t, f) for t in (emb, emb_w, emb_b))
    V, D = emb.shape
    B, tw = target_ids.shape
    neg = tw - 1
    in_ok = (in_ids >= 0) & (in_ids < V)
    t_ok = (target_ids >= 0) & (target_ids < V)
    ok = in_ok[:, None] & t_ok
    x = np.where(in_ok[:, None], emb[np.where(in_ok, in_ids, 0)], f(0))                          # [B, D]
    w = np.where(t_ok[..., None], emb_w[np.where(t_ok, target_ids, 0)], f(0))                    # [B, tw, D]
    bias = emb_b.reshape(-1)[np.where(t_ok, target_ids, 0)]
    z = np.where(ok, (x[:, None, :] * w).sum(-1, dtype=f) + bias, f(0)).astype(f)
    y = np.zeros((B, tw), f)
    y[:, 0] = 1
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        p = (f(1) / (f(1) + np.exp(-z))).astype(f)
        term = -np.maximum(np.log(np.where(y == 1, p, f(1) - p)), f(-100))
        scale = np.empty((B, tw), f)
        scale[:, 0] = f(grad_scale) / f(B)
        scale[:, 1:] = f(grad_scale) / (f(B) * f(neg))
        g = (p - y) / np.maximum((f(1) - p) * p, f(1e-12)) * scale * (f(1) - p) * p
    term, g = np.where(ok, term, f(0)).astype(f), np.where(ok, g, f(0)).astype(f)
    loss = term[:, 0].sum(dtype=f) / f(B) + term[:, 1:].sum(dtype=f) / (f(B) * f(neg))
    d_in = (g[..., None] * w).sum(1, dtype=f)
    return dict(true_logits=z[:, 0].copy(), neg_logits=z[:, 1:].copy(), g=g, d_in=d_in.astype(f), loss=np.asarray([loss], f))


def target_rows(emb, in_ids, target_ids, g, dtype=np.float64):
    """The merged gradients of the target rows -> (rows [U] ascending, dw [U, D], db [U]); occurrences in ascending order."""
    f = dtype
    emb = np.asarray(emb, f)
    V, D = emb.shape
    flat = target_ids.reshape(-1)
    tw = target_ids.shape[1]
    rows = np.unique(flat[(flat >= 0) & (flat < V)])
    dw, db = np.zeros((len(rows), D), f), np.zeros(len(rows), f)
    gf = np.asarray(g, f).reshape(-1)
    for u, r in enumerate(rows):
        for pos in np.nonzero(flat == r)[0]:
            i = in_ids[pos // tw]
            if 0 <= i < V:
                dw[u] += gf[pos] * emb[i]
                db[u] += gf[pos]
    return rows, dw, db


def train_step(p, in_ids, target_ids, lr, dtype=np.float64):
    """One SGD step from the state_dict p -> (forward dict, dense gradients {key: array}, parameters after the step)."""
    f = dtype
    emb, emb_w, emb_b = (np.asarray(p[k], f) for k in KEYS)
    V = emb.shape[0]
    c = sgns(emb, emb_w, emb_b, in_ids, target_ids, 1.0, f)
    rows, dw, db = target_rows(emb, in_ids, target_ids, c["g"], f)
    grads = {k: np.zeros_like(np.asarray(p[k], f)) for k in KEYS}
    for b, i in enumerate(in_ids):
        if 0 <= i < V:
            grads[KEYS[0]][i] += c["d_in"][b]
    grads[KEYS[1]][rows] = dw
    grads[KEYS[2]][rows, 0] = db
    new = {k: (np.asarray(p[k], f) - f(lr) * grads[k]).astype(f) for k in KEYS}
    return c, grads, new


def scores(W, a, b, c, dtype=np.float64):
    """net.py:100-108: <W[b] - W[a] + W[c], W[v] / max(|W[v]|, 1e-12)> for every row v -> [Q, V]; the row is
    normalised first, as F.normalize does: a one-column table scores exactly +-target."""
    f = dtype
    W = np.asarray(W, f)
    target = W[b] - W[a] + W[c]
    norm = np.maximum(np.sqrt((W * W).sum(1, dtype=f)), f(1e-12)).astype(f)
    return (target @ (W / norm[:, None]).astype(f).T).astype(f)


def topk(s, k):
    """The k best of every row of s: higher score first, equal scores by the lower id -> (values [Q, k], ids [Q, k])."""
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), -s), axis=1)[:, :k]
    return np.take_along_axis(s, order, 1), order.astype(np.int64)


def separated(s64, k, gap=1e-4):
    """True when the k best float64 scores of every query are pairwise more than gap of the largest |score| apart."""
    v, _ = topk(s64, k)
    return bool((-(np.diff(v, axis=1)) > gap * np.abs(s64).max(1, keepdims=True)).all())


def load_golden(path):
    g = dict(np.load(path))
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0])
