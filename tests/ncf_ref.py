"""numpy restatement of the reference's NCF (models/recall/ncf/net.py, dygraph_model.py, evaluate.py) — TEST INFRASTRUCTURE
ONLY: the three nets, the log loss, their gradients (tables dense), Paddle's Adam and evaluate.py's metric, in the dtype
asked for (float64: the yardstick; float32: what float32 arithmetic alone costs, the tolerance's unit).

Parameters are a dict under the reference's names: MF_Embedding_User.weight [U, mf], MF_Embedding_Item.weight, MLP_Embedding_
User.weight [U, layers[0] / 2], MLP_Embedding_Item.weight, layer_i.weight [in, out], layer_i.bias, prediction.weight [w, 1],
prediction.bias.  The mode follows from the names present: GMF has no MLP tables and no tower, MLP has no MF tables."""
import math

import numpy as np

EPS_LOSS, B1, B2, EPS_ADAM = 1e-4, 0.9, 0.999, 1e-8


def relerr(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(float(np.abs(want).max()), 1e-30))


def n_fc(p):
    n = 0
    while "layer_%d.weight" % (n + 1) in p:
        n += 1
    return n


def forward(p, users, items, dt=np.float64):
    """-> dict(pred [B], and what the backward needs)."""
    p = {k: np.asarray(v, dt) for k, v in p.items()}
    u, i = np.asarray(users).reshape(-1), np.asarray(items).reshape(-1)
    c = dict(u=u, i=i, acts=[])
    parts = []
    if "MF_Embedding_User.weight" in p:
        c["mfu"], c["mfi"] = p["MF_Embedding_User.weight"][u], p["MF_Embedding_Item.weight"][i]
        parts.append(c["mfu"] * c["mfi"])
    n = n_fc(p)
    if n:
        x = np.concatenate([p["MLP_Embedding_User.weight"][u], p["MLP_Embedding_Item.weight"][i]], 1)
        for l in range(1, n + 1):
            c["acts"].append(x)
            x = np.maximum(x @ p["layer_%d.weight" % l] + p["layer_%d.bias" % l], dt(0))
        parts.append(x)
    c["pin"] = np.concatenate(parts, 1)
    z = c["pin"] @ p["prediction.weight"].reshape(-1) + p["prediction.bias"][0]
    c["pred"] = (dt(1) / (dt(1) + np.exp(-z))).astype(dt)
    return c


def loss_and_grads(p, users, items, labels, dt=np.float64, mean_over=0):
    """mean(log_loss(pred, label, 1e-4)) over mean_over (0 -> B) -> (loss, pred, {name: gradient}); tables dense."""
    p = {k: np.asarray(v, dt) for k, v in p.items()}
    c = forward(p, users, items, dt)
    y, pr, eps = np.asarray(labels).reshape(-1).astype(dt), c["pred"], dt(EPS_LOSS)
    inv = dt(1) / dt(mean_over or len(y))
    loss = (-y * np.log(pr + eps) - (dt(1) - y) * np.log(dt(1) - pr + eps)).sum(dtype=dt) * inv
    dz = (-y / (pr + eps) + (dt(1) - y) / (dt(1) - pr + eps)) * inv * (pr * (dt(1) - pr))
    g = {"prediction.weight": (c["pin"].T @ dz).reshape(-1, 1), "prediction.bias": dz.sum(dtype=dt).reshape(1)}
    dpin = dz[:, None] * p["prediction.weight"].reshape(1, -1)
    mf = p["MF_Embedding_User.weight"].shape[1] if "MF_Embedding_User.weight" in p else 0

    def scatter(name, ids, rows):
        out = np.zeros_like(p[name])
        np.add.at(out, ids, rows)
        g[name] = out

    if mf:
        scatter("MF_Embedding_User.weight", c["u"], dpin[:, :mf] * c["mfi"])
        scatter("MF_Embedding_Item.weight", c["i"], dpin[:, :mf] * c["mfu"])
    n = n_fc(p)
    if n:
        d = dpin[:, mf:] * (c["pin"][:, mf:] > 0)
        for l in range(n, 0, -1):
            x = c["acts"][l - 1]
            g["layer_%d.weight" % l], g["layer_%d.bias" % l] = x.T @ d, d.sum(0, dtype=dt)
            d = d @ p["layer_%d.weight" % l].T
            if l > 1:
                d = d * (x > 0)
        half = d.shape[1] // 2
        scatter("MLP_Embedding_User.weight", c["u"], d[:, :half])
        scatter("MLP_Embedding_Item.weight", c["i"], d[:, half:])
    return dt(loss), pr, g


def adam(p, g, m, v, step, lr, dt=np.float64):
    """paddle.optimizer.Adam, dygraph default (not lazy): every element of every parameter moves.  step is 1-based."""
    newp, newm, newv = {}, {}, {}
    b1, b2, eps = dt(B1), dt(B2), dt(EPS_ADAM)
    lr_t = dt(lr) * np.sqrt(dt(1) - b2 ** dt(step)) / (dt(1) - b1 ** dt(step))
    for k in p:
        gk = np.asarray(g[k], dt).reshape(np.shape(p[k]))
        newm[k] = b1 * np.asarray(m[k], dt) + (dt(1) - b1) * gk
        newv[k] = b2 * np.asarray(v[k], dt) + (dt(1) - b2) * gk * gk
        newp[k] = np.asarray(p[k], dt) - lr_t * newm[k] / (np.sqrt(newv[k]) + eps * np.sqrt(dt(1) - b2 ** dt(step)))
    return newp, newm, newv


def train_step(p, m, v, users, items, labels, step, lr, dt=np.float64, mean_over=0):
    """-> dict(loss, pred, g, n, m, v)."""
    loss, pred, g = loss_and_grads(p, users, items, labels, dt, mean_over)
    if m is None:
        m = {k: np.zeros_like(np.asarray(x, dt)) for k, x in p.items()}
        v = {k: np.zeros_like(np.asarray(x, dt)) for k, x in p.items()}
    n, nm, nv = adam(p, g, m, v, step, lr, dt)
    return dict(loss=np.asarray([loss]), pred=pred, g=g, n=n, m=nm, v=nv)


def hr_ndcg(pred, label, chunk=100, top=10):
    """evaluate.py:51-68 over (prediction, label) lines in file order -> (user_num, hit ratio, ndcg)."""
    pred, label = np.asarray(pred, np.float64).reshape(-1), np.asarray(label).reshape(-1)
    hits, ndcg = [], []
    for a in range(0, len(pred), chunk):
        order = np.argsort(-pred[a:a + chunk], kind="stable")[:top]
        lab = label[a:a + chunk][order].tolist()
        if 1 in lab:
            hits.append(1)
            ndcg.append(math.log(2) / math.log(lab.index(1) + 2))
        else:
            hits.append(0)
            ndcg.append(0)
    return len(hits), float(np.mean(hits)), float(np.mean(ndcg))


def load_golden(path):
    """-> (arrays, starting parameters {name: array}, lr, steps)."""
    g = dict(np.load(path))
    p = {k[2:]: v for k, v in g.items() if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0])
