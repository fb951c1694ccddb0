"""NumPy restatement of the reference's rank/dcn net (models/rank/dcn/net.py, dcn/dygraph_model.py) — TEST ORACLE.

Float64 by default (`dtype`): the cross stack forward / backward (what rec_dcn_cross_fwd / rec_dcn_cross_bwd compute) and
the whole net with a hand-written backward.  p = the reference's state_dict: "embedding.weight" [N, >= D], "layer_w" [d],
"layer_b" [d], "linear_{i}.weight" / ".bias", "fc.weight" [H + d, 1], "fc.bias" [1] (numpy arrays).

    feat    = [embedding(ids) (0 where id == 0) | dense]                                   net.py:107-115
    s_l     = <x_l, w>;  x_{l+1} = x_0 * s_l + b + x_l;  l2 = sum_l sum (x_l * w)^2        net.py:117-138
    pred    = sigmoid(fc([relu-tower(feat) | x_L]));  loss = mean log_loss + l2            net.py:140-158, dygraph_model.py:98
The backward keeps every x_l of the forward and walks the layers in reverse with the plain chain rule (it does not use
the closed form x_l = x_0 * (1 + s_0 + ..) + l * b that the kernel rebuilds x_l with).
"""
import numpy as np

LOG_EPS = 1e-4                       # paddle.nn.functional.log_loss default epsilon


def cross_forward(x0, w, b, L, dtype=np.float64):
    """-> (x_L [B,d], s [B,L], l2 (coefficient 1), xs = [x_0 .. x_L])."""
    x0, w, b = np.asarray(x0, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    xs, s, l2 = [x0], np.zeros((x0.shape[0], L), dtype), dtype(0)
    x = x0
    for l in range(L):
        xw = x * w
        sl = xw.sum(axis=1, keepdims=True, dtype=dtype)
        l2 = l2 + (xw * xw).sum(dtype=dtype)
        s[:, l] = sl[:, 0]
        x = (x0 * sl + b) + x
        xs.append(x)
    return x, s, l2, xs


def cross_backward(x0, w, b, L, dxl, coeff=1.0, dtype=np.float64):
    """Gradients of  sum(x_L * dxl) + coeff * l2  -> (dx0 [B,d], dw [d], db [d])."""
    x0, w, b, g = np.asarray(x0, dtype), np.asarray(w, dtype), np.asarray(b, dtype), np.asarray(dxl, dtype).copy()
    _, s, _, xs = cross_forward(x0, w, b, L, dtype)
    c2 = dtype(2.0 * coeff)
    dx0, dw, db = np.zeros_like(x0), np.zeros_like(w), np.zeros_like(b)
    for l in reversed(range(L)):                        # x_{l+1} = x_0 * s_l + b + x_l, g = dT / d x_{l+1}
        xl = xs[l]
        t = (g * x0).sum(axis=1, keepdims=True, dtype=dtype)           # dT / d s_l
        dx0 += g * s[:, l:l + 1]
        db += g.sum(axis=0, dtype=dtype)
        dw += (t * xl).sum(axis=0, dtype=dtype) + c2 * (xl * xl * w).sum(axis=0, dtype=dtype)
        g = g + t * w + c2 * xl * w * w                                # dT / d x_l
    return dx0 + g, dw, db


def n_linear(p):
    return sum(1 for k in p if k.startswith("linear_") and k.endswith(".weight"))


def features(ids, dense, p, D, dtype=np.float64):
    ids = np.asarray(ids, np.int64)
    B, S = ids.shape
    E = np.asarray(p["embedding.weight"], dtype)[:, :D]
    emb = E[ids] * (ids != 0)[..., None]
    return np.concatenate([emb.reshape(B, S * D), np.asarray(dense, np.float32).astype(dtype)], axis=1)


def forward(ids, dense, p, D, L, dtype=np.float64):
    """-> dict(feat, zs, hs, cross_out, s, l2, xs, last, logit, pred)."""
    feat = features(ids, dense, p, D, dtype)
    hs, zs, h = [feat], [], feat
    for i in range(n_linear(p)):
        z = h @ np.asarray(p["linear_%d.weight" % i], dtype) + np.asarray(p["linear_%d.bias" % i], dtype)
        h = np.maximum(z, 0)
        zs.append(z)
        hs.append(h)
    xl, s, l2, xs = cross_forward(feat, p["layer_w"], p["layer_b"], L, dtype)
    last = np.concatenate([h, xl], axis=1)
    logit = last @ np.asarray(p["fc.weight"], dtype) + np.asarray(p["fc.bias"], dtype)
    pred = 1.0 / (1.0 + np.exp(-logit))
    return dict(feat=feat, zs=zs, hs=hs, cross_out=xl, s=s, l2=l2, xs=xs, last=last, logit=logit, pred=pred)


def log_loss_mean(pred, label, dtype=np.float64):
    t = np.asarray(label).astype(dtype).reshape(-1, 1)
    e = dtype(LOG_EPS)
    return (-t * np.log(pred + e) - (1 - t) * np.log(1 - pred + e)).mean(dtype=dtype)


def loss_and_grads(ids, dense, label, p, D, L, dtype=np.float64, dz=None):
    """Forward + loss + backward.  -> dict: pred, logloss, l2, loss, cross_out, dfeat [B,d], g = {state_dict key: grad}
    (embedding.weight: [N,D], row 0 zero).  dz [B,1] (optional): d loss / d logit to use instead of the log-loss's own
    (the float32 value the engine's loss head hands its backward)."""
    ids = np.asarray(ids, np.int64)
    B, S = ids.shape
    f = forward(ids, dense, p, D, L, dtype)
    pred = f["pred"]
    ll = log_loss_mean(pred, label, dtype)
    t = np.asarray(label).astype(dtype).reshape(-1, 1)
    e = dtype(LOG_EPS)
    if dz is None:
        dz = ((-t / (pred + e) + (1 - t) / (1 - pred + e)) / dtype(B)) * (pred * (1 - pred))
    dz = np.asarray(dz, dtype).reshape(B, 1)
    g = {}
    fcw = np.asarray(p["fc.weight"], dtype)
    g["fc.weight"] = f["last"].T @ dz
    g["fc.bias"] = dz.sum(axis=0)
    dlast = dz @ fcw.T
    n = n_linear(p)
    H = f["hs"][-1].shape[1]
    dh = dlast[:, :H]
    for i in reversed(range(n)):
        dzl = dh * (f["zs"][i] > 0)
        g["linear_%d.weight" % i] = f["hs"][i].T @ dzl
        g["linear_%d.bias" % i] = dzl.sum(axis=0)
        dh = dzl @ np.asarray(p["linear_%d.weight" % i], dtype).T
    dx0, g["layer_w"], g["layer_b"] = cross_backward(f["feat"], p["layer_w"], p["layer_b"], L, dlast[:, H:], 1.0, dtype)
    dfeat = dh + dx0
    N = np.asarray(p["embedding.weight"]).shape[0]
    gE = np.zeros((N, D), dtype)
    rows = dfeat[:, :S * D].reshape(B * S, D)
    for r, gr in zip(ids.reshape(-1), rows):
        if r != 0:
            gE[r] += gr
    g["embedding.weight"] = gE
    return dict(pred=pred, logloss=ll, l2=f["l2"], loss=ll + f["l2"], cross_out=f["cross_out"], dfeat=dfeat, g=g,
                dz=dz, s=f["s"])


class Trainer:
    """Adam trajectory in float32 arrays (gradients in float64 from the float32 dz of the engine's loss head, then
    rounded): the Paddle Adam of oracle/deepfm_ref on every tensor; lazy: only the table rows the batch touches."""

    def __init__(self, p, D, L, lazy=False):
        self.D, self.L, self.lazy, self.step = D, L, lazy, 0
        self.p = {k: np.array(v, np.float32, copy=True) for k, v in p.items()}
        self.p["embedding.weight"] = self.p["embedding.weight"][:, :D].copy()
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}

    def train_step(self, ids, dense, label, lr=1e-3):
        from oracle import deepfm_ref as R
        self.step += 1
        o32 = forward(ids, dense, self.p, self.D, self.L)
        p32, t = o32["pred"].astype(np.float32), np.asarray(label).astype(np.float32).reshape(-1, 1)
        e = np.float32(LOG_EPS)
        dz = ((-t / (p32 + e) + (1 - t) / (1 - p32 + e)) / np.float32(len(t))) * (p32 * (1 - p32))
        o = loss_and_grads(ids, dense, label, self.p, self.D, self.L, dz=dz)
        for k, gr in o["g"].items():
            gr = np.asarray(gr, np.float32).reshape(self.p[k].shape)
            if k == "embedding.weight" and self.lazy:
                rows = np.unique(np.asarray(ids))
                rows = rows[rows != 0]
                R.adam_update_rows(self.p[k], self.m[k], self.v[k], rows, gr[rows], self.step, lr=lr)
            else:
                R.adam_update(self.p[k], self.m[k], self.v[k], gr, self.step, lr=lr)
        return float(o["loss"]), o["pred"]
