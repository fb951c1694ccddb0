"""NumPy restatement of the reference's rank/gatenet net (models/rank/gatenet/net.py, gatenet/dygraph_model.py) — TEST
ORACLE.  Float64 by default (`dtype`): the two gates forward / backward (what the rec_gate_* kernels compute) and the whole
net with a hand-written backward.  p = the reference's state_dict: "embedding.weight" [N, >= D],
"embedding_gate_weight_{s}" [1] (absent: no embedding gate), "linear_{i}.weight" / ".bias", "hidden_gate_weight_{i}"
[n_i, n_i] (absent: no hidden gate), "last_layer.weight" [n_last, 1], "last_layer.bias" [1].

    out_s   = e_s * sigmoid(w_s * sum_k e_s[k]),  e_s = embedding(ids[:, s])  (w_s ONE scalar; no padding row)  net.py:88-103
    feat    = [out_0 | .. | out_{S-1} | dense]                                                               net.py:110
    y_i     = relu(x @ W_i + b_i);  x = y_i * tanh(y_i @ G_i)   for every layer, the last included            net.py:112-118
    pred    = sigmoid(last_layer(x));  loss = mean log_loss(pred, label)                    net.py:119-120, dygraph_model.py:56-60
"""
import numpy as np

LOG_EPS = 1e-4                       # paddle.nn.functional.log_loss default epsilon


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def gate_emb_forward(e, w, dtype=np.float64):
    """e [B,S,D], w [S] -> (out [B,S,D], a [B,S,1], t [B,S,1])."""
    e, w = np.asarray(e, dtype), np.asarray(w, dtype).reshape(1, -1, 1)
    t = e.sum(axis=2, keepdims=True, dtype=dtype)
    with np.errstate(over="ignore"):
        a = sigmoid(w * t)
    return e * a, a, t


def gate_emb_backward(e, w, g, dtype=np.float64):
    """g [B,S,D] = d loss / d out -> (d e [B,S,D], d w [S])."""
    e, g = np.asarray(e, dtype), np.asarray(g, dtype)
    wv = np.asarray(w, dtype).reshape(1, -1, 1)
    _, a, t = gate_emb_forward(e, w, dtype)
    da = (g * e).sum(axis=2, keepdims=True, dtype=dtype)
    dp = da * a * (1 - a)
    return g * a + dp * wv, (dp * t).sum(axis=(0, 2), dtype=dtype)


def gate_hidden_forward(y, t, dtype=np.float64):
    """-> (x = y * tanh(t), h = tanh(t))."""
    h = np.tanh(np.asarray(t, dtype))
    return np.asarray(y, dtype) * h, h


def gate_hidden_backward(u, y, h, dtype=np.float64):
    """-> (dt = u * y * (1 - h^2), uh = u * h)."""
    u, y, h = np.asarray(u, dtype), np.asarray(y, dtype), np.asarray(h, dtype)
    return u * y * (1 - h * h), u * h


def n_linear(p):
    return sum(1 for k in p if k.startswith("linear_") and k.endswith(".weight"))


def gate_weights(p, S, dtype=np.float64):
    """The S scalars as one vector, or None when the net has no embedding gate."""
    if "embedding_gate_weight_0" not in p:
        return None
    return np.asarray([np.asarray(p["embedding_gate_weight_%d" % s], dtype).reshape(()) for s in range(S)], dtype)


def forward(ids, dense, p, D, dtype=np.float64):
    """-> dict(e, gw, feat, xs, ys, hs, logit, pred): xs[i] the input of layer i (xs[-1] the last_layer's), ys / hs per layer
    (hs[i] None without the hidden gate)."""
    ids = np.asarray(ids, np.int64)
    B, S = ids.shape
    e = np.asarray(p["embedding.weight"], dtype)[:, :D][ids]
    gw = gate_weights(p, S, dtype)
    out = e if gw is None else gate_emb_forward(e, gw, dtype)[0]
    feat = np.concatenate([out.reshape(B, S * D), np.asarray(dense, np.float32).astype(dtype)], axis=1)
    xs, ys, hs, x = [feat], [], [], feat
    for i in range(n_linear(p)):
        y = np.maximum(x @ np.asarray(p["linear_%d.weight" % i], dtype) + np.asarray(p["linear_%d.bias" % i], dtype), 0)
        h = None
        x = y
        if "hidden_gate_weight_%d" % i in p:
            x, h = gate_hidden_forward(y, y @ np.asarray(p["hidden_gate_weight_%d" % i], dtype), dtype)
        ys.append(y)
        hs.append(h)
        xs.append(x)
    logit = x @ np.asarray(p["last_layer.weight"], dtype) + np.asarray(p["last_layer.bias"], dtype)
    return dict(e=e, gw=gw, feat=feat, xs=xs, ys=ys, hs=hs, logit=logit, pred=sigmoid(logit))


def log_loss_mean(pred, label, dtype=np.float64):
    t = np.asarray(label).astype(dtype).reshape(-1, 1)
    e = dtype(LOG_EPS)
    return (-t * np.log(pred + e) - (1 - t) * np.log(1 - pred + e)).mean(dtype=dtype)


def loss_and_grads(ids, dense, label, p, D, dtype=np.float64, dz=None):
    """Forward + loss + backward -> dict: pred, loss, dfeat [B, S*D + Dn] (d loss / d feat), de [B,S,D] (d loss / d e),
    g = {state_dict key: grad} (embedding.weight densified [N,D]; every row is live).  dz [B,1] (optional): d loss /
    d logit to use instead of the log-loss's own (the float32 value the engine's loss head hands its backward)."""
    ids = np.asarray(ids, np.int64)
    B, S = ids.shape
    f = forward(ids, dense, p, D, dtype)
    pred = f["pred"]
    loss = log_loss_mean(pred, label, dtype)
    t = np.asarray(label).astype(dtype).reshape(-1, 1)
    eps = dtype(LOG_EPS)
    if dz is None:
        dz = ((-t / (pred + eps) + (1 - t) / (1 - pred + eps)) / dtype(B)) * (pred * (1 - pred))
    dz = np.asarray(dz, dtype).reshape(B, 1)
    g = {}
    g["last_layer.weight"] = f["xs"][-1].T @ dz
    g["last_layer.bias"] = dz.sum(axis=0)
    u = dz @ np.asarray(p["last_layer.weight"], dtype).T
    for i in reversed(range(n_linear(p))):
        y, h = f["ys"][i], f["hs"][i]
        if h is not None:
            G = np.asarray(p["hidden_gate_weight_%d" % i], dtype)
            dt, uh = gate_hidden_backward(u, y, h, dtype)
            g["hidden_gate_weight_%d" % i] = y.T @ dt
            u = dt @ G.T + uh
        dy = u * (y > 0)                                      # the ReLU's own mask: y, not the gated x
        g["linear_%d.weight" % i] = f["xs"][i].T @ dy
        g["linear_%d.bias" % i] = dy.sum(axis=0)
        u = dy @ np.asarray(p["linear_%d.weight" % i], dtype).T
    dfeat = u
    de = dfeat[:, :S * D].reshape(B, S, D)
    if f["gw"] is not None:
        de, dgw = gate_emb_backward(f["e"], f["gw"], de, dtype)
        for s in range(S):
            g["embedding_gate_weight_%d" % s] = dgw[s:s + 1]
    N = np.asarray(p["embedding.weight"]).shape[0]
    gE = np.zeros((N, D), dtype)
    np.add.at(gE, ids.reshape(-1), de.reshape(B * S, D))
    g["embedding.weight"] = gE
    return dict(pred=pred, loss=loss, dfeat=dfeat, de=de, g=g, dz=dz)


class Trainer:
    """Adam trajectory in float32 arrays (gradients in float64 from the float32 dz of the engine's loss head, then
    rounded): the Paddle Adam of oracle/deepfm_ref on every tensor; lazy: only the table rows the batch touches."""

    def __init__(self, p, D, lazy=False):
        self.D, self.lazy, self.step = D, lazy, 0
        self.p = {k: np.array(v, np.float32, copy=True) for k, v in p.items()}
        self.p["embedding.weight"] = self.p["embedding.weight"][:, :D].copy()
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}

    def train_step(self, ids, dense, label, lr=1e-3):
        from oracle import deepfm_ref as R
        self.step += 1
        o32 = forward(ids, dense, self.p, self.D)
        p32, t = o32["pred"].astype(np.float32), np.asarray(label).astype(np.float32).reshape(-1, 1)
        e = np.float32(LOG_EPS)
        dz = ((-t / (p32 + e) + (1 - t) / (1 - p32 + e)) / np.float32(len(t))) * (p32 * (1 - p32))
        o = loss_and_grads(ids, dense, label, self.p, self.D, dz=dz)
        for k, gr in o["g"].items():
            gr = np.asarray(gr, np.float32).reshape(self.p[k].shape)
            if k == "embedding.weight" and self.lazy:
                rows = np.unique(np.asarray(ids))
                R.adam_update_rows(self.p[k], self.m[k], self.v[k], rows, gr[rows], self.step, lr=lr)
            else:
                R.adam_update(self.p[k], self.m[k], self.v[k], gr, self.step, lr=lr)
        return float(o["loss"]), o["pred"]
