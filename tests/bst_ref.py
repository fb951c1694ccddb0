"""Float64 restatement of BST (models/rank/bst/net.py, dygraph_model.py): forward, backward and the Adagrad step, and each
new kernel of csrc/bst_ops.hip — TEST INFRASTRUCTURE ONLY.  `dtype=np.float32` evaluates the same formulas in float32:
the error yardstick of the tests (bound = 8 x that error, floor 1e-6).

Parameters are a dict under the reference's state_dict names (Linear weights [in, out]).  Feeds are a dict: userid,
target_item, target_cat, target_position [B,1]; hist_item, hist_cat, hist_position [B,T]; label [B,1].  Dropout is given as
ready masks (keep / (1 - p), or None): `masks` maps a site name to its mask — "pp0", "pp1", ... for the 'd' letters of the
pre / post-process commands in the order the forward meets them (shape [B*L, d_model]), "att" for the softmax weights
([B*H*L, L]) and "ffn" behind hid2_l."""
import numpy as np

F64 = np.float64
LN_EPS, SLOPE, LOG_EPS, ADAGRAD_EPS, LR = 1e-5, 0.01, 1e-4, 1e-6, 1e-3
TABLES = ("hist_item_emb_attr", "hist_cat_emb_attr", "hist_position_emb_attr", "target_item_emb_attr",
          "target_cat_emb_attr", "target_position_emb_attr", "userid_attr")
ID_FEEDS = ("hist_item", "hist_cat", "hist_position", "target_item", "target_cat", "target_position", "userid")
# zero in exact arithmetic: a constant added to every key (k_liner.bias) or to every score of a row shifts each softmax
# row by a constant.  With preprocess_cmd "n" the final layer norm removes the row mean of its input, so the bias of hid2_l
# (added to every position alike, ahead of LN(LN(.))) still matters per column, not per row — it is NOT one of these.
STRUCTURAL_ZERO = ("bst.k_liner.bias",)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


# ------------------------------------------------------------------------------------------------ kernels
def mha_fwd(q, k, v, B, L, H, scale=1.0, mask=None, dtype=F64):
    """q, k [B*L, H*dk], v [B*L, H*dv]; mask [B*H*L, L] (keep / (1-p)) or None -> (out [B*L, H*dv], lse [B,H,L], P)."""
    dk, dv = q.shape[1] // H, v.shape[1] // H
    q4 = np.asarray(q, dtype).reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    k4 = np.asarray(k, dtype).reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    v4 = np.asarray(v, dtype).reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    s = (q4 @ k4.transpose(0, 1, 3, 2)) * dtype(scale)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    P = e / l
    Pd = P if mask is None else P * np.asarray(mask, dtype).reshape(B, H, L, L)
    out = (Pd @ v4).transpose(0, 2, 1, 3).reshape(B * L, H * dv)
    return out, (m + np.log(l))[..., 0], P


def mha_bwd(q, k, v, B, L, H, d_out, scale=1.0, mask=None, dtype=F64):
    """-> (dq, dk, dv) in the layouts of q, k, v."""
    dk, dv = q.shape[1] // H, v.shape[1] // H
    _, _, P = mha_fwd(q, k, v, B, L, H, scale, None, dtype)
    q4 = np.asarray(q, dtype).reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    k4 = np.asarray(k, dtype).reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    v4 = np.asarray(v, dtype).reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    g4 = np.asarray(d_out, dtype).reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    mk = dtype(1) if mask is None else np.asarray(mask, dtype).reshape(B, H, L, L)
    dP = (g4 @ v4.transpose(0, 1, 3, 2)) * mk
    dV = (P * mk).transpose(0, 1, 3, 2) @ g4
    dS = P * (dP - (P * dP).sum(-1, keepdims=True))
    dQ = (dS @ k4) * dtype(scale)
    dK = (dS.transpose(0, 1, 3, 2) @ q4) * dtype(scale)
    back = lambda t, d: t.transpose(0, 2, 1, 3).reshape(B * L, H * d)
    return back(dQ, dk), back(dK, dk), back(dV, dv)


def add_layer_norm_fwd(x, r=None, eps=LN_EPS, dtype=F64):
    """-> (y, mean, rstd): y = LN(x + r) over the last axis, biased variance, no affine parameters."""
    t = np.asarray(x, dtype) if r is None else np.asarray(x, dtype) + np.asarray(r, dtype)
    mu = t.mean(-1, keepdims=True)
    var = ((t - mu) ** 2).mean(-1, keepdims=True)
    rstd = 1 / np.sqrt(var + dtype(eps))
    return (t - mu) * rstd, mu[..., 0], rstd[..., 0]


def add_layer_norm_bwd(y, rstd, dy, dtype=F64):
    y, dy, rs = np.asarray(y, dtype), np.asarray(dy, dtype), np.asarray(rstd, dtype)[..., None]
    return rs * (dy - dy.mean(-1, keepdims=True) - y * (dy * y).mean(-1, keepdims=True))


def leaky_relu_fwd(x, slope=SLOPE, dtype=F64):
    x = np.asarray(x, dtype)
    return np.where(x > 0, x, dtype(slope) * x)


def leaky_relu_bwd(y, dy, slope=SLOPE, dtype=F64):
    return np.where(np.asarray(y) > 0, np.asarray(dy, dtype), dtype(slope) * np.asarray(dy, dtype))


def log_loss(pred, label, dtype=F64):
    """paddle.nn.functional.log_loss (epsilon 1e-4) + mean -> (loss, d loss / d pred)."""
    e, y, n = dtype(LOG_EPS), np.asarray(label, dtype), dtype(pred.size)
    loss = (-y * np.log(pred + e) - (1 - y) * np.log(1 - pred + e)).mean()
    return loss, (-y / (pred + e) + (1 - y) / (1 - pred + e)) / n


def adagrad(p, acc, g, lr=LR, eps=ADAGRAD_EPS):
    """paddle.optimizer.Adagrad: acc += g^2; p -= lr g / (sqrt(acc) + eps) -> (p, acc)."""
    dt = p.dtype.type
    acc = acc + g * g
    return p - dt(lr) * g / (np.sqrt(acc) + dt(eps)), acc


# ------------------------------------------------------------------------------------------------ the net
def config(n_head, d_key, d_value, preprocess_cmd="da", postprocess_cmd="da"):
    return dict(n_head=int(n_head), d_key=int(d_key), d_value=int(d_value), pre=str(preprocess_cmd), post=str(postprocess_cmd))


def dropout_sites(cfg):
    """The 'd' sites of the pre / post-process commands in forward order: pre (attention input), post (first residual),
    pre (second residual), pre (final)."""
    cmds = cfg["pre"] + cfg["post"] + cfg["pre"] + cfg["pre"]
    return ["pp%d" % i for i in range(cmds.count("d"))]


def num_dnn(p):
    return sum(1 for k in p if k.startswith("bst.dnn_linear_") and k.endswith(".weight"))


class _Proc:
    """pre_post_process_layer (prev None) / pre_post_process_layer_ (net.py:272-317) with a tape for the backward."""

    def __init__(self, masks, dtype):
        self.masks, self.dtype, self.site = masks or {}, dtype, 0

    def fwd(self, x, prev, cmd):
        out, tape = (x if prev is None else x + prev), []
        for c in cmd:
            if c == "n":
                out, _, rstd = add_layer_norm_fwd(out, None, LN_EPS, self.dtype)
                tape.append(("n", out, rstd))
            elif c == "d":
                m = self.masks.get("pp%d" % self.site)
                self.site += 1
                if m is not None:
                    m = np.asarray(m, self.dtype)
                    out = out * m
                    tape.append(("d", m, None))
        return out, tape

    def bwd(self, g, tape):
        for kind, a, b in reversed(tape):
            g = g * a if kind == "d" else add_layer_norm_bwd(a, b, g, self.dtype)
        return g


def forward_backward(p, feeds, cfg, masks=None, dtype=F64, want_grads=True):
    """-> (pred [B,1], loss, grads {name: array, tables dense}, cache)."""
    p = {k: np.asarray(v, dtype) for k, v in p.items()}
    ids = {k: np.asarray(feeds[k], np.int64) for k in ID_FEEDS}
    B, T = ids["hist_item"].shape
    L, H = T + 1, cfg["n_head"]
    W = lambda n: p["bst.%s.weight" % n]
    bias = lambda n: p["bst.%s.bias" % n]
    hist = np.concatenate([W(TABLES[i])[ids[ID_FEEDS[i]]] for i in range(3)], 2)                    # [B, T, dm]
    tgt = np.concatenate([W(TABLES[i])[ids[ID_FEEDS[i]].reshape(B, 1)] for i in range(3, 6)], 2)    # [B, 1, dm]
    user = W("userid_attr")[ids["userid"].reshape(B)]                                               # [B, dm]
    dm = hist.shape[2]
    X = np.concatenate([hist, tgt], 1).reshape(B * L, dm)
    masks = masks or {}
    pr = _Proc(masks, dtype)
    # encoder_layer (net.py:400-416)
    a_in, tape0 = pr.fwd(X, None, cfg["pre"])
    q, k, v = (a_in @ W(n) + bias(n) for n in ("q_liner", "k_liner", "v_liner"))
    m_att = masks.get("att")
    ctx, _, _ = mha_fwd(q, k, v, B, L, H, 1.0, m_att, dtype)
    att = ctx @ W("po_liner") + bias("po_liner")
    A, tape1 = pr.fwd(att, X, cfg["post"])
    h1 = A @ W("hid_l") + bias("hid_l")
    a1 = leaky_relu_fwd(h1, SLOPE, dtype)
    f = a1 @ W("hid2_l") + bias("hid2_l")
    m_ffn = masks.get("ffn")
    if m_ffn is not None:
        f = f * np.asarray(m_ffn, dtype)
    E1, tape2 = pr.fwd(f, A, cfg["pre"])
    E, tape3 = pr.fwd(E1, None, cfg["pre"])                                                         # net.py:450
    Z = np.concatenate([user[:, None, :], E.reshape(B, L, dm)], 1).reshape(B * (L + 1), dm)
    n = num_dnn(p)
    x, acts = Z, []
    for i in range(n):
        z = x @ W("dnn_linear_%d" % i) + bias("dnn_linear_%d" % i)
        y = leaky_relu_fwd(z, SLOPE, dtype) if i < n - 1 else z
        acts.append((x, y))
        x = y
    logit = x.reshape(B, L + 1).sum(1, keepdims=True) + p["bias"]
    pred = sigmoid(logit)
    loss, dpred = log_loss(pred, feeds["label"], dtype)
    cache = dict(X=X, a_in=a_in, q=q, k=k, v=v, ctx=ctx, att=att, A=A, a1=a1, f=f, E=E, Z=Z, logit=logit)
    if not want_grads:
        return pred, loss, None, cache
    g = {}
    dlogit = dpred * pred * (1 - pred)
    g["bias"] = dlogit.sum().reshape(1)
    d = np.repeat(dlogit, L + 1, 1).reshape(B * (L + 1), 1)

    def lin_bwd(name, x_in, dy):
        g["bst.%s.weight" % name] = x_in.T @ dy
        g["bst.%s.bias" % name] = dy.sum(0)
        return dy @ W(name).T

    for i in reversed(range(n)):
        x_in, y = acts[i]
        if i < n - 1:
            d = leaky_relu_bwd(y, d, SLOPE, dtype)
        d = lin_bwd("dnn_linear_%d" % i, x_in, d)
    dZ = d.reshape(B, L + 1, dm)
    d_user = dZ[:, 0]
    gE1 = pr.bwd(pr.bwd(dZ[:, 1:].reshape(B * L, dm), tape3), tape2)          # feeds f and A
    gf = gE1 if m_ffn is None else gE1 * np.asarray(m_ffn, dtype)
    da1 = lin_bwd("hid2_l", a1, gf)
    gA = gE1 + lin_bwd("hid_l", A, leaky_relu_bwd(a1, da1, SLOPE, dtype))
    g_att = pr.bwd(gA, tape1)                                                 # feeds att and X
    d_ctx = lin_bwd("po_liner", ctx, g_att)
    dq, dk, dv = mha_bwd(q, k, v, B, L, H, d_ctx, 1.0, m_att, dtype)
    g_ain = lin_bwd("q_liner", a_in, dq) + lin_bwd("k_liner", a_in, dk) + lin_bwd("v_liner", a_in, dv)
    dX = (g_att + pr.bwd(g_ain, tape0)).reshape(B, L, dm)
    widths = [W(TABLES[i]).shape[1] for i in range(3)]
    c0 = 0
    for s in range(3):
        for t, rows, idv in ((s, dX[:, :T, c0:c0 + widths[s]], ids[ID_FEEDS[s]]),
                             (s + 3, dX[:, T:, c0:c0 + widths[s]], ids[ID_FEEDS[s + 3]].reshape(B, 1))):
            gt = np.zeros_like(W(TABLES[t]))
            np.add.at(gt, idv.reshape(-1), rows.reshape(-1, widths[s]))
            g["bst.%s.weight" % TABLES[t]] = gt
        c0 += widths[s]
    gu = np.zeros_like(W("userid_attr"))
    np.add.at(gu, ids["userid"].reshape(-1), d_user)
    g["bst.userid_attr.weight"] = gu
    cache.update(dX=dX.reshape(B * L, dm), dZ=dZ, dq=dq, dk=dk, dv=dv, d_ctx=d_ctx)
    return pred, loss, g, cache


def train_step(p, acc, feeds, cfg, masks=None, lr=LR, dtype=F64):
    """One Adagrad step over ALL parameters -> (pred, loss, grads, new params, new accumulators).  acc None: zeros."""
    pred, loss, g, _ = forward_backward(p, feeds, cfg, masks, dtype)
    new, nacc = {}, {}
    for k in p:
        pk = np.asarray(p[k], dtype)
        ak = np.zeros_like(pk) if acc is None else np.asarray(acc[k], dtype)
        new[k], nacc[k] = adagrad(pk, ak, g[k].reshape(pk.shape), lr)
    return pred, loss, g, new, nacc


def load_golden(path):
    """-> (g, params, feeds, cfg) of a tests/golden/bst_*.npz."""
    g = dict(np.load(path))
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    feeds = {k[2:]: g[k] for k in g if k.startswith("f_")}
    H, dk, dv = (int(x) for x in g["heads"])
    return g, p, feeds, config(H, dk, dv, str(g["pre"]), str(g["post"]))


def step_bound(g64, acc64, new64, grad_err_bound, lr=LR, eps=ADAGRAD_EPS):
    """Elementwise bound on a parameter after ONE Adagrad step from accumulator acc64: the step is lr g / (s + eps) with
    s = sqrt(acc + g^2), its sensitivity to g is lr (s + eps - g^2 / s) / (s + eps)^2 (= lr eps / (|g| + eps)^2 from
    accumulator 0), times the absolute gradient bound of the tensor, capped at lr (no step is larger), plus 4 float32
    roundings of the stored parameter."""
    s = np.sqrt(acc64 + g64 * g64)
    sens = lr * (s + eps - np.where(s > 0, g64 * g64 / np.maximum(s, 1e-300), 0.0)) / (s + eps) ** 2
    return np.minimum(sens * grad_err_bound, lr) + 4 * np.finfo(np.float32).eps * np.abs(new64)


def kbias_noise_scale(cache, B, L, H):
    """The scale of the terms that cancel in the gradient of k_liner.bias (STRUCTURAL_ZERO): it is sum_j dK_j with dK_j =
    sum_i P_ij (dP_ij - D_i) q_i, and sum_j P_ij (dP_ij - D_i) = 0 for every i.  -> max over the columns of
    sum_{b,i,j} P_ij (|dP_ij| + |D_i|) |q_i|, from a float64 forward_backward cache (no attention dropout)."""
    q, k, v, g = cache["q"], cache["k"], cache["v"], cache["d_ctx"]
    dk, dv = q.shape[1] // H, v.shape[1] // H
    _, _, P = mha_fwd(q, k, v, B, L, H)
    q4 = q.reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    v4 = v.reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    g4 = g.reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    dP = g4 @ v4.transpose(0, 1, 3, 2)
    D = (P * dP).sum(-1, keepdims=True)
    w = (P * (np.abs(dP) + np.abs(D))).sum(-1)                       # [B, H, L]
    return float((w[..., None] * np.abs(q4)).sum((0, 2)).max())
