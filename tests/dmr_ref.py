"""NumPy restatement of the reference's DMR (models/rank/dmr/net.py) — TEST INFRASTRUCTURE ONLY.

forward() / backward() follow net.py line by line, the [B, T, T] lower-triangular tile included, in float64 or (dtype=
np.float32) float32; adam_step() is paddle.optimizer.Adam's first steps.  Below them are the formulas of the new C-ABI
calls (include/recengine.h "DMR"), which tests/dmr_cpu_kernels.py and the GPU tests evaluate: prefix_pool_*, prelu_* and
match_loss_* (the tail glue is three lines of torch in the stand-in).  The product never imports this module."""
import numpy as np

T_HIST = 50
PAD = np.float32(-2 ** 32 + 1)                               # -4294967296.0 in float32

TABLES = ("uid_embeddings_var", "mid_embeddings_var", "cat_embeddings_var", "brand_embeddings_var", "btag_embeddings_var",
          "dm_btag_embeddings_var", "campaign_id_embeddings_var", "customer_embeddings_var", "cms_segid_embeddings_var",
          "cms_group_id_embeddings_var", "final_gender_code_embeddings_var", "age_level_embeddings_var",
          "pvalue_level_embeddings_var", "shopping_level_embeddings_var", "occupation_embeddings_var",
          "new_user_class_level_embeddings_var", "pid_embeddings_var", "position_embeddings_var",
          "dm_position_embeddings_var", "dm_item_vectors_var")
LINEARS = ("query_layer", "att_layer1_layer", "att_layer2_layer", "att_layer3_layer", "dnn_layer1_layer", "query_layer2",
           "att_layer1_layer2", "att_layer2_layer2", "att_layer3_layer2", "logits_layer", "dnn0_layer", "dnn1_layer",
           "dnn2_layer", "dnn3_layer")
PRELUS = ("query_prelu", "dnn_layer1_prelu", "query_prelu2", "dnn0_prelu", "dnn1_prelu", "dnn2_prelu", "dnn3_prelu")
BN = "inp_layer"
BN_MOMENTUM, BN_EPS = 0.99, 1e-3
# the 17 scalar columns behind the five history blocks (net.py:405-425; column 14 is the price's slot, unused as an id)
SCALARS = ("uid", "cms_segid", "cms_group_id", "final_gender_code", "age_level", "pvalue_level", "shopping_level",
           "occupation", "new_user_class_level", "mid", "cate_id", "campaign_id", "customer", "brand", "price_slot", "pid",
           "label")
USER_FEAT = (("uid", "uid_embeddings_var"), ("cms_segid", "cms_segid_embeddings_var"),
             ("cms_group_id", "cms_group_id_embeddings_var"), ("final_gender_code", "final_gender_code_embeddings_var"),
             ("age_level", "age_level_embeddings_var"), ("pvalue_level", "pvalue_level_embeddings_var"),
             ("shopping_level", "shopping_level_embeddings_var"), ("occupation", "occupation_embeddings_var"),
             ("new_user_class_level", "new_user_class_level_embeddings_var"))
ITEM_FEAT = (("mid", "mid_embeddings_var"), ("cate_id", "cat_embeddings_var"), ("brand", "brand_embeddings_var"),
             ("campaign_id", "campaign_id_embeddings_var"), ("customer", "customer_embeddings_var"))


def load_golden(golden_dir, name="dmr_E4"):
    """The golden of tools/make_golden_dmr.py as one dict (the main file and its two tower side files)."""
    import os
    g = {}
    for suffix in ("", "_tower_g", "_tower_n"):
        with np.load(os.path.join(golden_dir, name + suffix + ".npz")) as z:
            g.update({k: z[k] for k in z.files})
    return g


def param_keys():
    """state_dict keys, in no particular order."""
    return ([t + ".weight" for t in TABLES] + [l + s for l in LINEARS for s in (".weight", ".bias")] +
            [q + "._weight" for q in PRELUS] + [BN + s for s in (".weight", ".bias", "._mean", "._variance")])


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def split_feeds(sparse, T=T_HIST):
    s = np.asarray(sparse)
    f = dict(btag_his=s[:, 0:T], cate_his=s[:, T:2 * T], brand_his=s[:, 2 * T:3 * T], mask=s[:, 3 * T:4 * T],
             match_mask=s[:, 4 * T:5 * T])
    for i, n in enumerate(SCALARS):
        f[n] = s[:, 5 * T + i]
    return f


def _prelu(x, a, axis):
    sh = [1] * x.ndim
    sh[axis] = -1
    return np.where(x > 0, x, a.reshape(sh) * x)


def _prelu_bwd(x, dy, a, axis):
    sh = [1] * x.ndim
    sh[axis] = -1
    dx = np.where(x > 0, dy, a.reshape(sh) * dy)
    da = np.where(x > 0, 0, dy * x).sum(axis=tuple(i for i in range(x.ndim) if i != axis))
    return dx, da


def forward(p, sparse, price, T=T_HIST, train=True, dtype=np.float64):
    """net.py:393-554.  p: state_dict as arrays.  -> dict of outputs and of what backward() needs."""
    P = {k: np.asarray(v, dtype) for k, v in p.items()}
    f = split_feeds(sparse, T)
    emb = lambda tab, ids: P[tab + ".weight"][ids]
    lin = lambda x, n: x @ P[n + ".weight"] + P[n + ".bias"]
    B = f["mid"].shape[0]
    pad = dtype(PAD)
    c = dict(f=f, B=B, T=T)
    hist = c["hist"] = np.concatenate([emb("cat_embeddings_var", f["cate_his"]), emb("brand_embeddings_var", f["brand_his"])], -1)
    item_eb = c["item_eb"] = np.concatenate([emb("cat_embeddings_var", f["cate_id"]), emb("brand_embeddings_var", f["brand"])], -1)
    tile = lambda tab: np.broadcast_to(P[tab + ".weight"][None, :T], (B, T, P[tab + ".weight"].shape[1]))
    ctx = c["ctx"] = np.concatenate([tile("position_embeddings_var"), emb("btag_embeddings_var", f["btag_his"])], -1)
    ctx_dm = c["ctx_dm"] = np.concatenate([tile("dm_position_embeddings_var"), emb("dm_btag_embeddings_var", f["btag_his"])], -1)
    valid = c["valid"] = f["mask"] == 1
    mm = c["mm"] = f["match_mask"].astype(dtype)

    def att(q, names):
        feat = np.concatenate([q, hist, q - hist, q * hist], -1)
        a1 = sigmoid(lin(feat, names[0]))
        a2 = sigmoid(lin(a1, names[1]))
        return feat, a1, a2, lin(a2, names[2])[..., 0]

    # ---- user-to-item (deep_match, net.py:239-303)
    c["q1p"] = lin(ctx_dm, "query_layer")
    q1 = c["q1"] = _prelu(c["q1p"], P["query_prelu._weight"], 1)
    c["feat1"], c["a11"], c["a12"], s1 = att(q1, ("att_layer1_layer", "att_layer2_layer", "att_layer3_layer"))
    sm = np.where(valid, s1, pad)
    tril = np.tril(np.ones((T, T), bool))
    M = np.where(tril[None], sm[:, None, :], pad)                          # [B, T, T]: row i holds s_j for j <= i
    W1 = c["W1"] = softmax(M)
    pooled = c["pooled"] = W1 @ hist
    c["d1p"] = lin(pooled, "dnn_layer1_layer")
    d1 = c["d1"] = _prelu(c["d1p"], P["dnn_layer1_prelu._weight"], 1)
    uv = c["uv"] = d1[:, -1]
    uv2 = c["uv2"] = d1[:, -2] * mm[:, -2, None]
    V = P["dm_item_vectors_var.weight"]
    if train:
        logits = uv2 @ V.T                                                 # + the constant zero dm_item_biases
        lab = c["aux_label"] = f["cate_his"][:, -1]
        mx = logits.max(-1, keepdims=True)
        lse = c["lse"] = (mx + np.log(np.exp(logits - mx).sum(-1, keepdims=True)))[:, 0]
        c["aux"] = np.asarray([(lse - logits[np.arange(B), lab]).mean() * dtype(0.1)])
        c["logits"] = logits
    rel_u2i = (uv * V[f["cate_id"]]).sum(-1, keepdims=True)
    # ---- item-to-item (dmr_fcn_attention, net.py:305-357)
    c["q2in"] = np.concatenate([np.broadcast_to(item_eb[:, None, :], (B, T, item_eb.shape[1])), ctx], -1)
    c["q2p"] = lin(c["q2in"], "query_layer2")
    q2 = c["q2"] = _prelu(c["q2p"], P["query_prelu2._weight"], 1)
    c["feat2"], c["a21"], c["a22"], s2 = att(q2, ("att_layer1_layer2", "att_layer2_layer2", "att_layer3_layer2"))
    w2 = c["w2"] = softmax(np.where(valid, s2, pad))
    att_out = (w2[:, None, :] @ hist)[:, 0]
    rel_i2i = np.where(valid, s2, 0).sum(-1, keepdims=True)
    c["s1"], c["s2"] = s1, s2
    # ---- tower (net.py:460-552)
    hist_sum = c["hist_sum"] = hist.sum(1)
    pr = np.asarray(price, dtype).reshape(B, 1)
    parts = [emb(t, f[n]) for n, t in USER_FEAT] + [emb(t, f[n]) for n, t in ITEM_FEAT] + \
            [pr, emb("pid_embeddings_var", f["pid"]), hist_sum, item_eb * hist_sum, rel_u2i, rel_i2i, att_out]
    inp = c["inp"] = np.concatenate(parts, -1)
    if train:
        mean, var = inp.mean(0), inp.var(0)
        c["new_mean"] = BN_MOMENTUM * P[BN + "._mean"] + (1 - BN_MOMENTUM) * mean
        c["new_var"] = BN_MOMENTUM * P[BN + "._variance"] + (1 - BN_MOMENTUM) * var
    else:
        mean, var = P[BN + "._mean"], P[BN + "._variance"]
    c["invstd"] = 1 / np.sqrt(var + dtype(BN_EPS))
    c["xhat"] = (inp - mean) * c["invstd"]
    x = c["bn"] = c["xhat"] * P[BN + ".weight"] + P[BN + ".bias"]
    c["tower"] = []
    for i in range(4):
        z = lin(x, "dnn%d_layer" % i)
        c["tower"].append((x, z))
        x = _prelu(z, P["dnn%d_prelu._weight" % i], 1)
    c["dnn3"] = x
    c["y_hat"] = sigmoid(x)
    if train:
        z = x.sum(1)
        y = f["label"].astype(dtype)
        c["ctr"] = np.asarray([(np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean()])
        c["loss"] = c["ctr"] + c["aux"]
    c["P"] = P
    return c


def backward(c):
    """Gradients of loss = ctr + aux for every state_dict key (tables dense; logits_layer and the BatchNorm statistics:
    zeros — they get none)."""
    P, f, B, T = c["P"], c["f"], c["B"], c["T"]
    dt = c["inp"].dtype
    g = {k: np.zeros_like(v) for k, v in P.items()}
    hist, valid = c["hist"], c["valid"]
    E2 = hist.shape[-1]
    E = E2 // 2

    def lin_bwd(name, x, dy):
        g[name + ".weight"] += x.reshape(-1, x.shape[-1]).T @ dy.reshape(-1, dy.shape[-1])
        g[name + ".bias"] += dy.reshape(-1, dy.shape[-1]).sum(0)
        return dy @ P[name + ".weight"].T

    def table_bwd(tab, ids, d):
        np.add.at(g[tab + ".weight"], np.asarray(ids).reshape(-1), d.reshape(-1, d.shape[-1]))

    # ---- tower
    y = f["label"].astype(dt)
    d = ((c["y_hat"].sum(1) - y) / B)[:, None]                              # d ctr / d sum(dnn3, 1)
    for i in (3, 2, 1, 0):
        x, z = c["tower"][i]
        d, g["dnn%d_prelu._weight" % i] = _prelu_bwd(z, d, P["dnn%d_prelu._weight" % i], 1)
        d = lin_bwd("dnn%d_layer" % i, x, d)
    g[BN + ".weight"] = (d * c["xhat"]).sum(0)
    g[BN + ".bias"] = d.sum(0)
    dxh = d * P[BN + ".weight"]
    d_inp = c["invstd"] * (dxh - dxh.mean(0) - c["xhat"] * (dxh * c["xhat"]).mean(0))
    col = [0]

    def take(n):
        col[0] += n
        return d_inp[:, col[0] - n:col[0]]

    d_hist = np.zeros_like(hist)
    d_item_eb = np.zeros_like(c["item_eb"])
    for n, t in USER_FEAT:
        table_bwd(t, f[n], take(P[t + ".weight"].shape[1]))
    for n, t in ITEM_FEAT:
        dd = take(P[t + ".weight"].shape[1])
        if n == "cate_id":
            d_item_eb[:, :E] += dd
        elif n == "brand":
            d_item_eb[:, E:] += dd
        else:
            table_bwd(t, f[n], dd)
    take(1)                                                                 # price
    table_bwd("pid_embeddings_var", f["pid"], take(P["pid_embeddings_var.weight"].shape[1]))
    d_sum, d_prod, d_rel_u2i, d_rel_i2i, d_att = take(E2), take(E2), take(1), take(1), take(E2)
    d_hist += (d_sum + d_prod * c["item_eb"])[:, None, :]
    d_item_eb += d_prod * c["hist_sum"]

    def att_bwd(ds, q, feat, a1, a2, names):
        dd = lin_bwd(names[2], a2, ds[..., None]) * a2 * (1 - a2)
        dd = lin_bwd(names[1], a1, dd) * a1 * (1 - a1)
        df = lin_bwd(names[0], feat, dd)
        n = q.shape[-1]
        d0, d1, d2, d3 = df[..., :n], df[..., n:2 * n], df[..., 2 * n:3 * n], df[..., 3 * n:]
        d_hist[...] += d1 - d2 + d3 * q
        return d0 + d2 + d3 * hist

    # ---- item-to-item
    w2 = c["w2"]
    d_hist += w2[:, :, None] * d_att[:, None, :]
    gw = (hist @ d_att[:, :, None])[..., 0]                                 # [B, T]
    dsm = w2 * (gw - (w2 * gw).sum(-1, keepdims=True))
    ds2 = np.where(valid, dsm, 0) + np.where(valid, d_rel_i2i, 0)
    dq2 = att_bwd(ds2, c["q2"], c["feat2"], c["a21"], c["a22"], ("att_layer1_layer2", "att_layer2_layer2", "att_layer3_layer2"))
    dq2p, g["query_prelu2._weight"] = _prelu_bwd(c["q2p"], dq2, P["query_prelu2._weight"], 1)
    dq2in = lin_bwd("query_layer2", c["q2in"], dq2p)
    d_item_eb += dq2in[..., :E2].sum(1)
    O = P["position_embeddings_var.weight"].shape[1]
    g["position_embeddings_var.weight"][:T] += dq2in[..., E2:E2 + O].sum(0)
    table_bwd("btag_embeddings_var", f["btag_his"], dq2in[..., E2 + O:])
    # ---- user-to-item
    V = P["dm_item_vectors_var.weight"]
    dl = np.exp(c["logits"] - c["lse"][:, None])
    dl[np.arange(B), c["aux_label"]] -= 1
    dl *= dt.type(0.1) / B
    g["dm_item_vectors_var.weight"] += dl.T @ c["uv2"]
    dd1 = np.zeros_like(c["d1"])
    dd1[:, -2] = (dl @ V) * c["mm"][:, -2, None]
    dd1[:, -1] = d_rel_u2i * V[f["cate_id"]]
    table_bwd("dm_item_vectors_var", f["cate_id"], d_rel_u2i * c["uv"])
    dd1p, g["dnn_layer1_prelu._weight"] = _prelu_bwd(c["d1p"], dd1, P["dnn_layer1_prelu._weight"], 1)
    dpool = lin_bwd("dnn_layer1_layer", c["pooled"], dd1p)
    W1 = c["W1"]
    d_hist += np.swapaxes(W1, 1, 2) @ dpool
    dW1 = dpool @ np.swapaxes(hist, 1, 2)                                   # [B, T, T]
    dM = W1 * (dW1 - (W1 * dW1).sum(-1, keepdims=True))
    dsm1 = np.where(np.tril(np.ones((T, T), bool))[None], dM, 0).sum(1)
    ds1 = np.where(valid, dsm1, 0)
    dq1 = att_bwd(ds1, c["q1"], c["feat1"], c["a11"], c["a12"], ("att_layer1_layer", "att_layer2_layer", "att_layer3_layer"))
    dq1p, g["query_prelu._weight"] = _prelu_bwd(c["q1p"], dq1, P["query_prelu._weight"], 1)
    dctx = lin_bwd("query_layer", c["ctx_dm"], dq1p)
    g["dm_position_embeddings_var.weight"][:T] += dctx[..., :O].sum(0)
    table_bwd("dm_btag_embeddings_var", f["btag_his"], dctx[..., O:])
    # ---- the shared tables
    table_bwd("cat_embeddings_var", f["cate_his"], d_hist[..., :E])
    table_bwd("brand_embeddings_var", f["brand_his"], d_hist[..., E:])
    table_bwd("cat_embeddings_var", f["cate_id"], d_item_eb[:, :E])
    table_bwd("brand_embeddings_var", f["brand"], d_item_eb[:, E:])
    c["d_hist"], c["d_item_eb"], c["ds1"], c["ds2"] = d_hist, d_item_eb, ds1, ds2
    return g


NO_GRAD = ("logits_layer.weight", "logits_layer.bias", BN + "._mean", BN + "._variance")


def adam_step(p, g, lr, state=None, beta1=0.9, beta2=0.999, eps=1e-8, dtype=np.float64):
    """paddle.optimizer.Adam (non-lazy) on every parameter that has a gradient.  state: {'t', 'm', 'v'} carried between
    steps (None: the first step).  -> (new parameters, state)."""
    st = state if state is not None else dict(t=0, m={}, v={})
    st["t"] += 1
    t = st["t"]
    new = {}
    for k, w in p.items():
        w = np.asarray(w, dtype)
        if k in NO_GRAD:
            new[k] = w.copy()
            continue
        gk = np.asarray(g[k], dtype)
        m = st["m"][k] = dtype(beta1) * st["m"].get(k, 0) + dtype(1 - beta1) * gk
        v = st["v"][k] = dtype(beta2) * st["v"].get(k, 0) + dtype(1 - beta2) * gk * gk
        lr_t = dtype(lr) * np.sqrt(dtype(1 - beta2 ** t)) / dtype(1 - beta1 ** t)
        new[k] = w - lr_t * m / (np.sqrt(v) + dtype(eps) * np.sqrt(dtype(1 - beta2 ** t)))
    return new, st


def train_step(p, sparse, price, lr, state=None, dtype=np.float64):
    """One train step: -> (forward record, gradients, parameters after Adam with the BatchNorm statistics moved, state)."""
    c = forward(p, sparse, price, train=True, dtype=dtype, T=(np.shape(sparse)[1] - 17) // 5)
    g = backward(c)
    new, state = adam_step(p, g, lr, state, dtype=dtype)
    new[BN + "._mean"], new[BN + "._variance"] = c["new_mean"], c["new_var"]
    return c, g, new, state


# ------------------------------------------------------------------------------------------------ the new C-ABI calls
def prefix_pool_fwd(score, mask, hist, rows, dtype=np.float64):
    """-> (out [B,R,D], w [B,R,T], rel [B])."""
    s, h = np.asarray(score, dtype), np.asarray(hist, dtype)
    valid = np.asarray(mask) == 1
    T = s.shape[1]
    j = np.arange(T)
    v = np.stack([np.where(valid & (j[None, :] <= r), s, dtype(PAD)) for r in rows], 1)        # [B, R, T]
    w = softmax(v)
    return w @ h, w, np.where(valid, s, 0).sum(1)


def prefix_pool_bwd(mask, hist, rows, w, d_out, d_rel=None, dtype=np.float64):
    """-> (dscore [B,T], d_hist [B,T,D])."""
    h, w, do = np.asarray(hist, dtype), np.asarray(w, dtype), np.asarray(d_out, dtype)
    valid = np.asarray(mask) == 1
    T = h.shape[1]
    j = np.arange(T)
    gg = do @ np.swapaxes(h, 1, 2)                                          # [B, R, T]
    dv = w * (gg - (w * gg).sum(-1, keepdims=True))
    gate = np.stack([valid & (j[None, :] <= r) for r in rows], 1)
    ds = np.where(gate, dv, 0).sum(1)
    if d_rel is not None:
        ds = ds + np.where(valid, np.asarray(d_rel, dtype).reshape(-1, 1), 0)
    return ds, np.swapaxes(w, 1, 2) @ do


def _channels(m, n, num_alpha, period, base):
    return (base + np.arange(m) % period)[:, None].repeat(n, 1) if period > 0 else np.arange(n)[None, :].repeat(m, 0)


def prelu_fwd(x, alpha, period=0, base=0, dtype=np.float64):
    x, a = np.asarray(x, dtype), np.asarray(alpha, dtype)
    ch = _channels(x.shape[0], x.shape[1], a.size, period, base)
    return np.where(x > 0, x, a[ch] * x)


def prelu_bwd(x, dy, alpha, period=0, base=0, dtype=np.float64):
    x, dy, a = np.asarray(x, dtype), np.asarray(dy, dtype), np.asarray(alpha, dtype)
    ch = _channels(x.shape[0], x.shape[1], a.size, period, base)
    da = np.zeros(a.size, dtype)
    np.add.at(da, ch.reshape(-1), np.where(x > 0, 0, dy * x).reshape(-1))
    return np.where(x > 0, dy, a[ch] * dy), da


def match_loss_fwd(U, V, bias, label, dtype=np.float64):
    """-> (loss, lse [B]); a label outside [0, C) contributes its lse alone."""
    z = np.asarray(U, dtype) @ np.asarray(V, dtype).T + (0 if bias is None else np.asarray(bias, dtype))
    mx = z.max(-1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))[:, 0]
    lab = np.asarray(label)
    ok = (lab >= 0) & (lab < z.shape[1])
    zl = np.where(ok, z[np.arange(z.shape[0]), np.where(ok, lab, 0)], 0)
    return (lse - zl).mean(), lse


def match_loss_bwd(U, V, bias, label, d_loss, dtype=np.float64):
    """-> (dU [B,K], dV [C,K])."""
    U, V = np.asarray(U, dtype), np.asarray(V, dtype)
    z = U @ V.T + (0 if bias is None else np.asarray(bias, dtype))
    G = softmax(z)
    lab = np.asarray(label)
    ok = (lab >= 0) & (lab < z.shape[1])
    G[np.arange(z.shape[0])[ok], lab[ok]] -= 1
    G *= dtype(d_loss) / z.shape[0]
    return G @ V, G.T @ U
