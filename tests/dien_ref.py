"""DIEN (models/rank/dien/net.py DIENLayer + dygraph_model.py) restated in numpy: forward, backward and the SGD step.

Every function takes `dtype`: float64 is the reference the tests compare against; float32 evaluates the same formulas in
the kernels' precision and gives the tests their error scale (tests/test_dien_gpu.py: a kernel may be 8 x as far from
the float64 result as this float32 evaluation is, floor 1e-6).  Against the golden (tests/golden/dien_D8.npz, recorded
from the reference's own net.py in float32) the float64 run agrees to the float32 rounding of that recording: the bound
used in tests/test_dien.py is 2e-5 of a tensor's largest magnitude (measured there: at most 1.4e-6).

Layouts are the reference's: Linear weights [in, out]; GRU weight_ih [3H, E], weight_hh [3H, H], gate order r, z, c
(Paddle's documented GRU formula, which is torch.nn.GRU's gate for gate):
    r = s(W_ir x + b_ir + W_hr h + b_hr)   z = s(W_iz x + b_iz + W_hz h + b_hz)
    c = tanh(W_ic x + b_ic + r * (W_hc h + b_hc))   h' = z * h + (1 - z) * c
"""
import numpy as np

EPS = 1e-8
TABLES = ("hist_item_emb_attr", "hist_cat_emb_attr", "target_item_emb_attr", "target_cat_emb_attr",
          "target_item_seq_emb_attr", "target_cat_seq_emb_attr", "neg_item_seq_emb_attr", "neg_cat_seq_emb_attr")
GRUS = ("gru_net.%s_l0", "gru_net.%s_l1", "gru_cell_attention.%s")


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lookup(W, ids, padding_idx=0):
    """Embedding with padding_idx: that id reads as a zero row."""
    out = W[ids]
    if padding_idx is not None:
        out = np.where((ids == padding_idx)[..., None], np.zeros((), W.dtype), out)
    return out


# ---------------------------------------------------------------- GRU
def gru_fwd(X, W_ih, W_hh, b_ih, b_hh, dtype=np.float64):
    X, W_ih, W_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (X, W_ih, W_hh, b_ih, b_hh))
    B, T, _ = X.shape
    H = W_hh.shape[1]
    Gi = X @ W_ih.T + b_ih
    h = np.zeros((B, H), dtype)
    sv = {k: np.zeros((B, T, H), dtype) for k in ("r", "z", "c", "hc", "hp")}
    Hout = np.zeros((B, T, H), dtype)
    for t in range(T):
        gh = h @ W_hh.T + b_hh
        r = sigmoid(Gi[:, t, :H] + gh[:, :H])
        z = sigmoid(Gi[:, t, H:2 * H] + gh[:, H:2 * H])
        hc = gh[:, 2 * H:]
        c = np.tanh(Gi[:, t, 2 * H:] + r * hc)
        for k, v in (("r", r), ("z", z), ("c", c), ("hc", hc), ("hp", h)):
            sv[k][:, t] = v
        h = z * h + (1 - z) * c
        Hout[:, t] = h
    sv["Gi"] = Gi
    return Hout, sv


def gru_bwd(sv, W_hh, dH_out=None, dh_T=None, dtype=np.float64):
    """-> (dGi, dGh) [B,T,3H]."""
    W_hh = np.asarray(W_hh, dtype)
    B, T, H = sv["r"].shape
    dGi, dGh = np.zeros((B, T, 3 * H), dtype), np.zeros((B, T, 3 * H), dtype)
    dh = np.zeros((B, H), dtype) if dh_T is None else np.asarray(dh_T, dtype).copy()
    for t in range(T - 1, -1, -1):
        r, z, c, hc, hp = (sv[k][:, t] for k in ("r", "z", "c", "hc", "hp"))
        d = dh + (np.asarray(dH_out[:, t], dtype) if dH_out is not None else 0)
        dz = d * (hp - c) * z * (1 - z)
        dc = d * (1 - z) * (1 - c * c)
        dr = dc * hc * r * (1 - r)
        dGi[:, t] = np.concatenate([dr, dz, dc], 1)
        dGh[:, t] = np.concatenate([dr, dz, dc * r], 1)
        dh = dGh[:, t] @ W_hh + d * z
    return dGi, dGh


def gru_param_grads(X, sv, dGi, dGh, W_ih, dtype=np.float64):
    X, W_ih = np.asarray(X, dtype), np.asarray(W_ih, dtype)
    E, H3 = X.shape[2], dGi.shape[2]
    gi, gh = dGi.reshape(-1, H3), dGh.reshape(-1, H3)
    return dict(weight_ih=gi.T @ X.reshape(-1, E), weight_hh=gh.T @ sv["hp"].reshape(-1, H3 // 3), bias_ih=gi.sum(0),
                bias_hh=gh.sum(0), dX=(gi @ W_ih).reshape(X.shape))


# ---------------------------------------------------------------- auxiliary loss (net.py:219-254)
def aux_fwd(gru_out, hist, neg, dtype=np.float64):
    go, hist, neg = (np.asarray(a, dtype) for a in (gru_out, hist, neg))
    B = go.shape[0]
    p = (go[:, :-1] * hist[:, 1:]).sum(2)
    n = (go[:, :-1] * neg[:, 1:]).sum(2)
    terms = np.log(dtype(EPS) + sigmoid(np.clip(n, -15, 15))) + np.log(dtype(EPS) + sigmoid(p))
    return terms.sum() / dtype(B), (p, n)


def aux_bwd(gru_out, hist, neg, d_aux=1.0, dtype=np.float64):
    """-> (d_gru_out, d_hist contribution, d_neg), all [B,T,H]."""
    go, hist, neg = (np.asarray(a, dtype) for a in (gru_out, hist, neg))
    B = go.shape[0]
    _, (p, n) = aux_fwd(go, hist, neg, dtype)
    sp, sn = sigmoid(p), sigmoid(n)
    dp = dtype(d_aux) / dtype(B) * sp * (1 - sp) / (dtype(EPS) + sp)
    dn = np.where((n > -15) & (n < 15), dtype(d_aux) / dtype(B) * sn * (1 - sn) / (dtype(EPS) + sn), 0).astype(dtype)
    d_go, d_hist, d_neg = np.zeros_like(go), np.zeros_like(go), np.zeros_like(go)
    d_go[:, :-1] = dp[..., None] * hist[:, 1:] + dn[..., None] * neg[:, 1:]
    d_hist[:, 1:] = dp[..., None] * go[:, :-1]
    d_neg[:, 1:] = dn[..., None] * go[:, :-1]
    return d_go, d_hist, d_neg


# ---------------------------------------------------------------- attention over positions (net.py:192-209)
def attention_fwd(hist, q, mask, att_w, att_b, dtype=np.float64):
    hist, q, mask = (np.asarray(a, dtype) for a in (hist, q, mask))
    att_w, att_b = [np.asarray(a, dtype) for a in att_w], [np.asarray(a, dtype) for a in att_b]
    B, T, E = hist.shape
    feat = np.concatenate([hist, q, hist - q, hist * q], 2)
    a1 = sigmoid(feat @ att_w[0] + att_b[0])
    a2 = sigmoid(a1 @ att_w[1] + att_b[1])
    score = (a2 @ att_w[2] + att_b[2]).reshape(B, T)
    # the reference adds the -1e9 mask in float32, where the sum rounds to -1e9 whatever the score is (that is what makes
    # a row masked everywhere come out uniform): masked positions take that float32 sum in every dtype
    m = mask.reshape(B, T)
    s = np.where(m != 0, (score.astype(np.float32) + m.astype(np.float32)).astype(dtype), score + m)
    s = s * dtype(E) ** dtype(-0.5)
    e = np.exp(s - s.max(1, keepdims=True))
    w = e / e.sum(1, keepdims=True)
    return w, w[..., None] * hist, (feat, a1, a2)


def attention_bwd(hist, q, w, saved, att_w, dx_att, dtype=np.float64):
    """-> (d_hist contribution, d_q, dscore)."""
    hist, q, w, dx_att = (np.asarray(a, dtype) for a in (hist, q, w, dx_att))
    att_w = [np.asarray(a, dtype) for a in att_w]
    _, a1, a2 = saved
    B, T, E = hist.shape
    g = (dx_att * hist).sum(2)
    dscore = dtype(E) ** dtype(-0.5) * (w * (g - (w * g).sum(1, keepdims=True)))
    d_hist = w[..., None] * dx_att
    d2 = (dscore.reshape(B, T, 1) @ att_w[2].T) * a2 * (1 - a2)
    d1 = (d2 @ att_w[1].T) * a1 * (1 - a1)
    df = d1 @ att_w[0].T
    d_hist = d_hist + df[..., :E] + df[..., 2 * E:3 * E] + df[..., 3 * E:] * q
    d_q = df[..., E:2 * E] - df[..., 2 * E:3 * E] + df[..., 3 * E:] * hist
    return d_hist, d_q, dscore


# ---------------------------------------------------------------- the whole net
def _gru_p(p, pat, dtype):
    return [np.asarray(p[pat % k], dtype) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def forward(p, att, feeds, dtype=np.float64):
    """p: state_dict arrays; att = (weights, biases) of the attention MLP; feeds: the ten arrays of create_feeds.
    -> dict(logit, aux, loss, cost, pred) + what backward() needs."""
    hi, hc, ti, tc, label, mask, tis, tcs, ni, nc = feeds
    f = lambda name, ids: lookup(np.asarray(p[name + ".weight"], dtype), np.asarray(ids))
    hist = np.concatenate([f("hist_item_emb_attr", hi), f("hist_cat_emb_attr", hc)], 2)
    neg = np.concatenate([f("neg_item_seq_emb_attr", ni), f("neg_cat_seq_emb_attr", nc)], 2)
    q = np.concatenate([f("target_item_seq_emb_attr", tis), f("target_cat_seq_emb_attr", tcs)], 2)
    tgt = np.concatenate([f("target_item_emb_attr", np.asarray(ti).reshape(-1)),
                          f("target_cat_emb_attr", np.asarray(tc).reshape(-1))], 1)
    B, T, E = hist.shape
    h0, sv0 = gru_fwd(hist, *_gru_p(p, GRUS[0], dtype), dtype=dtype)
    h1, sv1 = gru_fwd(h0, *_gru_p(p, GRUS[1], dtype), dtype=dtype)
    w, x_att, att_saved = attention_fwd(hist, q, np.asarray(mask).reshape(B, T), att[0], att[1], dtype)
    aux, _ = aux_fwd(h1, hist, neg, dtype)
    ha, sva = gru_fwd(x_att, *_gru_p(p, GRUS[2], dtype), dtype=dtype)
    emb = np.concatenate([ha[:, -1], tgt], 1)
    W = [np.asarray(p["linear_%d.weight" % i], dtype) for i in range(3)]
    b = [np.asarray(p["linear_%d.bias" % i], dtype) for i in range(3)]
    x1 = sigmoid(emb @ W[0] + b[0])
    x2 = sigmoid(x1 @ W[1] + b[1])
    item_b = np.asarray(p["item_b_attr.weight"], dtype)[np.asarray(ti).reshape(-1)]       # no padding row
    logit = x2 @ W[2] + b[2] + item_b
    y = np.asarray(label, dtype).reshape(B, 1)
    loss = (np.maximum(logit, 0) - logit * y + np.log1p(np.exp(-np.abs(logit)))).mean()
    return dict(logit=logit, aux=aux, loss=loss, cost=loss + aux, pred=sigmoid(logit), hist=hist, neg=neg, q=q, tgt=tgt,
                h0=h0, h1=h1, sv0=sv0, sv1=sv1, sva=sva, w=w, x_att=x_att, att_saved=att_saved, emb=emb, x1=x1, x2=x2, y=y)


def backward(p, att, feeds, fw, dtype=np.float64):
    """Gradients of cost = BCE + aux w.r.t. every entry of state_dict (tables as dense arrays; row 0 of the eight padded
    tables stays zero)."""
    hi, hc, ti, tc, label, mask, tis, tcs, ni, nc = (np.asarray(a) for a in feeds)
    B, T, E = fw["hist"].shape
    Ei = np.asarray(p["hist_item_emb_attr.weight"]).shape[1]
    W = [np.asarray(p["linear_%d.weight" % i], dtype) for i in range(3)]
    g = {}
    dz = (fw["pred"] - fw["y"]) / dtype(B)
    g["linear_2.weight"], g["linear_2.bias"] = fw["x2"].T @ dz, dz.sum(0)
    d2 = (dz @ W[2].T) * fw["x2"] * (1 - fw["x2"])
    g["linear_1.weight"], g["linear_1.bias"] = fw["x1"].T @ d2, d2.sum(0)
    d1 = (d2 @ W[1].T) * fw["x1"] * (1 - fw["x1"])
    g["linear_0.weight"], g["linear_0.bias"] = fw["emb"].T @ d1, d1.sum(0)
    de = d1 @ W[0].T
    # attention GRU: only the last state is used
    Wa = _gru_p(p, GRUS[2], dtype)
    dGi, dGh = gru_bwd(fw["sva"], Wa[1], dh_T=de[:, :E], dtype=dtype)
    ga = gru_param_grads(fw["x_att"], fw["sva"], dGi, dGh, Wa[0], dtype)
    d_hist, d_q, _ = attention_bwd(fw["hist"], fw["q"], fw["w"], fw["att_saved"], att[0], ga["dX"], dtype)
    d_go, dh_aux, d_neg = aux_bwd(fw["h1"], fw["hist"], fw["neg"], 1.0, dtype)
    d_hist = d_hist + dh_aux
    W1, W0 = _gru_p(p, GRUS[1], dtype), _gru_p(p, GRUS[0], dtype)
    dGi, dGh = gru_bwd(fw["sv1"], W1[1], dH_out=d_go, dtype=dtype)
    g1 = gru_param_grads(fw["h0"], fw["sv1"], dGi, dGh, W1[0], dtype)
    dGi, dGh = gru_bwd(fw["sv0"], W0[1], dH_out=g1["dX"], dtype=dtype)
    g0 = gru_param_grads(fw["hist"], fw["sv0"], dGi, dGh, W0[0], dtype)
    d_hist = d_hist + g0["dX"]
    for pat, gg in zip(GRUS, (g0, g1, ga)):
        for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            g[pat % k] = gg[k]

    def table(name, ids, grad, pad=0):
        out = np.zeros(np.asarray(p[name + ".weight"]).shape, dtype)
        ids, grad = ids.reshape(-1), grad.reshape(ids.size, -1)
        keep = ids != pad if pad is not None else np.ones(ids.shape, bool)
        np.add.at(out, ids[keep], grad[keep])
        g[name + ".weight"] = out

    table("hist_item_emb_attr", hi, d_hist[..., :Ei])
    table("hist_cat_emb_attr", hc, d_hist[..., Ei:])
    table("target_item_seq_emb_attr", tis, d_q[..., :Ei])
    table("target_cat_seq_emb_attr", tcs, d_q[..., Ei:])
    table("neg_item_seq_emb_attr", ni, d_neg[..., :Ei])
    table("neg_cat_seq_emb_attr", nc, d_neg[..., Ei:])
    table("target_item_emb_attr", ti, de[:, E:E + Ei])
    table("target_cat_emb_attr", tc, de[:, E + Ei:])
    table("item_b_attr", ti, dz, pad=None)
    g["_d_hist"], g["_d_q"], g["_d_neg"] = d_hist, d_q, d_neg
    return g


def sgd_step(p, grads, lr, dtype=np.float64):
    return {k: np.asarray(v, dtype) - dtype(lr) * grads[k] for k, v in p.items()}


def relerr(got, ref):
    """max|got - ref| / max|ref| — the error measure of the DIEN tests."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))
