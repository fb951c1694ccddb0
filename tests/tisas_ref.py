"""NumPy restatement of the reference's TiSASRec (models/recall/tisas/net.py, dygraph_model.py) with a hand-written
backward, evaluated in float64 or float32 — TEST INFRASTRUCTURE ONLY, checked against the recordings of the reference's own
files (tests/golden/tisas_h1.npz, tisas_h2.npz; tools/make_golden_tisas.py).  The relation tensors [B, L, L, D] ARE formed
here, as in the reference: this is the statement the fused kernels are held to.

Every dropout site takes an explicit mask (already scaled: 1 / (1 - p) where kept, 0 where dropped; None = identity):
  emb [B*L, D]; pos_k, pos_v [B*L, D] (per sample); time_k, time_v [B*L*L, D]; per block n: att<n> [B*H*L, L], ffn1_<n>,
  ffn2_<n> [B*L, D].  The five input masks are shared by all blocks (net.py:244-258)."""
import numpy as np

from mtl_ref import relerr  # noqa: F401

NEG = -2 ** 32 + 1
LN_EPS = 1e-8
BETA1, BETA2, ADAM_EPS = 0.9, 0.98, 1e-8


def structural_zero(key):
    """K_w.bias of every block: a constant added to every key adds q_i . c to every score of row i, and softmax is shift
    invariant (the replaced scores do not see it either), so its gradient is zero in exact arithmetic and rounding noise
    in float32 — which Adam turns into a step of up to lr in either direction.  No two float32 evaluations agree on it;
    tests hold it to a noise bound (backward()'s kbias_scale) and to what the steps can move."""
    return key.startswith("attention_layers.") and key.endswith(".K_w.bias")


def _m(mask, shape, dtype):
    return None if mask is None else np.asarray(mask, dtype).reshape(shape)


def embed_fwd(table, ids, scale, mask=None, dtype=np.float64):
    """item_emb(ids) * scale, dropout, * (ids != 0) -> [n, D]."""
    ids = np.asarray(ids).reshape(-1)
    x = np.asarray(table, dtype)[ids] * dtype(scale)
    if mask is not None:
        x = x * _m(mask, x.shape, dtype)
    return x * (ids != 0)[:, None].astype(dtype)


def embed_bwd(d_out, ids, scale, mask=None, dtype=np.float64):
    """The gradient rows of table[ids] (zero for id 0: the padding row takes none)."""
    ids = np.asarray(ids).reshape(-1)
    g = np.asarray(d_out, dtype) * dtype(scale)
    if mask is not None:
        g = g * _m(mask, g.shape, dtype)
    return g * (ids != 0)[:, None].astype(dtype)


def ln_fwd(x, gamma, beta, eps=LN_EPS, r=None, row_ids=None, dtype=np.float64):
    """t = (x + r) * (row_ids != 0); y = LayerNorm(t) -> (y, t, mean, rstd)."""
    t = np.asarray(x, dtype) + (np.asarray(r, dtype) if r is not None else dtype(0))
    if row_ids is not None:
        t = t * (np.asarray(row_ids).reshape(-1) != 0)[:, None].astype(dtype)
    mu = t.mean(-1, dtype=dtype)
    var = ((t - mu[:, None]) ** 2).mean(-1, dtype=dtype)
    rstd = dtype(1) / np.sqrt(var + dtype(eps))
    y = (t - mu[:, None]) * rstd[:, None] * np.asarray(gamma, dtype) + np.asarray(beta, dtype)
    return y, t, mu, rstd


def ln_bwd(t, mean, rstd, gamma, dy, row_ids=None, extra=None, dtype=np.float64):
    """-> (d(x) = d(r), dgamma, dbeta); extra: a further gradient of t."""
    t, dy = np.asarray(t, dtype), np.asarray(dy, dtype)
    xhat = (t - np.asarray(mean, dtype)[:, None]) * np.asarray(rstd, dtype)[:, None]
    g = dy * np.asarray(gamma, dtype)
    dx = np.asarray(rstd, dtype)[:, None] * (g - g.mean(-1, dtype=dtype)[:, None] - xhat * (g * xhat).mean(-1, dtype=dtype)[:, None])
    if extra is not None:
        dx = dx + np.asarray(extra, dtype)
    if row_ids is not None:
        dx = dx * (np.asarray(row_ids).reshape(-1) != 0)[:, None].astype(dtype)
    return dx, (dy * xhat).sum(0, dtype=dtype), dy.sum(0, dtype=dtype)


def attn_fwd(q, k, v, tables, tm, log_seqs, H, scale, masks=None, dtype=np.float64):
    """net.py:85-164 after the projections.  q, k, v [B*L, D]; tables = (pos_k, pos_v [L, D], time_k, time_v [T, D]); tm
    [B, L, L]; log_seqs [B, L]; masks: {att [B*H*L, L], pos_k, pos_v [B*L, D], time_k, time_v [B*L*L, D]}.
    -> (out [B*L, D], lse [B, H, L], cache for attn_bwd)."""
    masks = masks or {}
    log_seqs, tm = np.asarray(log_seqs), np.asarray(tm)
    B, L = log_seqs.shape
    D = np.shape(q)[1]
    hd = D // H
    pos_k, pos_v, time_k, time_v = (np.asarray(t, dtype) for t in tables)
    sh4, sh5 = (B, L, H, hd), (B, L, L, H, hd)
    PK, PV = np.broadcast_to(pos_k, (B, L, D)), np.broadcast_to(pos_v, (B, L, D))
    TK, TV = time_k[tm], time_v[tm]                                               # the [B, L, L, D] relation tensors
    mk = {n: _m(masks.get(n), s, dtype) for n, s in (("pos_k", (B, L, D)), ("pos_v", (B, L, D)), ("time_k", (B, L, L, D)),
                                                     ("time_v", (B, L, L, D)), ("att", (B, H, L, L)))}
    if mk["pos_k"] is not None:
        PK = PK * mk["pos_k"]
    if mk["pos_v"] is not None:
        PV = PV * mk["pos_v"]
    if mk["time_k"] is not None:
        TK = TK * mk["time_k"]
    if mk["time_v"] is not None:
        TV = TV * mk["time_v"]
    q4 = np.asarray(q, dtype).reshape(sh4)
    KP4 = (np.asarray(k, dtype).reshape(B, L, D) + PK).reshape(sh4)
    VP4 = (np.asarray(v, dtype).reshape(B, L, D) + PV).reshape(sh4)
    TK5, TV5 = TK.reshape(sh5), TV.reshape(sh5)
    s = (np.einsum("bihd,bjhd->bhij", q4, KP4) + np.einsum("bihd,bijhd->bhij", q4, TK5)) * dtype(scale)
    replaced = (log_seqs == 0)[:, None, :, None] | (np.arange(L)[None, :] > np.arange(L)[:, None])[None, None]
    replaced = np.broadcast_to(replaced, s.shape)
    s = np.where(replaced, dtype(NEG), s)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    z = e.sum(-1, keepdims=True, dtype=dtype)
    a = e / z
    lse = (mx + np.log(z))[..., 0]
    ad = a if mk["att"] is None else a * mk["att"]
    out = np.einsum("bhij,bjhd->bihd", ad, VP4) + np.einsum("bhij,bijhd->bihd", ad, TV5)
    cache = dict(q4=q4, KP4=KP4, VP4=VP4, TK5=TK5, TV5=TV5, a=a, ad=ad, mk=mk, replaced=replaced, scale=scale, tm=tm,
                 T=time_k.shape[0], shape=(B, L, H, hd, D))
    return out.reshape(B * L, D), lse, cache


def attn_bwd(d_out, c, dtype=np.float64):
    """-> (dq, dk, dv [B*L, D], d_pos_k, d_pos_v [L, D], d_time_k, d_time_v [T, D])."""
    B, L, H, hd, D = c["shape"]
    mk = c["mk"]
    dO4 = np.asarray(d_out, dtype).reshape(B, L, H, hd)
    da = np.einsum("bihd,bjhd->bhij", dO4, c["VP4"]) + np.einsum("bihd,bijhd->bhij", dO4, c["TV5"])
    if mk["att"] is not None:
        da = da * mk["att"]
    a = c["a"]
    ds = a * (da - (a * da).sum(-1, keepdims=True, dtype=dtype))
    gs = np.where(c["replaced"], dtype(0), ds) * dtype(c["scale"])                # a replaced score has no gradient
    dq = np.einsum("bhij,bjhd->bihd", gs, c["KP4"]) + np.einsum("bhij,bijhd->bihd", gs, c["TK5"])
    dKP = np.einsum("bhij,bihd->bjhd", gs, c["q4"]).reshape(B, L, D)
    c["kbias_scale"] = float(np.einsum("bhij,bihd->hd", np.abs(gs), np.abs(c["q4"])).max())   # the terms that cancel in sum_j dK_j
    dVP = np.einsum("bhij,bihd->bjhd", c["ad"], dO4).reshape(B, L, D)
    dTK = np.einsum("bhij,bihd->bijhd", gs, c["q4"]).reshape(B, L, L, D)
    dTV = np.einsum("bhij,bihd->bijhd", c["ad"], dO4).reshape(B, L, L, D)
    d_pos_k = (dKP if mk["pos_k"] is None else dKP * mk["pos_k"]).sum(0, dtype=dtype)
    d_pos_v = (dVP if mk["pos_v"] is None else dVP * mk["pos_v"]).sum(0, dtype=dtype)
    if mk["time_k"] is not None:
        dTK = dTK * mk["time_k"]
    if mk["time_v"] is not None:
        dTV = dTV * mk["time_v"]
    d_time_k, d_time_v = np.zeros((c["T"], D), dtype), np.zeros((c["T"], D), dtype)
    np.add.at(d_time_k, c["tm"].reshape(-1), dTK.reshape(-1, D))
    np.add.at(d_time_v, c["tm"].reshape(-1), dTV.reshape(-1, D))
    return dq.reshape(B * L, D), dKP.reshape(B * L, D), dVP.reshape(B * L, D), d_pos_k, d_pos_v, d_time_k, d_time_v


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def head(feats, pos, neg, table, dtype=np.float64):
    """net.py:305-308 + dygraph_model.py:42-53 -> dict(loss, cnt, pl, nl, d_feats, coef_pos, coef_neg, row_loss)."""
    feats, table = np.asarray(feats, dtype), np.asarray(table, dtype)
    pos, neg = np.asarray(pos).reshape(-1), np.asarray(neg).reshape(-1)
    ep, en = table[pos], table[neg]
    pl, nl = (feats * ep).sum(-1, dtype=dtype), (feats * en).sum(-1, dtype=dtype)
    sel = pos != 0
    cnt = dtype(sel.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        row = np.where(sel, _softplus(-pl) + _softplus(nl), dtype(0)).astype(dtype)
        loss = _softplus(-pl)[sel].sum(dtype=dtype) / cnt + _softplus(nl)[sel].sum(dtype=dtype) / cnt
        cp = np.where(sel, (_sigmoid(pl) - 1) / cnt, 0).astype(dtype)
        cn = np.where(sel, _sigmoid(nl) / cnt, 0).astype(dtype)
    return dict(loss=dtype(loss), cnt=cnt, pl=pl, nl=nl, d_feats=cp[:, None] * ep + cn[:, None] * en, coef_pos=cp, coef_neg=cn,
                row_loss=row)


# ---------------------------------------------------------------------------------------------------- the whole net
def num_blocks(p):
    return 1 + max(int(k.split(".")[1]) for k in p if k.startswith("attention_layers."))


def _lin(x, w, b, dtype):
    return x @ np.asarray(w, dtype) + np.asarray(b, dtype)


def _conv(x, w, b, dtype):                       # Conv1D, kernel size 1: weight [C_out, C_in, 1]
    return x @ np.asarray(w, dtype)[:, :, 0].T + np.asarray(b, dtype)


def seq2feats(p, log_seqs, tm, H, masks=None, dtype=np.float64):
    """net.py:244-289 -> (log_feats [B*L, D], the record the backward needs)."""
    masks = masks or {}
    log_seqs = np.asarray(log_seqs)
    B, L = log_seqs.shape
    D = p["item_emb.weight"].shape[1]
    ids = log_seqs.reshape(-1)
    seqs = embed_fwd(p["item_emb.weight"], ids, np.sqrt(dtype(D)), masks.get("emb"), dtype)
    tables = (p["abs_pos_K_emb.weight"][:L], p["abs_pos_V_emb.weight"][:L], p["time_matrix_K_emb.weight"],
              p["time_matrix_V_emb.weight"])
    scale = 1.0 / np.sqrt(dtype(D // H))
    rec = dict(B=B, L=L, D=D, H=H, ids=ids, blocks=[], masks=masks)
    x, r, first = seqs, None, True                # the next layer norm's input is (x + r) * mask
    for n in range(num_blocks(p)):
        g = lambda name: p["%s.%d.%s" % (name.split("/")[0], n, name.split("/")[1])]
        Q, S, mu_a, rs_a = ln_fwd(x, g("attention_layernorms/weight"), g("attention_layernorms/bias"), LN_EPS, r,
                                  None if first else ids, dtype)
        q = _lin(Q, g("attention_layers/Q_w.weight"), g("attention_layers/Q_w.bias"), dtype)
        k = _lin(S, g("attention_layers/K_w.weight"), g("attention_layers/K_w.bias"), dtype)
        v = _lin(S, g("attention_layers/V_w.weight"), g("attention_layers/V_w.bias"), dtype)
        am = {s: masks.get(s) for s in ("pos_k", "pos_v", "time_k", "time_v")}
        am["att"] = masks.get("att%d" % n)
        M, lse, ac = attn_fwd(q, k, v, tables, tm, log_seqs, H, scale, am, dtype)
        U, T2, mu_f, rs_f = ln_fwd(Q, g("forward_layernorms/weight"), g("forward_layernorms/bias"), LN_EPS, M, None, dtype)
        h0 = _conv(U, g("forward_layers/conv1.weight"), g("forward_layers/conv1.bias"), dtype)
        m1, m2 = _m(masks.get("ffn1_%d" % n), h0.shape, dtype), _m(masks.get("ffn2_%d" % n), h0.shape, dtype)
        h = np.maximum(h0 if m1 is None else h0 * m1, 0)
        f = _conv(h, g("forward_layers/conv2.weight"), g("forward_layers/conv2.bias"), dtype)
        if m2 is not None:
            f = f * m2
        rec["blocks"].append(dict(Q=Q, S=S, mu_a=mu_a, rs_a=rs_a, first=first, q=q, k=k, v=v, M=M, lse=lse, ac=ac, U=U, T2=T2,
                                  mu_f=mu_f, rs_f=rs_f, h=h, m1=m1, m2=m2, f=f))
        x, r, first = f, U, False
    feats, T3, mu_l, rs_l = ln_fwd(x, p["last_layernorm.weight"], p["last_layernorm.bias"], LN_EPS, r, None if first else ids,
                                   dtype)
    rec.update(feats=feats, T3=T3, mu_l=mu_l, rs_l=rs_l, last_masked=not first, tables=tables, seqs=seqs)
    return feats, rec


def forward(p, log_seqs, tm, pos, neg, H, masks=None, dtype=np.float64):
    feats, rec = seq2feats(p, log_seqs, tm, H, masks, dtype)
    hd = head(feats, pos, neg, p["item_emb.weight"], dtype)
    rec.update(head=hd, pos=np.asarray(pos).reshape(-1), neg=np.asarray(neg).reshape(-1), loss=np.asarray(hd["loss"]).reshape(1),
               log_feats=feats.reshape(rec["B"], rec["L"], rec["D"]))
    return rec


def backward(p, rec, dtype=np.float64):
    """-> {state_dict key: gradient}, dense.  rec["kbias_scale"][key]: the noise scale of a structural_zero gradient."""
    g, hd, ids = {}, rec["head"], rec["ids"]
    D, L = rec["D"], rec["L"]
    gt = np.zeros(p["item_emb.weight"].shape, dtype)

    def scatter(rows_ids, rows):
        keep = rows_ids != 0
        np.add.at(gt, rows_ids[keep], rows[keep])

    scatter(rec["pos"], hd["coef_pos"][:, None] * rec["feats"])
    scatter(rec["neg"], hd["coef_neg"][:, None] * rec["feats"])
    dx, g["last_layernorm.weight"], g["last_layernorm.bias"] = ln_bwd(rec["T3"], rec["mu_l"], rec["rs_l"], p["last_layernorm.weight"],
                                                                      hd["d_feats"], ids if rec["last_masked"] else None, None,
                                                                      dtype)
    tabs = [np.zeros(np.shape(t), dtype) for t in rec["tables"]]
    for n in reversed(range(len(rec["blocks"]))):
        b = rec["blocks"][n]
        key = lambda name: "%s.%d.%s" % (name.split("/")[0], n, name.split("/")[1])
        w = lambda name: np.asarray(p[key(name)], dtype)
        df = dx if b["m2"] is None else dx * b["m2"]
        w2, w1 = w("forward_layers/conv2.weight")[:, :, 0], w("forward_layers/conv1.weight")[:, :, 0]
        g[key("forward_layers/conv2.weight")] = (df.T @ b["h"])[:, :, None]
        g[key("forward_layers/conv2.bias")] = df.sum(0, dtype=dtype)
        dh = (df @ w2) * (b["h"] > 0)
        if b["m1"] is not None:
            dh = dh * b["m1"]
        g[key("forward_layers/conv1.weight")] = (dh.T @ b["U"])[:, :, None]
        g[key("forward_layers/conv1.bias")] = dh.sum(0, dtype=dtype)
        dU = dh @ w1 + dx
        dT2, g[key("forward_layernorms/weight")], g[key("forward_layernorms/bias")] = ln_bwd(
            b["T2"], b["mu_f"], b["rs_f"], w("forward_layernorms/weight"), dU, None, None, dtype)
        dq, dk, dv, dpk, dpv, dtk, dtv = attn_bwd(dT2, b["ac"], dtype)
        rec.setdefault("kbias_scale", {})[key("attention_layers/K_w.bias")] = b["ac"]["kbias_scale"]
        for acc, d in zip(tabs, (dpk, dpv, dtk, dtv)):
            acc += d
        dS = np.zeros_like(dq)
        dQ = dT2.copy()
        for name, x, d in (("Q_w", b["Q"], dq), ("K_w", b["S"], dk), ("V_w", b["S"], dv)):
            g[key("attention_layers/%s.weight" % name)] = x.T @ d
            g[key("attention_layers/%s.bias" % name)] = d.sum(0, dtype=dtype)
            if name == "Q_w":
                dQ = dQ + d @ w("attention_layers/Q_w.weight").T
            else:
                dS = dS + d @ w("attention_layers/%s.weight" % name).T
        dx, g[key("attention_layernorms/weight")], g[key("attention_layernorms/bias")] = ln_bwd(
            b["S"], b["mu_a"], b["rs_a"], w("attention_layernorms/weight"), dQ, None if b["first"] else ids, dS, dtype)
    scatter(ids, embed_bwd(dx, ids, np.sqrt(dtype(D)), rec["masks"].get("emb"), dtype))
    g["item_emb.weight"] = gt
    for name, d in zip(("abs_pos_K_emb.weight", "abs_pos_V_emb.weight"), tabs[:2]):
        g[name] = np.zeros(p[name].shape, dtype)
        g[name][:L] = d
    g["time_matrix_K_emb.weight"], g["time_matrix_V_emb.weight"] = tabs[2], tabs[3]
    return g


def adam_step(p, g, lr, state=None, dtype=np.float64):
    """paddle.optimizer.Adam(beta1 0.9, beta2 0.98), non-lazy, epsilon 1e-8.  state: {'t', 'm', 'v'} or None."""
    st = dict(t=state["t"], m=dict(state["m"]), v=dict(state["v"])) if state is not None else dict(t=0, m={}, v={})
    st["t"] += 1
    t, new = st["t"], {}
    for k, wk in p.items():
        wk = np.asarray(wk, dtype)
        gk = np.asarray(g[k], dtype).reshape(wk.shape)
        m = st["m"][k] = dtype(BETA1) * np.asarray(st["m"].get(k, 0), dtype) + dtype(1 - BETA1) * gk
        v = st["v"][k] = dtype(BETA2) * np.asarray(st["v"].get(k, 0), dtype) + dtype(1 - BETA2) * gk * gk
        lr_t = dtype(lr) * np.sqrt(dtype(1 - BETA2 ** t)) / dtype(1 - BETA1 ** t)
        new[k] = wk - lr_t * m / (np.sqrt(v) + dtype(ADAM_EPS) * np.sqrt(dtype(1 - BETA2 ** t)))
    return new, st


def train_step(p, log_seqs, tm, pos, neg, H, lr, state=None, masks=None, dtype=np.float64):
    """-> (forward record, gradients, parameters after Adam, optimizer state)."""
    rec = forward(p, log_seqs, tm, pos, neg, H, masks, dtype)
    g = backward(p, rec, dtype)
    new, state = adam_step(p, g, lr, state, dtype)
    return rec, g, new, state


def infer(p, log_seqs, tm, item_indices, H, dtype=np.float64):
    """net.py:298-303: only row 0's candidates -> logits [B, I]."""
    feats, rec = seq2feats(p, log_seqs, tm, H, None, dtype)
    final = feats.reshape(rec["B"], rec["L"], rec["D"])[:, -1]
    return final @ np.asarray(p["item_emb.weight"], dtype)[np.asarray(item_indices)[0]].T


def ndcg_hr(logits):
    """infer.py: the rank of candidate 0 among the row's candidates -> (NDCG@10, HR@10) summed over the rows."""
    ndcg = hr = 0.0
    for row in np.asarray(logits):
        rank = int((-row).argsort().argsort()[0])
        if rank < 10:
            ndcg += 1 / np.log2(rank + 2)
            hr += 1
    return ndcg, hr


def load_golden(path):
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0])
