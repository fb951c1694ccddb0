"""ENSFM (models/recall/ensfm) in numpy, in a chosen dtype: forward, backward and Paddle's Adagrad — TEST INFRASTRUCTURE ONLY.

Written in the reference's own, materialising formulation (net.py:63-98: the [B, I+1, C] `dot`, the three [B, P, C] tensors;
dygraph_model.py:40-51: the two [n, C, C] outer-product stacks), and the backward by the chain rule through those same
tensors, so it is a statement of the maths that shares nothing with the fused kernels."""
import numpy as np

TABLES = ("user_feature_emb.weight", "all_item_feature_emb.weight", "user_bias.weight", "item_bias.weight")
DENSE = ("H_i", "H_s", "bias")
PARAMS = TABLES + DENSE
ACC_INIT, EPS = 1e-8, 1e-6
FWD = ("loss", "pre", "pos_r", "q_emb", "p_emb")


def relerr(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


def load_golden(path):
    g = dict(np.load(path))
    p = {k: g["p_" + k] for k in PARAMS}
    return g, p, float(g["lr"][0]), float(g["w"][0]), int(g["steps"][0])


def forward(p, u, attr, ur=None, dtype=np.float64):
    """net.py:63-98 -> dict(pre, and with ur: pos_r, q_emb, p_emb, h, plus what the backward needs)."""
    P = {k: np.asarray(v, dtype) for k, v in p.items()}
    U, V, Hi, Hs = P["user_feature_emb.weight"], P["all_item_feature_emb.weight"], P["H_i"], P["H_s"]
    ue, ve = U[u], V[attr]                                             # [B, Fu, D], [I+1, Fi, D]
    su, sv = ue.sum(1), ve.sum(1)
    ucross, icross = dtype(0.5) * (su ** 2 - (ue ** 2).sum(1)), dtype(0.5) * (sv ** 2 - (ve ** 2).sum(1))
    ub, ib = P["user_bias.weight"][u].sum(1), P["item_bias.weight"][attr].sum(1)     # [B, 1], [I+1, 1]
    p_emb = np.concatenate([su, ucross @ Hs + ub + P["bias"], np.ones((len(u), 1), dtype)], 1)
    q_emb = np.concatenate([sv, np.ones((len(attr), 1), dtype), icross @ Hs + ib], 1)
    h = np.concatenate([Hi, np.ones((2, 1), dtype)], 0)                # [C, 1]
    dot = p_emb[:, None, :] * q_emb[None, :, :]                        # [B, I+1, C]: net.py:87
    pre = (dot @ h)[:, :, 0]
    c = dict(pre=pre, p_emb=p_emb, q_emb=q_emb, h=h, ue=ue, ve=ve, su=su, sv=sv, ucross=ucross, icross=icross)
    if ur is None:
        return c
    mask = (ur != len(attr) - 1).astype(dtype)                         # net.py:93
    pos_item = q_emb[ur] * mask[:, :, None]                            # [B, P, C]
    pos3 = p_emb[:, None, :] * pos_item                                # [B, P, C]
    c.update(pos_r=(pos3 @ h)[:, :, 0], pos_item=pos_item, pos3=pos3, mask=mask)
    return c


def loss_of(c, w, dtype=np.float64):
    """dygraph_model.py:40-51."""
    w = dtype(w)
    qq = (c["q_emb"][:, :, None] * c["q_emb"][:, None, :]).sum(0)      # [C, C]
    pp = (c["p_emb"][:, :, None] * c["p_emb"][:, None, :]).sum(0)
    hh = c["h"] @ c["h"].T
    loss = w * (qq * pp * hh).sum(0).sum(0)
    loss = loss + ((dtype(1.0) - w) * np.square(c["pos_r"]) - dtype(2.0) * c["pos_r"]).sum()
    c.update(qq=qq, pp=pp, hh=hh)
    return loss


def backward(p, c, u, attr, ur, w, dtype=np.float64):
    """The gradients of loss_of through forward's tensors -> {state_dict key: dense gradient}."""
    w = dtype(w)
    P = {k: np.asarray(v, dtype) for k, v in p.items()}
    D = P["H_i"].shape[0]
    p_emb, q_emb, h = c["p_emb"], c["q_emb"], c["h"]
    d_pos_r = (dtype(2.0) * (dtype(1.0) - w) * c["pos_r"] - dtype(2.0))             # [B, P]
    d_pos3 = d_pos_r[:, :, None] * h[None, None, :, 0]                              # [B, P, C]
    d_h = (d_pos_r[:, :, None] * c["pos3"]).sum((0, 1))[:, None]                    # [C, 1]
    d_p = (d_pos3 * c["pos_item"]).sum(1)
    d_pos_item = d_pos3 * p_emb[:, None, :]
    d_q = np.zeros_like(q_emb)
    np.add.at(d_q, ur.reshape(-1), (d_pos_item * c["mask"][:, :, None]).reshape(-1, q_emb.shape[1]))
    # the whole-data term: w sum(qq * pp * hh)
    d_qq, d_pp, d_hh = w * c["pp"] * c["hh"], w * c["qq"] * c["hh"], w * c["qq"] * c["pp"]
    d_q = d_q + q_emb @ (d_qq + d_qq.T)
    d_p = d_p + p_emb @ (d_pp + d_pp.T)
    d_h = d_h + (d_hh + d_hh.T) @ h
    g = {"H_i": d_h[:D]}

    def tower(d_out, score_col, ids, e, s, cross, table, bias_table):
        ds, dscore = d_out[:, :D], d_out[:, score_col:score_col + 1]               # the constant column takes nothing
        d_cross = dscore * P["H_s"].T                                               # [n, D]
        d_e = ds[:, None, :] + d_cross[:, None, :] * (s[:, None, :] - e)            # [n, F, D]
        gt, gb = np.zeros_like(P[table]), np.zeros_like(P[bias_table])
        np.add.at(gt, ids.reshape(-1), d_e.reshape(-1, D))
        np.add.at(gb, ids.reshape(-1), np.repeat(dscore, ids.shape[1], 0))
        return gt, gb, cross.T @ dscore, dscore.sum().reshape(1)

    gU, gub, gHs_u, gbias = tower(d_p, D, u, c["ue"], c["su"], c["ucross"], "user_feature_emb.weight", "user_bias.weight")
    gV, gib, gHs_i, _ = tower(d_q, D + 1, attr, c["ve"], c["sv"], c["icross"], "all_item_feature_emb.weight", "item_bias.weight")
    g.update({"user_feature_emb.weight": gU, "user_bias.weight": gub, "all_item_feature_emb.weight": gV, "item_bias.weight": gib,
              "H_s": gHs_u + gHs_i, "bias": gbias})
    return g


def adagrad_step(p, grads, lr, acc=None, dtype=np.float64):
    """paddle.optimizer.Adagrad(lr, initial_accumulator_value=1e-8), epsilon 1e-6, over every parameter:
    acc += g^2;  p -= lr g / (sqrt(acc) + eps).  -> (new parameters, new accumulators)."""
    new, nacc = {}, {}
    for k in p:
        a = np.full(np.shape(p[k]), ACC_INIT, dtype) if acc is None else np.asarray(acc[k], dtype)
        g = np.asarray(grads[k], dtype).reshape(np.shape(p[k]))
        nacc[k] = a + g * g
        new[k] = np.asarray(p[k], dtype) - dtype(lr) * g / (np.sqrt(nacc[k]) + dtype(EPS))
    return new, nacc


def train_step(p, u, attr, ur, w, lr, acc=None, dtype=np.float64):
    """-> (forward dict with loss, gradients, new parameters, new accumulators)."""
    c = forward(p, u, attr, ur, dtype)
    c["loss"] = np.asarray(loss_of(c, w, dtype)).reshape(1)
    g = backward(p, c, u, attr, ur, w, dtype)
    new, nacc = adagrad_step(p, g, lr, acc, dtype)
    return c, g, new, nacc
