"""NumPy restatement of the entire-space multitask nets (models/multitask/esmm, escm2: net.py, dygraph_model.py) and of the
two rec_field_sumpool_fwd / rec_esm_head kernels — TEST INFRASTRUCTURE ONLY.  float64 by default; dtype=np.float32 evaluates
the same formulas in float32 (the error of that evaluation against float64 is what the tests' tolerance is made of).  The
matrix product, the mixture, Adam and relerr are tests/mtl_ref.py's.

A net is known from its state_dict: `expert_0.weight` present -> ESCM2 (an MMoE trunk, one gate / tower per task: 3 in the
DR mode, else 2), otherwise ESMM (linear_0 .. linear_{n_ctr} the ctr tower, the rest the cvr tower; the split is the first
Linear with two outputs).  cfg = dict(mode="ESMM" | "IPW" | "DR", global_w, counterfactual_w)."""
import numpy as np

import mtl_ref as M
from mtl_ref import adam_step, mm, relerr, softmax  # noqa: F401

LOG_EPS, CLIP_LO, CLIP_HI = 1e-4, 1e-15, 1.0 - 1e-15
ESMM_CFG = dict(mode="ESMM", global_w=1.0, counterfactual_w=0.0)


# ------------------------------------------------------------------------------------------------ the kernels
def pool(W, ids, padding_idx=0, dtype=np.float64):
    """W [N, D], ids [B, F, L] -> [B, F*D]: per (sample, field) the sum over l, ascending, from +0, of the rows whose id is
    neither padding_idx nor outside [0, N)."""
    W, ids = np.asarray(W, dtype), np.asarray(ids)
    B, F, L = ids.shape
    N, D = W.shape
    out = np.zeros((B, F, D), dtype)
    for l in range(L):
        i = ids[:, :, l]
        ok = (i != padding_idx) & (i >= 0) & (i < N)
        out = out + np.where(ok[:, :, None], W[np.where(ok, i, 0)], dtype(0))
    return out.reshape(B, F * D)


def pool_bwd(dX, ids, N, padding_idx=0, dtype=np.float64):
    """The dense table gradient [N, D]: every kept lookup (b, f, l) adds dX[b, f*D:(f+1)*D] to its row, in flattened order."""
    ids = np.asarray(ids)
    B, F, L = ids.shape
    d = np.asarray(dX, dtype).reshape(B, F, -1)
    g = np.zeros((N, d.shape[2]), dtype)
    for b in range(B):
        for f in range(F):
            for l in range(L):
                i = ids[b, f, l]
                if i != padding_idx and 0 <= i < N:
                    g[i] = g[i] + d[b, f]
    return g


def log_loss(x, lab, dtype):
    eps = dtype(LOG_EPS)
    return -lab * np.log(x + eps) - (1 - lab) * np.log(1 - x + eps)


def d_log_loss(x, lab, dtype):
    eps = dtype(LOG_EPS)
    return (1 - lab) / (1 - x + eps) - lab / (x + eps)


def head(logits, click, buy, mode, global_w=1.0, counterfactual_w=0.0, grad_scale=1.0, dtype=np.float64):
    """logits [B, 2G], click / buy [B] int -> (pred [B, 2G+2], cost [B, 3], dlogits [B, 2G]) — include/recengine.h,
    rec_esm_head.  The clip bounds are the float32 values a float32 tensor is clipped to (the upper one is 1); the softmax
    backward is autograd's p (g - sum g p), as in mtl_ref.head."""
    G = 3 if mode == "DR" else 2
    z = np.asarray(logits, dtype)
    B = len(z)
    p = softmax(z.reshape(B, G, 2), dtype)
    clip = mode != "ESMM"
    lo, hi = dtype(np.float32(CLIP_LO)), dtype(np.float32(CLIP_HI))
    q = np.clip(p, lo, hi) if clip else p
    opened = ((p[:, :, 1] >= lo) & (p[:, :, 1] <= hi)) if clip else np.ones((B, G), bool)
    click, buy = np.asarray(click).reshape(B), np.asarray(buy).reshape(B)
    y, t = click.astype(dtype), buy.astype(dtype)
    o = y
    p1, q1 = q[:, 0, 1], q[:, 1, 1]
    r = p1 * q1
    gw, cw, gs = dtype(global_w), dtype(counterfactual_w), dtype(grad_scale)
    c0, c2 = log_loss(p1, y, dtype), log_loss(r, t, dtype)
    c1, dq_cf, di = np.zeros(B, dtype), np.zeros(B, dtype), np.zeros(B, dtype)
    if mode == "IPW":
        n_click = dtype(int(click.sum()))
        ips = dtype(1) / np.maximum(p1 * n_click, dtype(np.float32(1e-6)))
        ips = np.clip(ips, dtype(-15), dtype(15)) * dtype(B)
        c1 = log_loss(q1, t, dtype) * ips * o
        dq_cf = d_log_loss(q1, t, dtype) * ips * o
    elif mode == "DR":
        i1 = q[:, 2, 1]
        e = log_loss(q1, t, dtype) - i1
        ips = np.clip(o / np.maximum(p1, dtype(np.float32(1e-6))), dtype(-15), dtype(15))
        c1 = (i1 + e * ips) + e * e * ips
        de = ips + 2 * e * ips
        dq_cf = d_log_loss(q1, t, dtype) * de
        di = 1 - de
    dr = gw * d_log_loss(r, t, dtype)
    d1 = np.zeros((B, G), dtype)
    d1[:, 0] = gs * (d_log_loss(p1, y, dtype) + dr * q1)
    d1[:, 1] = gs * (dr * p1 + cw * dq_cf)
    if G == 3:
        d1[:, 2] = gs * cw * di
    d1 = np.where(opened, d1, dtype(0))
    gv = np.stack([np.zeros_like(d1), d1], 2)
    dl = p * (gv - (gv * p).sum(2, keepdims=True))
    pred = np.concatenate([q.reshape(B, 2 * G), (1 - r)[:, None], r[:, None]], 1)
    return pred, np.stack([c0, c1, c2], 1), dl.reshape(B, 2 * G)


def outs_of(pred):
    """pred [B, 2G+2] -> net.py's out_list side by side [B, 9 or 10]: ctr_out, ctr_prop_one, cvr_out, cvr_prop_one, ctcvr_prop,
    ctcvr_prop_one and, with three tasks, imp_prop_one."""
    pred = np.asarray(pred)
    G = (pred.shape[1] - 2) // 2
    cols = [pred[:, 0:2], pred[:, 1:2], pred[:, 2:4], pred[:, 3:4], pred[:, 2 * G:2 * G + 2], pred[:, 2 * G + 1:2 * G + 2]]
    return np.concatenate(cols + ([pred[:, 5:6]] if G == 3 else []), 1)


def loss_of(cost, global_w, counterfactual_w, dtype=np.float64):
    c = np.asarray(cost, dtype)
    return c[:, 0].mean() + dtype(counterfactual_w) * c[:, 1].mean() + dtype(global_w) * c[:, 2].mean()


# ------------------------------------------------------------------------------------------------ the nets
def is_escm2(p):
    return "expert_0.weight" in p


def esmm_towers(p):
    """-> ([linear indices of the ctr tower], [of the cvr tower])."""
    n = sum(1 for k in p if k.startswith("linear_") and k.endswith(".weight"))
    first_out = next(i for i in range(n) if p["linear_%d.weight" % i].shape[1] == 2 and i + 1 < n)
    return list(range(first_out + 1)), list(range(first_out + 1, n))


def _mlp_fwd(p, x, idx, dtype):
    acts, h = [], x
    for j, i in enumerate(idx):
        acts.append(h)
        h = mm(h, np.asarray(p["linear_%d.weight" % i], dtype)) + np.asarray(p["linear_%d.bias" % i], dtype)
        if j + 1 < len(idx):
            h = np.maximum(h, 0)
    return h, acts


def _mlp_bwd(p, g, acts, dz, idx, dtype):
    d = dz
    for j in reversed(range(len(idx))):
        i = idx[j]
        g["linear_%d.weight" % i] = mm(acts[j].T, d)
        g["linear_%d.bias" % i] = d.sum(0)
        d = mm(d, np.asarray(p["linear_%d.weight" % i], dtype).T)
        if j > 0:
            d = np.where(acts[j] > 0, d, dtype(0))
    return d


def train_step(p, ids, click, buy, lr, cfg, state=None, dtype=np.float64):
    """-> (forward record {pred, cost, loss, z, x}, gradients, parameters after Adam, optimizer state)."""
    w = lambda k: np.asarray(p[k], dtype)
    ids = np.asarray(ids)
    B = len(ids)
    N = p["embedding.weight"].shape[0]
    x = pool(p["embedding.weight"], ids, 0, dtype)
    g = {}
    if is_escm2(p):
        E = sum(1 for k in p if k.startswith("expert_") and k.endswith(".weight"))
        G = sum(1 for k in p if k.startswith("gate_") and k.endswith(".weight"))
        S = p["expert_0.weight"].shape[1]
        sl = [list(range(E))] * G
        H = np.concatenate([np.maximum(mm(x, w("expert_%d.weight" % e)) + w("expert_%d.bias" % e), 0) for e in range(E)], 1)
        lg = np.concatenate([mm(x, w("gate_%d.weight" % i)) + w("gate_%d.bias" % i) for i in range(G)], 1)
        prob, mix = M.mix_fwd(H, lg, S, E, sl, dtype)
        acts, z = [], []
        for t in range(G):
            a = np.maximum(mm(mix[:, t * S:(t + 1) * S], w("tower_%d.weight" % t)) + w("tower_%d.bias" % t), 0)
            acts.append(a)
            z.append(mm(a, w("tower_out_%d.weight" % t)) + w("tower_out_%d.bias" % t))
        z = np.concatenate(z, 1)
    else:
        ctr, cvr = esmm_towers(p)
        z0, acts0 = _mlp_fwd(p, x, ctr, dtype)
        z1, acts1 = _mlp_fwd(p, x, cvr, dtype)
        z = np.concatenate([z0, z1], 1)
    pred, cost, dz = head(z, click, buy, cfg["mode"], cfg["global_w"], cfg["counterfactual_w"], 1.0 / B, dtype)
    c = dict(pred=pred, cost=cost, loss=loss_of(cost, cfg["global_w"], cfg["counterfactual_w"], dtype), z=z, x=x, dz=dz)
    if is_escm2(p):
        dmix = np.zeros((B, G * S), dtype)
        for t in range(G):
            dzt, a = dz[:, 2 * t:2 * t + 2], acts[t]
            g["tower_out_%d.weight" % t] = mm(a.T, dzt)
            g["tower_out_%d.bias" % t] = dzt.sum(0)
            wo = w("tower_out_%d.weight" % t)            # the two products rounded and added: mtl_ref.backward says why
            da = np.where(a > 0, dzt[:, 0:1] * wo[:, 0][None, :] + dzt[:, 1:2] * wo[:, 1][None, :], dtype(0))
            g["tower_%d.weight" % t] = mm(mix[:, t * S:(t + 1) * S].T, da)
            g["tower_%d.bias" % t] = da.sum(0)
            dmix[:, t * S:(t + 1) * S] = mm(da, w("tower_%d.weight" % t).T)
        dH, dl = M.mix_bwd(H, prob, dmix, S, E, sl, True, dtype)
        dX = np.zeros_like(x)
        for e in range(E):
            d = dH[:, e * S:(e + 1) * S]
            g["expert_%d.weight" % e], g["expert_%d.bias" % e] = mm(x.T, d), d.sum(0)
            dX = dX + mm(d, w("expert_%d.weight" % e).T)
        for i in range(G):
            d = dl[:, i * E:(i + 1) * E]
            g["gate_%d.weight" % i], g["gate_%d.bias" % i] = mm(x.T, d), d.sum(0)
            dX = dX + mm(d, w("gate_%d.weight" % i).T)
    else:
        dX = _mlp_bwd(p, g, acts0, dz[:, 0:2], ctr, dtype) + _mlp_bwd(p, g, acts1, dz[:, 2:4], cvr, dtype)
    c["dX"] = dX
    g["embedding.weight"] = pool_bwd(dX, ids, N, 0, dtype)
    new, state = adam_step(p, g, lr, state, dtype)
    return c, g, new, state


def cfg_of(g):
    """The head configuration a golden records (mode as a string array, the two weights)."""
    return dict(mode=str(g["mode"][0]), global_w=float(g["global_w"][0]), counterfactual_w=float(g["counterfactual_w"][0]))


def load_golden(path):
    """-> (the npz as a dict, the initial state_dict, lr, steps, cfg).  Step s: ids_s [B, F, L], click_s, buy_s [B],
    outs_s [B, 9 or 10] (outs_of), loss_s [1], g_s_<key>, n_s_<key>."""
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0]), cfg_of(g)
