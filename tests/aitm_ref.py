"""NumPy restatement of AITM (models/multitask/aitm: net.py, dygraph_model.py) and of the kernels of csrc/aitm_ops.hip — TEST
INFRASTRUCTURE ONLY.  float64 by default; dtype=np.float32 evaluates the same formulas in float32 (the error of that
evaluation against float64 is what the tests' tolerance is made of).  The matrix product and relerr are tests/mtl_ref.py's.

A net is known from its state_dict (the reference's names): embedding_dict.{i}.weight [vocab_i, D] in CONFIG order,
click_tower / conversion_tower .layer.{0,3,6}.{weight,bias}, attention_layer.{q,k,v}_layer.weight (no bias), info_layer.0,
click_layer.0, conversion_layer.0.  Dropout sites, in forward order: "click0" "click1" "click2" "conv0" "conv1" "conv2" "info";
masks = {site: keep-and-scale factor array of the site's shape} (absent: no dropout there)."""
import numpy as np

from mtl_ref import mm, relerr  # noqa: F401

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
CONSTRAINT_W, L2 = 0.6, 1e-6
LOG_CLAMP, BCE_GRAD_FLOOR = -100.0, 1e-12
SITES = ("click0", "click1", "click2", "conv0", "conv1", "conv2", "info")


# ------------------------------------------------------------------------------------------------ the kernels
def field_begin_of(vocab):
    return np.concatenate([[0], np.cumsum(np.asarray(vocab, np.int64))]).astype(np.int64)


def gather(W, field_begin, ids, dtype=np.float64):
    """W [sum vocab, D], ids [B, F] -> (out [B, F*D], rows [B*F] (-1: outside its field), flagged)."""
    W, ids, fb = np.asarray(W, dtype), np.asarray(ids), np.asarray(field_begin, np.int64)
    B, F = ids.shape
    ok = (ids >= 0) & (ids < (fb[1:] - fb[:-1])[None, :])
    rows = np.where(ok, ids + fb[None, :-1], -1)
    out = np.where(ok[:, :, None], W[np.where(ok, rows, 0)], dtype(0))
    return out.reshape(B, F * W.shape[1]), rows.reshape(-1), bool((~ok).any())


def gather_bwd(dX, rows, N, dtype=np.float64):
    """The dense table gradient [N, D]: lookup i adds row i of dX viewed as [B*F, D] to its row, in flattened order."""
    d = np.asarray(dX, dtype).reshape(len(rows), -1)
    g = np.zeros((N, d.shape[1]), dtype)
    for i, r in enumerate(rows):
        if r >= 0:
            g[r] = g[r] + d[i]
    return g


def dot(a, b):
    """sum over the last axis of a * b.  In float32 every product is rounded and the sum runs left to right in float32, as
    in mtl_ref.mm: the float32 evaluation with the least help (NumPy's own sum is pairwise)."""
    if a.dtype != np.float32:
        return (a * b).sum(-1)
    return np.add.accumulate(a * b, axis=-1, dtype=np.float32)[..., -1]


def ait_fwd(QKV, T, dtype=np.float64):
    """QKV [B*T, 3d] -> (out [B, d], prob [B, T])."""
    x = np.asarray(QKV, dtype)
    d = x.shape[1] // 3
    x = x.reshape(-1, T, 3 * d)
    Q, K, V = x[:, :, :d], x[:, :, d:2 * d], x[:, :, 2 * d:]
    s = dot(Q, K) * (dtype(1) / np.sqrt(dtype(d)))
    e = np.exp(s - s.max(1, keepdims=True))
    a = e / e.sum(1, keepdims=True)
    out = np.zeros((len(x), d), dtype)
    for t in range(T):
        out = out + a[:, t:t + 1] * V[:, t]
    return out, a


def ait_bwd(QKV, prob, d_out, T, dtype=np.float64):
    """-> dQKV [B*T, 3d]."""
    x, a, g = np.asarray(QKV, dtype), np.asarray(prob, dtype), np.asarray(d_out, dtype)
    d = x.shape[1] // 3
    x = x.reshape(-1, T, 3 * d)
    Q, K, V = x[:, :, :d], x[:, :, d:2 * d], x[:, :, 2 * d:]
    da = dot(np.broadcast_to(g[:, None, :], V.shape), V)
    ds = a * (da - dot(a, da)[:, None]) * (dtype(1) / np.sqrt(dtype(d)))
    out = np.concatenate([ds[:, :, None] * K, ds[:, :, None] * Q, a[:, :, None] * g[:, None, :]], 2)
    return out.reshape(-1, 3 * d)


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-z))


def bce(p, y, dtype):
    with np.errstate(divide="ignore"):
        return -(y * np.maximum(np.log(p), dtype(LOG_CLAMP)) + (1 - y) * np.maximum(np.log(1 - p), dtype(LOG_CLAMP)))


def head(tc, ait, w_click, b_click, w_conv, b_conv, click, buy, constraint_w=CONSTRAINT_W, grad_scale=1.0, dtype=np.float64):
    """-> (pred [B, 2] = pCTR | pCVR, cost [B, 3] = BCE click | BCE buy | max(pCVR - pCTR, 0), dz [B, 2])."""
    tc, ait = np.asarray(tc, dtype), np.asarray(ait, dtype)
    z0 = mm(tc, np.asarray(w_click, dtype).reshape(-1, 1))[:, 0] + np.asarray(b_click, dtype).reshape(-1)[0]
    z1 = mm(ait, np.asarray(w_conv, dtype).reshape(-1, 1))[:, 0] + np.asarray(b_conv, dtype).reshape(-1)[0]
    p = np.stack([sigmoid(z0), sigmoid(z1)], 1).astype(dtype)
    y = np.stack([np.asarray(click).reshape(-1), np.asarray(buy).reshape(-1)], 1).astype(dtype)
    over = p[:, 1] > p[:, 0]
    cost = np.concatenate([bce(p, y, dtype), np.where(over, p[:, 1] - p[:, 0], dtype(0))[:, None]], 1)
    s = p * (1 - p)
    g = dtype(grad_scale) * ((p - y) / np.maximum(s, dtype(np.float32(BCE_GRAD_FLOOR))))
    h = np.where(over, dtype(constraint_w), dtype(0))
    g = g + np.stack([-h, h], 1)
    return p, cost, g * s


def loss_of(cost, constraint_w=CONSTRAINT_W, dtype=np.float64):
    c = np.asarray(cost, dtype)
    return c[:, 0].mean() + c[:, 1].mean() + dtype(constraint_w) * c[:, 2].sum()


def auc_histogram(pred, label, num_thresholds):
    p = np.asarray(pred, np.float32).reshape(-1)
    t = np.asarray(label).reshape(-1)
    bucket = np.clip((p * np.float32(num_thresholds)).astype(np.int64), 0, num_thresholds)
    return (np.bincount(bucket[t != 0], minlength=num_thresholds + 1).astype(np.int64),
            np.bincount(bucket[t == 0], minlength=num_thresholds + 1).astype(np.int64))


# ------------------------------------------------------------------------------------------------ the net
def tables(p):
    F = sum(1 for k in p if k.startswith("embedding_dict."))
    return [p["embedding_dict.%d.weight" % i] for i in range(F)]


def _tower_fwd(p, name, x, masks, site, dtype):
    acts, h = [], x
    for j in range(3):
        acts.append(h)
        h = np.maximum(mm(h, np.asarray(p["%s.layer.%d.weight" % (name, 3 * j)], dtype))
                       + np.asarray(p["%s.layer.%d.bias" % (name, 3 * j)], dtype), 0)
        if site + str(j) in masks:
            h = h * np.asarray(masks[site + str(j)], dtype)
    return h, acts


def _tower_bwd(p, g, name, d, out, acts, masks, site, dtype):
    """d: gradient by the tower's output `out` (after ReLU and dropout) -> gradient by the tower's input."""
    outs = acts[1:] + [out]
    for j in (2, 1, 0):
        if site + str(j) in masks:
            d = d * np.asarray(masks[site + str(j)], dtype)
        d = np.where(outs[j] > 0, d, dtype(0))
        g["%s.layer.%d.weight" % (name, 3 * j)] = mm(acts[j].T, d)
        g["%s.layer.%d.bias" % (name, 3 * j)] = d.sum(0)
        d = mm(d, np.asarray(p["%s.layer.%d.weight" % (name, 3 * j)], dtype).T)
    return d


def train_step(p, ids, click, buy, lr, state=None, masks=None, constraint_w=CONSTRAINT_W, l2=L2, dtype=np.float64):
    """-> (forward record {pred, cost, loss, ...}, gradients WITH the L2 term g + l2 w (what the optimizer applies),
    parameters after Adam, optimizer state)."""
    masks = masks or {}
    w = lambda k: np.asarray(p[k], dtype)
    ids = np.asarray(ids)
    B = len(ids)
    tabs = tables(p)
    fb = field_begin_of([len(t) for t in tabs])
    x, rows, flagged = gather(np.concatenate(tabs, 0), fb, ids, dtype)
    tc, acts_c = _tower_fwd(p, "click_tower", x, masks, "click", dtype)
    tv, acts_v = _tower_fwd(p, "conversion_tower", x, masks, "conv", dtype)
    info = np.maximum(mm(tc, w("info_layer.0.weight")) + w("info_layer.0.bias"), 0)
    if "info" in masks:
        info = info * np.asarray(masks["info"], dtype)
    d = tc.shape[1]
    X = np.stack([tv, info], 1).reshape(2 * B, d)
    Wqkv = np.concatenate([w("attention_layer.%s_layer.weight" % n) for n in "qkv"], 1)
    QKV = mm(X, Wqkv)
    ait, prob = ait_fwd(QKV, 2, dtype)
    pred, cost, dz = head(tc, ait, w("click_layer.0.weight"), w("click_layer.0.bias"), w("conversion_layer.0.weight"),
                          w("conversion_layer.0.bias"), click, buy, constraint_w, 1.0 / B, dtype)
    c = dict(pred=pred, cost=cost, loss=loss_of(cost, constraint_w, dtype), x=x, tc=tc, tv=tv, info=info, QKV=QKV, ait=ait,
             prob=prob, dz=dz, rows=rows, flagged=flagged)
    g = {}
    g["click_layer.0.weight"], g["click_layer.0.bias"] = mm(tc.T, dz[:, 0:1]), dz[:, 0:1].sum(0)
    g["conversion_layer.0.weight"], g["conversion_layer.0.bias"] = mm(ait.T, dz[:, 1:2]), dz[:, 1:2].sum(0)
    d_tc = mm(dz[:, 0:1], w("click_layer.0.weight").T)
    d_ait = mm(dz[:, 1:2], w("conversion_layer.0.weight").T)
    dQKV = ait_bwd(QKV, prob, d_ait, 2, dtype)
    gW = mm(X.T, dQKV)
    for i, n in enumerate("qkv"):
        g["attention_layer.%s_layer.weight" % n] = gW[:, i * d:(i + 1) * d]
    dX2 = mm(dQKV, Wqkv.T).reshape(B, 2, d)
    d_tv, d_info = dX2[:, 0], dX2[:, 1]
    if "info" in masks:
        d_info = d_info * np.asarray(masks["info"], dtype)
    d_info = np.where(info > 0, d_info, dtype(0))
    g["info_layer.0.weight"], g["info_layer.0.bias"] = mm(tc.T, d_info), d_info.sum(0)
    d_tc = d_tc + mm(d_info, w("info_layer.0.weight").T)
    dX = _tower_bwd(p, g, "click_tower", d_tc, tc, acts_c, masks, "click", dtype) \
        + _tower_bwd(p, g, "conversion_tower", d_tv, tv, acts_v, masks, "conv", dtype)
    c["dX"] = dX
    gt = gather_bwd(dX, rows, int(fb[-1]), dtype)
    for i in range(len(tabs)):
        g["embedding_dict.%d.weight" % i] = gt[fb[i]:fb[i + 1]]
    g = {k: np.asarray(v, dtype).reshape(np.shape(p[k])) + dtype(l2) * w(k) for k, v in g.items()}
    new, state = adam_step(p, g, lr, state, dtype)
    return c, g, new, state


def adam_step(p, g, lr, state=None, dtype=np.float64):
    """paddle.optimizer.Adam (non-lazy, beta 0.9 / 0.999, epsilon 1e-8) on gradients that already hold the L2 term.
    state: {'t', 'm', 'v'} of the steps before (None: the first step; not written).  -> (new parameters, new state)."""
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


def load_golden(path):
    """-> (the npz as a dict, the initial state_dict, lr, steps).  Step s: ids_s [B, F], click_s, buy_s [B], pred_s [B, 2]
    (pCTR | pCVR), loss_s [1], g_s_<key> (WITH the L2 term), n_s_<key>."""
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0])
