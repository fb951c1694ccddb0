"""numpy restatement of the reference's MatchPyramid (models/match/match-pyramid/net.py, dygraph_model.py) — TEST
INFRASTRUCTURE ONLY: the lookups, the interaction image, Conv2D("SAME"), ReLU, max_pool2d("VALID"), the two Linears, the
pairwise hinge, their gradients and Paddle's Adam, in the dtype asked for (float64: the yardstick; float32: what float32
arithmetic alone costs, the tolerance's unit).

Parameters are a dict under the reference's names: emb.weight [rows, E], conv.weight [K, 1, kh, kw], conv.bias, fc1.weight
[240, H], fc1.bias, fc2.weight [H, 1], fc2.bias.  The table may be any subset of the real one as long as the ids index IT: cfg
= dict(pad= the padding row of that table, filter=(kh, kw), pool=(ph, pw), stride=(sh, sw), relu=bool, pairs=64).

Rules that rest on Paddle's documentation, not on a Paddle run: "SAME" pads k - 1 per axis, floor((k - 1) / 2) in front; a
window's first maximum in row-major order takes the gradient; maximum(0, x) passes the gradient at x == 0."""
import numpy as np

B1, B2, EPS_ADAM = 0.9, 0.999, 1e-8


def relerr(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(float(np.abs(want).max()), 1e-30))


def same_pad(k):
    return (k - 1) // 2, (k - 1) - (k - 1) // 2


def pooled_shape(Ll, Lr, cfg):
    return (Ll - cfg["pool"][0]) // cfg["stride"][0] + 1, (Lr - cfg["pool"][1]) // cfg["stride"][1] + 1


def lookup(table, ids, pad, dt=np.float64):
    """[B, L, E]: a padding id, and an id outside the table, is a zero row."""
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < len(table)) & (ids != pad)
    return np.asarray(table, dt)[np.where(ok, ids, 0)] * ok[..., None].astype(dt), ok


def interaction_fwd(table, left, right, w, b, cfg, dt=np.float64):
    """-> dict(pooled [B, K * PH * PW], argmax int32 (cell i * Lr + j), and what the backward needs)."""
    (kh, kw), (ph, pw), (sh, sw) = cfg["filter"], cfg["pool"], cfg["stride"]
    L, okl = lookup(table, left, cfg["pad"], dt)
    R, okr = lookup(table, right, cfg["pad"], dt)
    B, Ll, Lr, K = L.shape[0], L.shape[1], R.shape[1], len(b)
    cross = np.matmul(L, R.transpose(0, 2, 1)).astype(dt)
    (pt, pb), (pl, pr) = same_pad(kh), same_pad(kw)
    xp = np.pad(cross, ((0, 0), (pt, pb), (pl, pr)))
    w, b = np.asarray(w, dt).reshape(K, kh, kw), np.asarray(b, dt)
    pre = np.broadcast_to(b[None, :, None, None], (B, K, Ll, Lr)).astype(dt).copy()
    for a in range(kh):
        for c in range(kw):
            pre += w[None, :, a, c, None, None] * xp[:, None, a:a + Ll, c:c + Lr]
    act = np.maximum(pre, dt(0)) if cfg["relu"] else pre
    PH, PW = pooled_shape(Ll, Lr, cfg)
    pooled, argmax = np.zeros((B, K, PH, PW), dt), np.zeros((B, K, PH, PW), np.int32)
    for p in range(PH):
        for q in range(PW):
            win = act[:, :, p * sh:p * sh + ph, q * sw:q * sw + pw].reshape(B, K, ph * pw)
            idx = win.argmax(-1)                                # the first of equals
            pooled[:, :, p, q] = np.take_along_axis(win, idx[..., None], -1)[..., 0]
            argmax[:, :, p, q] = (p * sh + idx // pw) * Lr + q * sw + idx % pw
    return dict(pooled=pooled.reshape(B, -1), argmax=argmax.reshape(B, -1), L=L, R=R, okl=okl, okr=okr, xp=xp, pre=pre, w=w)


def interaction_bwd(f, d_pooled, cfg, dt=np.float64):
    """-> dict(dL [B, Ll, E], dR [B, Lr, E], d_w [K, 1, kh, kw], d_b [K], d_cross)."""
    (kh, kw) = cfg["filter"]
    L, R, xp, pre, w = f["L"], f["R"], f["xp"], f["pre"], f["w"]
    B, K, Ll, Lr = pre.shape
    (pt, _), (pl, _) = same_pad(kh), same_pad(kw)
    d_act = np.zeros((B, K, Ll * Lr), dt)
    N = f["argmax"].shape[1] // K
    am = f["argmax"].reshape(B, K, N)
    bi, ki = np.meshgrid(np.arange(B), np.arange(K), indexing="ij")
    for n in range(N):                                          # a cell that wins several windows receives all of them
        np.add.at(d_act, (bi, ki, am[:, :, n]), np.asarray(d_pooled, dt).reshape(B, K, N)[:, :, n])
    d_pre = d_act.reshape(B, K, Ll, Lr)
    if cfg["relu"]:
        d_pre = d_pre * (pre > 0)
    d_w, d_xp = np.zeros((K, 1, kh, kw), dt), np.zeros_like(xp)
    for a in range(kh):
        for c in range(kw):
            d_w[:, 0, a, c] = (d_pre * xp[:, None, a:a + Ll, c:c + Lr]).sum((0, 2, 3), dtype=dt)
            d_xp[:, a:a + Ll, c:c + Lr] += (d_pre * w[None, :, a, c, None, None]).sum(1, dtype=dt)
    d_cross = d_xp[:, pt:pt + Ll, pl:pl + Lr]
    dL = np.matmul(d_cross, R) * f["okl"][..., None]
    dR = np.matmul(d_cross.transpose(0, 2, 1), L) * f["okr"][..., None]
    return dict(dL=dL.astype(dt), dR=dR.astype(dt), d_w=d_w, d_b=d_pre.sum((0, 2, 3), dtype=dt), d_cross=d_cross)


def hinge(pred, pairs, dt=np.float64):
    """-> (loss, d_pred [B]): mean_{r < pairs} max(0, 1 - pred[r] + pred[pairs + r]); the gradient flows at exactly 0."""
    pred = np.asarray(pred, dt).reshape(-1)
    x = dt(1) - pred[:pairs] + pred[pairs:2 * pairs]
    is_open = x >= 0
    d = np.zeros_like(pred)
    d[:pairs] = np.where(is_open, -dt(1) / dt(pairs), dt(0))
    d[pairs:2 * pairs] = np.where(is_open, dt(1) / dt(pairs), dt(0))
    return dt(np.where(is_open, x, dt(0)).sum(dtype=dt) / dt(pairs)), d, x


def forward(p, left, right, cfg, dt=np.float64):
    """-> dict(pred [B, 1], hid, and interaction_fwd's record)."""
    f = interaction_fwd(p["emb.weight"], left, right, p["conv.weight"], p["conv.bias"], cfg, dt)
    hid = np.maximum(f["pooled"] @ np.asarray(p["fc1.weight"], dt) + np.asarray(p["fc1.bias"], dt), dt(0))
    f["hid"], f["pred"] = hid, (hid @ np.asarray(p["fc2.weight"], dt) + np.asarray(p["fc2.bias"], dt)).astype(dt)
    return f


def loss_and_grads(p, left, right, cfg, dt=np.float64):
    """-> dict(loss [1], pred [B, 1], pooled, argmax, hinge (the hinge's arguments), dL, dR, g {name: gradient})."""
    f = forward(p, left, right, cfg, dt)
    loss, d_pred, x = hinge(f["pred"], cfg["pairs"], dt)
    d_pred = d_pred[:, None]
    g = {"fc2.weight": f["hid"].T @ d_pred, "fc2.bias": d_pred.sum(0, dtype=dt)}
    d_hid = (d_pred @ np.asarray(p["fc2.weight"], dt).T) * (f["hid"] > 0)
    g["fc1.weight"], g["fc1.bias"] = f["pooled"].T @ d_hid, d_hid.sum(0, dtype=dt)
    d_pooled = d_hid @ np.asarray(p["fc1.weight"], dt).T
    bw = interaction_bwd(f, d_pooled, cfg, dt)
    g["conv.weight"], g["conv.bias"] = bw["d_w"], bw["d_b"]
    ge = np.zeros(np.shape(p["emb.weight"]), dt)
    E = ge.shape[1]
    for ids, d, ok in ((left, bw["dL"], f["okl"]), (right, bw["dR"], f["okr"])):
        np.add.at(ge, np.where(ok, np.asarray(ids), 0).reshape(-1), d.reshape(-1, E))      # rows not ok carry zeros
    g["emb.weight"] = ge
    return dict(loss=np.asarray([loss]), pred=f["pred"], pooled=f["pooled"], argmax=f["argmax"], hinge=x, d_pooled=d_pooled,
                dL=bw["dL"], dR=bw["dR"], pre=f["pre"], g=g)


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


def train_step(p, m, v, left, right, cfg, step, lr, dt=np.float64):
    """-> loss_and_grads' dict plus n, m, v: the state after the step."""
    out = loss_and_grads(p, left, right, cfg, dt)
    if m is None:
        m = {k: np.zeros_like(np.asarray(x, dt)) for k, x in p.items()}
        v = {k: np.zeros_like(np.asarray(x, dt)) for k, x in p.items()}
    out["n"], out["m"], out["v"] = adam(p, out["g"], m, v, step, lr, dt)
    return out


def load_golden(path):
    """-> (arrays, starting parameters {name: array} with the table COMPACT (the rows `rows` of the real one, the padding row
    last), cfg for that table, lr, steps)."""
    g = dict(np.load(path))
    p = {k[2:]: v for k, v in g.items() if k.startswith("p_")}
    cfg = dict(pad=len(g["rows"]) - 1, filter=tuple(g["filter"]), pool=tuple(g["pool"]), stride=tuple(g["stride"]),
               relu=bool(g["relu"][0]), pairs=int(g["pairs"][0]))
    return g, p, cfg, float(g["lr"][0]), int(g["steps"][0])


def compact_ids(rows, ids):
    """Ids of the real table -> indices into its stored rows `rows` (ascending; every id must be among them)."""
    ids = np.asarray(ids)
    idx = np.searchsorted(rows, ids)
    assert (np.asarray(rows)[np.minimum(idx, len(rows) - 1)] == ids).all()
    return idx
