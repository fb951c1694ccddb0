"""numpy restatement of the reference's DSSM (models/match/dssm/net.py, dygraph_model.py) — TEST INFRASTRUCTURE ONLY: the
two towers, Paddle's clamped cosine, the softmax, the sliced loss, their gradients and Paddle's Adam, in the dtype asked for
(float64: the yardstick; float32: what float32 arithmetic alone costs, the tolerance's unit).

Parameters are a dict under the reference's names: query_linear_i.weight [in, out], query_linear_i.bias, pos_linear_i.weight,
pos_linear_i.bias.  relu: one bool per layer.  A tower input is dense [rows, trigram_d] (csr_dense makes it from CSR); the
documents are stacked field-major: the B positives' rows, then each negative's."""
import numpy as np

EPS_COS, B1, B2, EPS_ADAM = 1e-8, 0.9, 0.999, 1e-8


def relerr(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(float(np.abs(want).max()), 1e-30))


def csr_dense(cols, vals, lod, width, dt=np.float64):
    """[rows, width] of a CSR input; an entry outside [0, width) is skipped, as the kernels skip it."""
    cols, vals, lod = np.asarray(cols), np.asarray(vals), np.asarray(lod)
    out = np.zeros((len(lod) - 1, width), dt)
    for r in range(len(lod) - 1):
        for j in range(lod[r], lod[r + 1]):
            if 0 <= cols[j] < width:
                out[r, cols[j]] += dt(vals[j])
    return out


def n_layers(p):
    n = 0
    while "query_linear_%d.weight" % n in p:
        n += 1
    return n


def tower(p, name, x, relu, dt=np.float64):
    """-> [x, the output of layer 0, ...]: acts[i + 1] = act_i(acts[i] W_i + b_i)."""
    acts = [np.asarray(x, dt)]
    for i in range(n_layers(p)):
        y = acts[-1] @ np.asarray(p["%s_linear_%d.weight" % (name, i)], dt) + np.asarray(p["%s_linear_%d.bias" % (name, i)], dt)
        acts.append(np.maximum(y, dt(0)) if relu[i] else y)
    return acts


def tower_bwd(p, name, acts, relu, d, g, dt=np.float64):
    """d: the gradient of the tower's output (after its last activation).  Fills g."""
    for i in range(n_layers(p) - 1, -1, -1):
        if relu[i]:
            d = d * (acts[i + 1] > 0)
        g["%s_linear_%d.weight" % (name, i)] = acts[i].T @ d
        g["%s_linear_%d.bias" % (name, i)] = d.sum(0, dtype=dt)
        if i:
            d = d @ np.asarray(p["%s_linear_%d.weight" % (name, i)], dt).T


def cosine(x, y, dt=np.float64):
    """Paddle's cosine_similarity(axis=1, eps=1e-8): w12 / sqrt(max(w1 w2, eps^2)) -> (cos [R], and what its gradient needs)."""
    w12, w1, w2 = (x * y).sum(1, dtype=dt), (x * x).sum(1, dtype=dt), (y * y).sum(1, dtype=dt)
    prod, lim = w1 * w2, dt(EPS_COS) * dt(EPS_COS)
    is_open = prod >= lim
    inv = dt(1) / np.sqrt(np.where(is_open, prod, lim))
    return (w12 * inv).astype(dt), (w1, w2, inv.astype(dt), is_open)


def cosine_bwd(x, y, cs, aux, gcos, dt=np.float64):
    """(d/dx, d/dy) of sum(gcos * cos): y / root - cos x / w1 where the product is not clamped, y / eps where it is."""
    w1, w2, inv, is_open = aux
    safe = lambda w: np.where(is_open, w, dt(1))
    sx, sy = np.where(is_open, cs / safe(w1), dt(0)), np.where(is_open, cs / safe(w2), dt(0))
    gc = gcos[:, None]
    return gc * (y * inv[:, None] - sx[:, None] * x), gc * (x * inv[:, None] - sy[:, None] * y)


def head(q, d, slice_end, dt=np.float64):
    """q [B, N], d [(1 + neg) B, N] -> dict(cos [B, 1 + neg], hit_prob [B], terms [B], loss, dq, dd): net.py:83-101 and
    dygraph_model.py:56-59 with their gradient; rows at or beyond slice_end give nothing to the loss."""
    q, d = np.asarray(q, dt), np.asarray(d, dt)
    B = q.shape[0]
    docs = d.shape[0] // B
    cs, aux = zip(*[cosine(q, d[k * B:(k + 1) * B], dt) for k in range(docs)])
    cos = np.stack(cs, 1)
    e = np.exp(cos - cos.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True, dtype=dt)).astype(dt)
    M = min(B, int(slice_end))
    terms = -np.log(prob[:, 0])
    gcos = prob.copy()
    gcos[:, 0] -= dt(1)
    gcos = gcos / dt(M)
    gcos[M:] = 0
    dq, dd = np.zeros_like(q), np.zeros_like(d)
    for k in range(docs):
        a, b = cosine_bwd(q, d[k * B:(k + 1) * B], cs[k], aux[k], gcos[:, k], dt)
        dq += a
        dd[k * B:(k + 1) * B] = b
    return dict(cos=cos, hit_prob=prob[:, 0], terms=terms, loss=dt(terms[:M].sum(dtype=dt) / dt(M)), dq=dq, dd=dd)


def forward_infer(p, relu, q_in, d_in, dt=np.float64):
    """-> the positive cosine [B]."""
    qa, da = tower(p, "query", q_in, relu, dt), tower(p, "pos", d_in, relu, dt)
    return cosine(qa[-1], da[-1], dt)[0]


def loss_and_grads(p, relu, q_in, d_in, slice_end, dt=np.float64):
    """-> dict(loss [1], cos, hit_prob [min(B, slice_end)], g {name: gradient})."""
    qa, da = tower(p, "query", q_in, relu, dt), tower(p, "pos", d_in, relu, dt)
    h = head(qa[-1], da[-1], slice_end, dt)
    g = {}
    tower_bwd(p, "query", qa, relu, h["dq"], g, dt)
    tower_bwd(p, "pos", da, relu, h["dd"], g, dt)
    M = min(qa[-1].shape[0], int(slice_end))
    return dict(loss=np.asarray([h["loss"]]), cos=h["cos"], hit_prob=h["hit_prob"][:M], g=g)


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


def train_step(p, m, v, relu, q_in, d_in, slice_end, step, lr, dt=np.float64):
    """-> dict(loss, cos, hit_prob, g, n, m, v)."""
    out = loss_and_grads(p, relu, q_in, d_in, slice_end, dt)
    if m is None:
        m = {k: np.zeros_like(np.asarray(x, dt)) for k, x in p.items()}
        v = {k: np.zeros_like(np.asarray(x, dt)) for k, x in p.items()}
    out["n"], out["m"], out["v"] = adam(p, out["g"], m, v, step, lr, dt)
    return out


def load_golden(path):
    """-> (arrays, starting parameters {name: array}, lr, steps)."""
    g = dict(np.load(path))
    p = {k[2:]: v for k, v in g.items() if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0])
