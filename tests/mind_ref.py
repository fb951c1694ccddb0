"""NumPy restatement of MIND (models/recall/mind: net.py, dygraph_model.py) and of the kernels of csrc/mind_ops.hip — TEST
INFRASTRUCTURE ONLY.  float64 by default; dtype=np.float32 evaluates the same formulas in float32 (the error of that
evaluation against float64 is what the tests' tolerance is made of).  The matrix product and relerr are tests/mtl_ref.py's,
the left-to-right float32 dot tests/aitm_ref.py's.

A net is known from its state_dict (the reference's names): item_emb.weight [N, E], embedding_bias [N],
capsual_layer.routing_logits [1, K, T], capsual_layer.bilinear_mapping_matrix [E, H], capsual_layer.relu_layer.weight
[H, H] and .bias [H].  embedding_bias and routing_logits are trainable=False (net.py:142, :270): no gradient, never stepped.
log_q (net.py:40-47) and the step's negatives (net.py:55-58) are DATA here."""
import numpy as np

from aitm_ref import dot
from mtl_ref import mm, relerr  # noqa: F401

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
PAD = -2.0 ** 32 + 1                                   # net.py:189
HIT = -1e30                                            # net.py:96
FROZEN = ("embedding_bias", "capsual_layer.routing_logits")


# ------------------------------------------------------------------------------------------------ the kernels
def squash(Z, dtype=np.float64):
    """net.py:155-162 -> (squashed, n2)."""
    n2 = dot(Z, Z)[..., None]
    return n2 / (1 + n2) / np.sqrt(n2 + dtype(1e-8)) * Z, n2


def softmax(x, axis):
    e = np.exp(x - x.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def bmm(a, b):
    """[B, m, k] x [B, k, n] with mtl_ref.mm's summation per sample."""
    return np.stack([mm(x, y) for x, y in zip(a, b)]) if len(a) else np.zeros((0, a.shape[1], b.shape[2]), a.dtype)


def routing_fwd(low, seq_len, logits, iters, dtype=np.float64):
    """net.py:178-229.  low [B, T, H], seq_len [B], logits [K, T] -> (W [B, K, T], Z [B, K, H], caps [B, K, H])."""
    low, lg = np.asarray(low, dtype), np.asarray(logits, dtype)
    B, T, H = low.shape
    K = lg.shape[0]
    mask = (np.arange(T)[None, None, :] < np.asarray(seq_len).reshape(B, 1, 1))           # :164-176
    mask = np.broadcast_to(mask, (B, K, T))
    pad = dtype(PAD)
    Bl = np.broadcast_to(lg[None], (B, K, T)).astype(dtype)
    for _ in range(iters - 1):                                                            # :210-223
        W = softmax(np.where(mask, Bl, pad), 2)
        caps, _ = squash(bmm(W, low), dtype)
        Bl = Bl + np.swapaxes(bmm(low, np.swapaxes(caps, 1, 2)), 1, 2)
    W = softmax(np.where(mask, Bl, pad), 1)                                               # :225-226: axis = 1, the capsules
    Z = bmm(W, low)
    return W, Z, squash(Z, dtype)[0]


def routing_bwd(d_caps, Z, W, dtype=np.float64):
    """W is constant (B and the inner rounds are behind stop_gradient): -> d_low [B, T, H]."""
    g, Z, W = np.asarray(d_caps, dtype), np.asarray(Z, dtype), np.asarray(W, dtype)
    n2 = dot(Z, Z)[..., None]
    q, p1 = np.sqrt(n2 + dtype(1e-8)), 1 + n2
    f = n2 / p1 / q
    df = 1 / (p1 * p1) / q - dtype(0.5) * (n2 / p1) / ((n2 + dtype(1e-8)) * q)
    dZ = f * g + 2 * df * dot(Z, g)[..., None] * Z
    return bmm(np.swapaxes(W, 1, 2), dZ)


def label_attn_fwd(caps2, target, pow_p, dtype=np.float64):
    """net.py:284-297.  caps2 [B, K, H], target [B, H] -> (user [B, H], attn [B, K])."""
    x, q = np.asarray(caps2, dtype), np.asarray(target, dtype)
    s = dot(x, np.broadcast_to(q[:, None, :], x.shape))
    if pow_p != 1.0:
        with np.errstate(invalid="ignore"):
            s = np.power(s, dtype(pow_p))
    a = softmax(s, 1)
    user = np.zeros_like(q)
    for k in range(x.shape[1]):
        user = user + a[:, k:k + 1] * x[:, k]
    return user, a


def label_attn_bwd(caps2, target, attn, d_user, pow_p, dtype=np.float64):
    """-> (d_caps2 [B, K, H], d_target [B, H])."""
    x, q, a, g = (np.asarray(v, dtype) for v in (caps2, target, attn, d_user))
    da = dot(x, np.broadcast_to(g[:, None, :], x.shape))
    ds = a * (da - dot(a, da)[:, None])
    if pow_p != 1.0:
        s = dot(x, np.broadcast_to(q[:, None, :], x.shape))
        with np.errstate(invalid="ignore", divide="ignore"):
            ds = ds * dtype(pow_p) * np.power(s, dtype(pow_p - 1.0))
    d_x = a[:, :, None] * g[:, None, :] + ds[:, :, None] * q[:, None, :]
    d_q = np.zeros_like(q)
    for k in range(x.shape[1]):
        d_q = d_q + ds[:, k:k + 1] * x[:, k]
    return d_x, d_q


def ssm_head(user, true_w, true_b, S, sample_b, labels, neg, logq_true, logq_neg, grad_scale=1.0, dtype=np.float64):
    """net.py:86-112 after the gathers and the [B, n] product S.  -> (loss [B], dS [B, n], d_true [B])."""
    f = lambda v: np.asarray(v, dtype)
    labels, neg = np.asarray(labels).reshape(-1), np.asarray(neg).reshape(-1)
    x0 = dot(f(user), f(true_w)) + f(true_b) - f(logq_true)
    hit = labels[:, None] == neg[None, :]
    xs = np.where(hit, dtype(HIT), f(S) + f(sample_b)[None, :]) - f(logq_neg)[None, :]
    x = np.concatenate([x0[:, None], xs], 1)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    tot = e.sum(1, keepdims=True)
    loss = (m + np.log(tot))[:, 0] - x0
    sm = e / tot
    return loss, dtype(grad_scale) * sm[:, 1:], dtype(grad_scale) * (sm[:, 0] - 1)


# ------------------------------------------------------------------------------------------------ the net
def embed(table, ids, dtype=np.float64):
    """nn.Embedding(padding_idx=0): id 0 gives a zero row whatever row 0 holds."""
    ids = np.asarray(ids)
    return np.where((ids != 0)[..., None], np.asarray(table, dtype)[ids], dtype(0))


def forward(p, hist, seq_len, labels, neg, log_q, pow_p=1.0, iters=3, dtype=np.float64):
    """net.py:299-318 in train mode.  hist [B, T], seq_len [B], labels [B], neg [n], log_q [N] -> the forward record."""
    w = lambda k: np.asarray(p[k], dtype)
    hist, labels, neg = np.asarray(hist), np.asarray(labels).reshape(-1), np.asarray(neg).reshape(-1)
    B, T = hist.shape
    tab, M = w("item_emb.weight"), w("capsual_layer.bilinear_mapping_matrix")
    E, H = M.shape
    emb = embed(tab, hist, dtype)                                                          # [B, T, E]
    low = mm(emb.reshape(B * T, E), M).reshape(B, T, H)
    W, Z, caps = routing_fwd(low, seq_len, w("capsual_layer.routing_logits")[0], iters, dtype)
    caps2 = np.maximum(mm(caps.reshape(-1, H), w("capsual_layer.relu_layer.weight")) + w("capsual_layer.relu_layer.bias"), 0)
    caps2 = caps2.reshape(B, -1, H)
    target = embed(tab, labels, dtype)
    user, attn = label_attn_fwd(caps2, target, pow_p, dtype)
    true_w, sample_w = tab[labels], tab[neg]                                               # paddle.gather: id 0 is a row
    bias = w("embedding_bias")
    lq = np.asarray(log_q, dtype)
    S = mm(user, sample_w.T)
    with np.errstate(invalid="ignore", over="ignore"):
        loss_b, dS, d_true = ssm_head(user, true_w, bias[labels], S, bias[neg], labels, neg, lq[labels], lq[neg], 1.0 / B, dtype)
    return dict(B=B, T=T, E=E, H=H, hist=hist, labels=labels, neg=neg, emb=emb, low=low, W=W, Z=Z, caps=caps, caps2=caps2,
                target=target, user=user, attn=attn, true_w=true_w, sample_w=sample_w, S=S, loss_b=loss_b, loss=loss_b.mean(),
                dS=dS, d_true=d_true)


def scatter_rows(g, ids, d, padding):
    """g[ids[i]] += d[i] in flattened order; with padding, id 0 receives nothing."""
    for i, r in enumerate(np.asarray(ids).reshape(-1)):
        if not (padding and r == 0):
            g[r] = g[r] + d[i]
    return g


def backward(p, c, pow_p=1.0, dtype=np.float64):
    """-> the gradients of the stepped parameters, item_emb.weight as the dense [N, E] array Paddle's Adam receives."""
    w = lambda k: np.asarray(p[k], dtype)
    B, T, E, H = c["B"], c["T"], c["E"], c["H"]
    tab, M, Wr = w("item_emb.weight"), w("capsual_layer.bilinear_mapping_matrix"), w("capsual_layer.relu_layer.weight")
    dS, d_true, user = c["dS"], c["d_true"], c["user"]
    d_user = d_true[:, None] * c["true_w"] + mm(dS, c["sample_w"])
    d_sample_w = mm(dS.T, user)
    d_true_w = d_true[:, None] * user
    d_caps2, d_target = label_attn_bwd(c["caps2"], c["target"], c["attn"], d_user, pow_p, dtype)
    d_pre = np.where(c["caps2"] > 0, d_caps2, dtype(0)).reshape(-1, H)
    g = {"capsual_layer.relu_layer.weight": mm(c["caps"].reshape(-1, H).T, d_pre), "capsual_layer.relu_layer.bias": d_pre.sum(0)}
    d_caps = mm(d_pre, Wr.T).reshape(B, -1, H)
    d_low = routing_bwd(d_caps, c["Z"], c["W"], dtype).reshape(B * T, H)
    g["capsual_layer.bilinear_mapping_matrix"] = mm(c["emb"].reshape(B * T, E).T, d_low)
    d_emb = mm(d_low, M.T)
    gt = np.zeros_like(tab)
    scatter_rows(gt, c["hist"], d_emb, True)              # the four uses of the table, in the layer's order
    scatter_rows(gt, c["labels"], d_target, True)
    scatter_rows(gt, c["labels"], d_true_w, False)
    scatter_rows(gt, c["neg"], d_sample_w, False)
    g["item_emb.weight"] = gt
    return g, dict(d_user=d_user, d_caps2=d_caps2, d_target=d_target, d_caps=d_caps, d_low=d_low, d_emb=d_emb)


def adam_step(p, g, lr, state=None, dtype=np.float64):
    """paddle.optimizer.Adam (non-lazy, beta 0.9 / 0.999, epsilon 1e-8, no L2) on the parameters that have a gradient; the
    FROZEN ones pass through.  state: {'t', 'm', 'v'} of the steps before (None: the first step; not written)."""
    st = dict(t=state["t"], m=dict(state["m"]), v=dict(state["v"])) if state is not None else dict(t=0, m={}, v={})
    st["t"] += 1
    t, new = st["t"], {}
    for k, wk in p.items():
        if k in FROZEN:
            new[k] = np.asarray(wk).copy()
            continue
        wk = np.asarray(wk, dtype)
        gk = np.asarray(g[k], dtype).reshape(wk.shape)
        m = st["m"][k] = dtype(BETA1) * np.asarray(st["m"].get(k, 0), dtype) + dtype(1 - BETA1) * gk
        v = st["v"][k] = dtype(BETA2) * np.asarray(st["v"].get(k, 0), dtype) + dtype(1 - BETA2) * gk * gk
        lr_t = dtype(lr) * np.sqrt(dtype(1 - BETA2 ** t)) / dtype(1 - BETA1 ** t)
        new[k] = wk - lr_t * m / (np.sqrt(v) + dtype(ADAM_EPS) * np.sqrt(dtype(1 - BETA2 ** t)))
    return new, st


def train_step(p, hist, seq_len, labels, neg, log_q, lr, state=None, pow_p=1.0, iters=3, dtype=np.float64):
    """-> (forward record, gradients, parameters after Adam, optimizer state)."""
    c = forward(p, hist, seq_len, labels, neg, log_q, pow_p, iters, dtype)
    g, mid = backward(p, c, pow_p, dtype)
    c.update(mid)
    new, state = adam_step(p, g, lr, state, dtype)
    return c, g, new, state


def log_q_table(item_count, n_sample):
    """net.py:40-47, the reference's own sequence: float64 prob, cast to float32, then log1p / exp / log with every
    intermediate a float32, each function the correctly rounded float32 (through float64: the shim's arithmetic in
    tools/make_golden_mind.py).  prob[0] = 0, so log_q[0] = -inf."""
    import torch
    prob = np.array([0.0] * item_count)
    for i in range(1, item_count):
        prob[i] = (np.log(i + 2) - np.log(i + 1)) / np.log(item_count + 1)
    new_prob = torch.from_numpy(prob.astype("float32"))
    f = lambda fn, x: fn(x.double()).float()
    return prob, f(torch.log, -(f(torch.exp, (-f(torch.log1p, new_prob) * 2 * n_sample)) - 1.0)).numpy()


def load_golden(path):
    """-> (the npz as a dict, the initial state_dict, lr, steps).  Step s: hist_s [B, T], seq_len_s [B], label_s [B], neg_s
    [n], loss_s [1], user_cap_s [B, K, H], W_s [B, K, T], g_s_<key>, n_s_<key>; log_q [N]; pow_p, iters."""
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    return g, p, float(g["lr"][0]), int(g["steps"][0])
