"""Plain numpy restatements of the glue and loss entry points of paddlerec_amd/ops.py that only layer tests used to reach —
TEST INFRASTRUCTURE ONLY.  Written from the comments of the kernels (csrc/head_ops.hip, dmr_ops.hip, dien_ops.hip, emb_ops.hip,
sparse_update.hip) and the docstrings of ops.py; imports nothing from paddlerec_amd.

Every function takes `dtype` (float64: the reference; float32: the restatement whose own error sets the tolerance, see
tests/test_glue_kernels_gpu.py).  Inputs are the float32 arrays the kernel is given; a scalar the C entry point takes as
`float` (lr, scale, lo, hi) is rounded to float32 first, because that rounded value IS the kernel's input."""
import numpy as np

REC_FLAG_INDEX_OOB = 1


def relerr(a, b):
    """max|a - b| / max|b| (b: the reference; an all-zero reference compares absolutely)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def _a(x, dtype):
    return np.asarray(x, dtype=dtype)


def _s(x, dtype):
    """A `float` argument of the C entry point in dtype."""
    return dtype(np.float32(x))


# ---------------------------------------------------------------------------------------------------- loss
def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-z))


def bce_cost(z, t, dtype=np.float64):
    """binary_cross_entropy_with_logits per sample: max(z, 0) - z t + log1p(exp(-|z|))."""
    z, t = _a(z, dtype).reshape(-1), _a(t, dtype).reshape(-1)
    return np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))


def bce(z, t, mean_over=0, dtype=np.float64):
    """-> pred [B,1] = sigmoid(z), dz [B,1] = (pred - t) / n, loss [1] = sum(cost) / n, n = mean_over or B."""
    z, t = _a(z, dtype).reshape(-1), _a(t, dtype).reshape(-1)
    inv = dtype(1) / dtype(mean_over if mean_over > 0 else z.size)
    pred = sigmoid(z)
    return pred.reshape(-1, 1), ((pred - t) * inv).reshape(-1, 1), np.asarray([bce_cost(z, t, dtype).sum(dtype=dtype) * inv])


# ---------------------------------------------------------------------------------------------------- DMR tail glue
def dmr_tail_fwd(hist, item_eb, uv, match_mask, V, cate_id, dtype=np.float64):
    """hist [B,T,2E], item_eb [B,2E], uv [B,2,E], match_mask [B,1] int, V [C,E], cate_id [B] ->
    hist_sum [B,2E] = sum_t hist (UNMASKED), prod = item_eb * hist_sum, rel [B,1] = uv[:,1] . V[cate_id],
    U2 [B,E] = uv[:,0] * float(match_mask), flag (REC_FLAG_INDEX_OOB when a cate_id is outside [0, C): V reads as 0 there)."""
    hist, item_eb, uv, V = (_a(x, dtype) for x in (hist, item_eb, uv, V))
    cate_id = np.asarray(cate_id, np.int64)
    ok = (cate_id >= 0) & (cate_id < V.shape[0])
    rows = np.where(ok[:, None], V[np.where(ok, cate_id, 0)], dtype(0))
    hist_sum = hist.sum(1, dtype=dtype)
    rel = (uv[:, 1] * rows).sum(-1, keepdims=True, dtype=dtype)
    U2 = uv[:, 0] * np.asarray(match_mask).reshape(-1, 1).astype(dtype)
    return hist_sum, item_eb * hist_sum, rel, U2, (0 if ok.all() else REC_FLAG_INDEX_OOB)


def dmr_tail_bwd_match(dU2, d_rel, uv, match_mask, V, cate_id, dtype=np.float64):
    """-> d_uv [B,2,E]: row 0 = dU2 * float(match_mask) (dU2 None: 0), row 1 = d_rel V[cate_id] (0 where cate_id is out of
    range); dV_rows [B,E] = d_rel uv[:,1] (written for EVERY sample, out-of-range ones included)."""
    d_rel, uv, V = _a(d_rel, dtype).reshape(-1, 1), _a(uv, dtype), _a(V, dtype)
    cate_id = np.asarray(cate_id, np.int64)
    ok = (cate_id >= 0) & (cate_id < V.shape[0])
    rows = np.where(ok[:, None], V[np.where(ok, cate_id, 0)], dtype(0))
    d_uv = np.zeros(uv.shape, dtype)
    if dU2 is not None:
        d_uv[:, 0] = _a(dU2, dtype) * np.asarray(match_mask).reshape(-1, 1).astype(dtype)
    d_uv[:, 1] = d_rel * rows
    return d_uv, d_rel * uv[:, 1]


def dmr_tail_bwd_hist(f1, f2, d_sum, d_prod, item_eb, hist_sum, d_item_direct, d_ctx, d_hist, dtype=np.float64):
    """-> d_hist [B,T,D] + (f1 + f2 + d_sum + d_prod * item_eb, the last two broadcast over T; f1, f2 None: absent),
    d_item [B,D] = d_item_direct + d_prod * hist_sum + sum_t d_ctx[b,t,:D]  (d_ctx [B*T, >= D])."""
    d_hist = _a(d_hist, dtype)
    B, T, D = d_hist.shape
    d_sum, d_prod, item_eb, hist_sum, d_item_direct = (_a(x, dtype) for x in (d_sum, d_prod, item_eb, hist_sum, d_item_direct))
    a = np.broadcast_to((d_sum + d_prod * item_eb)[:, None, :], (B, T, D))
    for f in (f1, f2):
        if f is not None:
            a = a + _a(f, dtype).reshape(B, T, D)
    d_item = (d_item_direct + d_prod * hist_sum) + _a(d_ctx, dtype)[:, :D].reshape(B, T, D).sum(1, dtype=dtype)
    return d_hist + a, d_item


# ---------------------------------------------------------------------------------------------------- DIEN attention pieces
def att_feat_fwd(hist, q, dtype=np.float64):
    """hist, q [.., E] -> feat [n, 4E] = [h, q, h - q, h * q]."""
    h, q = _a(hist, dtype), _a(q, dtype)
    E = h.shape[-1]
    h, q = h.reshape(-1, E), q.reshape(-1, E)
    return np.concatenate([h, q, h - q, h * q], 1)


def att_feat_bwd(hist, q, dfeat, dtype=np.float64):
    """-> (dh = d0 + d2 + d3 * q, d_q = d1 - d2 + d3 * h), both of hist's shape; the kernel adds dh to d_hist or writes it."""
    h, q, df = _a(hist, dtype), _a(q, dtype), _a(dfeat, dtype)
    E = h.shape[-1]
    d0, d1, d2, d3 = (df[:, i * E:(i + 1) * E].reshape(h.shape) for i in range(4))
    return (d0 + d2) + d3 * q, (d1 - d2) + d3 * h


def softmax_weight_fwd(score, mask, hist, scale, dtype=np.float64):
    """score, mask [B,T], hist [B,T,E] -> w [B,T] = softmax_t((score + mask) * scale), x_att [B,T,E] = w * hist."""
    hist = _a(hist, dtype)
    B, T, _ = hist.shape
    x = (_a(score, dtype).reshape(B, T) + _a(mask, dtype).reshape(B, T)) * _s(scale, dtype)
    e = np.exp(x - x.max(1, keepdims=True))
    w = e / e.sum(1, keepdims=True, dtype=dtype)
    return w, w[:, :, None] * hist


def softmax_weight_bwd(w, hist, dx_att, scale, dtype=np.float64):
    """-> dscore [B,T] = scale * w * (g - sum_s w_s g_s) with g_t = dx_att[b,t] . hist[b,t]; dh [B,T,E] = w * dx_att (the
    kernel adds it to d_hist or writes it)."""
    w, hist, dx = _a(w, dtype), _a(hist, dtype), _a(dx_att, dtype)
    g = (dx * hist).sum(-1, dtype=dtype)
    return _s(scale, dtype) * (w * (g - (w * g).sum(1, keepdims=True, dtype=dtype))), w[:, :, None] * dx


# ---------------------------------------------------------------------------------------------------- record gather
def record_gather(rows, rec, D, init_value=None, state_col=-1, initial_range=0.0, seed=0, row_mul=1, row_add=0,
                  init_embedx=False):
    """Both embeddings of every row from its record line rec [N, stride] = W(D) | W1 | ... -> (W [n,D], W1 [n], flag), float32
    (a copy: there is no arithmetic to restate in another precision).  A row outside [0, N) reads as zeros and sets the flag.
    With initial_range > 0 and state_col >= 0 a row whose state float is 0 is unborn: W1 reads as creation value element 0 and
    W as elements 1 + d when init_embedx (zeros otherwise), keyed by row * row_mul + row_add;
    init_value(seed, key, element, range) is the library's host function."""
    rows, rec = np.asarray(rows, np.int64), np.asarray(rec, np.float32)
    W, W1, flag = np.zeros((len(rows), D), np.float32), np.zeros(len(rows), np.float32), 0
    for i, row in enumerate(rows):
        if not 0 <= row < rec.shape[0]:
            flag |= REC_FLAG_INDEX_OOB
            continue
        r = rec[row]
        if initial_range > 0 and state_col >= 0 and r[state_col] == 0:
            key = int(row) * row_mul + row_add
            W1[i] = init_value(seed, key, 0, initial_range)
            if init_embedx:
                W[i] = [init_value(seed, key, 1 + d, initial_range) for d in range(D)]
        else:
            W[i], W1[i] = r[:D], r[D]
    return W, W1, flag


# ---------------------------------------------------------------------------------------------------- dense glue
def sgd_dense(p, g, lr, dtype=np.float64):
    """p - lr * g."""
    return _a(p, dtype) - _s(lr, dtype) * _a(g, dtype)


def copy_f32(src):
    return np.array(src, np.float32, copy=True)


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def splitmix_uniform(n, lo, hi, seed, dtype=np.float64):
    """value i = lo + (hi - lo) * u_i, u_i = the top 24 bits of splitmix64(seed ^ splitmix64(i)) / 2^24 (uint64 arithmetic,
    wrapping)."""
    with np.errstate(over="ignore"):
        r = _splitmix64(np.uint64(seed) ^ _splitmix64(np.arange(n, dtype=np.uint64)))
    u = (r >> np.uint64(40)).astype(dtype) * dtype(1.0 / 16777216.0)
    return _s(lo, dtype) + (_s(hi, dtype) - _s(lo, dtype)) * u
