"""The word2vec kernels (csrc/w2v_ops.hip) and the layer on the GPU against tests/word2vec_ref.py.  Tolerance, the project's
rule (tests/mtl_checks.py): max|got - ref64| / max|ref64| <= max(8 x the float32 restatement's error on the same inputs,
1e-6); every kernel runs twice and the two results are compared bit for bit."""
import numpy as np
import pytest
import torch

import word2vec_checks as K
import word2vec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, D, neg, pad): one sample; the golden's shape; a ragged last block and 75 float4 a row, more than a wave; the same with
# NaN behind every row; the scalar form; the limits
SHAPES = [(1, 1, 1, 0), (7, 12, 3, 0), (67, 300, 5, 0), (67, 300, 5, 4), (6, 13, 2, 3), (3, 1024, 32, 0)]
V = 41


def _table(rng, rows, D, pad, scale=0.5):
    """[rows, D] float32 values and their device view with row stride D + pad, NaN behind every row."""
    a = (scale * rng.standard_normal((rows, D))).astype(np.float32)
    full = torch.full((rows, D + pad), float("nan"), dtype=torch.float32, device=DEV)
    full[:, :D] = torch.from_numpy(a).to(DEV)
    return a, full[:, :D], full


def _pads_untouched(full, D):
    return bool(torch.isnan(full[:, D:]).all())


def _case(B, D, neg, pad, shared_neg=False, one_true=False, seed=0):
    rng = np.random.default_rng(100 * B + D + neg + pad + seed)
    emb, emb_v, emb_full = _table(rng, V, D, pad)
    w, w_v, w_full = _table(rng, V, D, pad)
    b, b_v, b_full = _table(rng, V, 1, pad)
    in_ids = rng.integers(0, V, B).astype(np.int64)
    tgt = rng.integers(0, V, (B, 1 + neg)).astype(np.int64)
    if shared_neg:
        tgt[:, 1:] = tgt[0, 1:]
    if one_true:
        tgt[:, 0] = 5
    if B > 2:
        in_ids[1], tgt[2, 0] = 0, 0                              # id 0 is an ordinary word
    return dict(emb=emb, w=w, b=b, emb_v=emb_v, w_v=w_v, b_v=b_v, full=(emb_full, w_full, b_full), in_ids=in_ids, tgt=tgt,
                D=D, pad=pad, B=B, neg=neg)


def _fwd(c, d_in=None):
    from paddlerec_amd import ops
    return ops.w2v_sgns_fwd_bwd(torch.from_numpy(c["in_ids"]).to(DEV), torch.from_numpy(c["tgt"]).to(DEV), c["emb_v"], c["w_v"],
                                c["b_v"], 1.0, None, d_in)


def _check_fwd(c, out, what):
    r64, r32 = (R.sgns(c["emb"], c["w"], c["b"], c["in_ids"], c["tgt"], 1.0, dt) for dt in (np.float64, np.float32))
    for k, got in zip(("true_logits", "neg_logits", "g", "d_in", "loss"), out):
        K.check_close(got.cpu().numpy(), r32[k], r64[k], "%s %s" % (what, k))


@pytest.mark.parametrize("B,D,neg,pad", SHAPES)
def test_sgns_fwd_bwd(B, D, neg, pad):
    c = _case(B, D, neg, pad)
    din_full = torch.full((B, D + pad), float("nan"), dtype=torch.float32, device=DEV)
    out = _fwd(c, din_full[:, :D])
    again = _fwd(c)
    assert int(out[5].item()) == 0
    for x, y in zip(out[:5], again[:5]):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))            # bit for bit
    _check_fwd(c, out, "fwd_bwd %s" % ((B, D, neg, pad),))
    assert _pads_untouched(din_full, D) and all(_pads_untouched(f, d) for f, d in zip(c["full"], (D, D, 1)))
    for f, ref in zip(c["full"], (c["emb"], c["w"], c["b"])):                                            # inputs are only read
        assert np.array_equal(f[:, :ref.shape[1]].cpu().numpy(), ref)


def test_sgns_out_of_range_ids_are_flagged_and_contribute_nothing():
    c = _case(7, 12, 3, 0)
    c["in_ids"][3], c["tgt"][2, 1], c["tgt"][5, 0] = V, -1, 1 << 40
    out = _fwd(c)
    assert int(out[5].item()) & 1
    g = out[2].cpu().numpy()
    assert (g[3] == 0).all() and g[2, 1] == 0 and g[5, 0] == 0 and g[2, 0] != 0 and not out[3][3].any()
    _check_fwd(c, out, "fwd_bwd with ids outside the table")


def _update(c, g):
    """-> (emb_w after, emb_b after, d_w_rows, d_b_rows, uniq rows) of one rec_w2v_target_update over fresh copies."""
    from paddlerec_amd import ops
    B, D, pad, n = c["B"], c["D"], c["pad"], c["tgt"].size
    w_full, b_full = c["full"][1].clone(), c["full"][2].clone()
    tgt = torch.from_numpy(c["tgt"]).to(DEV)
    groups = ops.IdGroups(n, DEV)
    ops.ids_group(tgt.reshape(-1), V, None, ops.Workspace(DEV), None, None, groups)
    dw_full = torch.full((n, D + pad), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    ops.w2v_target_update(groups, g, torch.from_numpy(c["in_ids"]).to(DEV), c["emb_v"], w_full[:, :D], b_full[:, :1], 0.25,
                          dw_full[:, :D], db)
    _, uniq, offs = groups.host()
    return w_full, b_full, dw_full, db, uniq, offs


def _check_update(c, what, expect_long=None):
    g = _fwd(c)[2]
    emb_before = c["full"][0].clone()
    first, second = _update(c, g), _update(c, g)
    for x, y in zip(first[:4], second[:4]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))                                      # bit for bit
    w_full, b_full, dw_full, db, uniq, offs = first
    D, U = c["D"], len(uniq)
    if expect_long is not None:
        assert (np.diff(offs).max() > 16) == expect_long          # which of the two kernels the longest segment took
    assert torch.equal(c["full"][0].view(torch.int32), emb_before.view(torch.int32))                      # emb bit-unchanged
    gn = g.cpu().numpy()
    (rows, dw64, db64), (_, dw32, db32) = (R.target_rows(c["emb"], c["in_ids"], c["tgt"], gn, dt) for dt in (np.float64, np.float32))
    assert np.array_equal(uniq, rows)
    K.check_close(dw_full[:U, :D].cpu().numpy(), dw32, dw64, what + " d_w_rows")
    K.check_close(db[:U].cpu().numpy(), db32, db64, what + " d_b_rows")
    lr = 0.25
    for before, after, d64, d32, name in ((c["w"], w_full[:, :D], dw64, dw32, "emb_w"), (c["b"], b_full[:, :1], db64[:, None], db32[:, None], "emb_b")):
        n64, n32 = before.astype(np.float64), before.copy()
        n64[rows] -= lr * d64
        n32[rows] = n32[rows] - np.float32(lr) * d32.astype(np.float32)
        K.check_delta(before, after.cpu().numpy(), n32, n64, "%s %s" % (what, name))
    assert _pads_untouched(w_full, D) and _pads_untouched(b_full, 1) and _pads_untouched(dw_full, D)
    assert bool(torch.isnan(dw_full[U:]).all()) and bool(torch.isnan(db[U:]).all())                       # nothing behind row U


@pytest.mark.parametrize("B,D,neg,pad", SHAPES)
def test_target_update(B, D, neg, pad):
    _check_update(_case(B, D, neg, pad), "target_update %s" % ((B, D, neg, pad),))


def test_target_update_long_segments_of_shared_negatives():
    """All 600 samples share the negatives: five segments of 600 occurrences, the block-per-slice path."""
    _check_update(_case(600, 12, 5, 0, shared_neg=True), "target_update shared negatives", expect_long=True)


def test_target_update_all_true_ids_one_row():
    _check_update(_case(67, 300, 5, 0, one_true=True), "target_update one true row", expect_long=True)
    _check_update(_case(9, 13, 2, 3, one_true=True), "target_update one true row, short", expect_long=False)


def test_target_update_drops_an_out_of_range_id():
    c = _case(67, 12, 3, 0)
    c["in_ids"][3], c["tgt"][2, 1], c["tgt"][5, 0] = V, -1, V + 7
    _check_update(c, "target_update with ids outside the table")


def test_layer_two_steps_gpu():
    G = K.gold()
    m = K.layer_of(G, DEV)
    K.check_layer(G, m, "gpu layer")
    from paddlerec_amd.word2vec import Word2VecInferLayer
    g = G["g"]
    inf = Word2VecInferLayer(50, 12, device=DEV, table=torch.as_tensor(g["n_1_embedding.weight"]).to(DEV))
    values, ids = inf.forward(*(torch.as_tensor(g[n]).to(DEV) for n in ("a_ids", "b_ids", "c_ids")))
    assert np.array_equal(ids.cpu().numpy(), g["topk_ids"])
    s = R.scores(g["n_1_embedding.weight"], g["a_ids"], g["b_ids"], g["c_ids"])
    K.check_close(values.cpu().numpy(), g["topk_values"], R.topk(s, 4)[0], "gpu layer recorded analogy values")


def _tile():
    from paddlerec_amd import _lib
    return _lib.REC_W2V_TOPK_TILE_ROWS


def _topk(W, a, b, c, k, pad=0):
    from paddlerec_amd import ops
    full = torch.full((W.shape[0], W.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    full[:, :W.shape[1]] = torch.from_numpy(W).to(DEV)
    st = ops.new_status(DEV)
    args = [torch.from_numpy(x).to(DEV) for x in (a, b, c)]
    v1, i1 = ops.w2v_analogy_topk(*args, full[:, :W.shape[1]], k, st)
    v2, i2 = ops.w2v_analogy_topk(*args, full[:, :W.shape[1]], k, st)
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(i1, i2) and int(st.item()) == 0
    return v1.cpu().numpy(), i1.cpu().numpy()


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("D", [300, 13, 1])
@pytest.mark.parametrize("Q", [1, 5, 67])
@pytest.mark.parametrize("Vn", [85, "T+3", "3T+1", "T"])
def test_analogy_topk(Vn, Q, D, k):
    """D 300 and 13: the k + 2 best float64 scores of every query are more than 1e-4 of the largest apart (asserted), so the
    ids must equal the reference's.  D 1: a one-column row normalises to exactly +-1, so the scores are exactly +-target and
    no draw can separate them; there the ids must equal the reference's under the tie rule, lower id first, across tiles."""
    T = _tile()
    Vn = {85: 85, "T+3": T + 3, "3T+1": 3 * T + 1, "T": T}[Vn]
    W, a, b, c, s64 = K.analogy_case(Vn, Q, D, k)
    if D > 1:
        assert R.separated(s64, k + 2)
    else:
        assert len(np.unique(np.abs(s64))) <= Q + 1                       # exactly +-target (or 0): ties everywhere
    want_v, want_i = R.topk(s64, k)
    got_v, got_i = _topk(W, a, b, c, k, pad=(3 if D == 13 else 0))
    assert np.array_equal(got_i, want_i)
    K.check_close(got_v, R.topk(R.scores(W, a, b, c, np.float32), k)[0], want_v, "analogy_topk %s" % ((Vn, Q, D, k),))
    assert (np.diff(got_v, axis=1) <= 0).all()                            # descending


def test_analogy_topk_ties_order_by_lower_id_and_a_zero_row_scores_zero():
    T = _tile()
    W, a, b, c, s64 = K.analogy_case(T + 3, 5, 13, 4)
    W = W.copy()
    best = int(R.topk(s64, 1)[1][0, 0])
    lo, hi = (3 if best != 3 else 4), T + 1                               # two copies of query 0's best row, in different tiles
    assert best not in (lo, hi, 7) and not {lo, hi, 7} & {int(a[0]), int(b[0]), int(c[0])}
    W[lo] = W[hi] = 2.0 * W[best]                                         # the same direction: one score, exactly, three times
    W[7] = 0.0                                                            # an all-zero row: 0 / 1e-12 = 0
    s = R.scores(W, a, b, c)
    want_v, want_i = R.topk(s, 4)
    assert s[0, lo] == s[0, hi] == s[0, best] and list(want_i[0, :3]) == sorted([best, lo, hi]) and (s[:, 7] == 0).all()
    got_v, got_i = _topk(W, a, b, c, 4)
    assert list(got_i[0, :3]) == sorted([best, lo, hi]) and got_v[0, 0] == got_v[0, 1] == got_v[0, 2]      # lower id first
    K.check_close(got_v[0, :3], R.topk(R.scores(W, a, b, c, np.float32), 3)[0][0], want_v[0, :3], "analogy_topk tie values")
    # the zero row's score: target = W[7] - W[1] + W[7] = -W[1] has positive columns, every other row negative ones
    Wz = -np.abs(W) - 0.01
    Wz[7] = 0.0
    one, zero = np.asarray([1], np.int64), np.asarray([7], np.int64)
    v, i = _topk(Wz, one, zero, zero, 1)
    assert i[0, 0] == 7 and v[0, 0] == 0.0
