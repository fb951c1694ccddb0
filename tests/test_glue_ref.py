"""tests/glue_ref.py itself, on the host: each restatement against the CPU mirrors the layer tests already run on
(tests/dmr_cpu_kernels.py, tests/cpu_kernels.py) within float32 round-off, and every backward against central differences of
its own forward in float64.

The mirrors evaluate in float32, so they are held to the project's rule: err = max|mirror - ref64| / max|ref64| within
max(8 x the float32 restatement's error, 1e-6).  The central differences (step 1e-6, float64) are held to a relative error
of 1e-6: every forward here is at most quadratic in its inputs except the softmax and the loss, whose third derivatives are
of order one at the inputs drawn below, so the truncation error is ~1e-12 and the round-off ~1e-16 / 1e-6 = 1e-10 of the
function's scale.  Achieved on the inputs below: at most 3e-9 (printed by each test)."""
import numpy as np
import pytest
import torch

import glue_ref as G

F32, F64 = np.float32, np.float64


def _bound(ref32, ref64):
    return max(8 * G.relerr(ref32, ref64), 1e-6)


def _mirror(got, ref64, ref32, what):
    e, b = G.relerr(np.asarray(got).reshape(np.shape(ref64)), ref64), _bound(ref32, ref64)
    print("%-40s err %.3g  float32-ref err %.3g" % (what, e, G.relerr(ref32, ref64)))
    assert e <= b, (what, e, b)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _central(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        d = np.zeros_like(x)
        d[i] = h
        g[i] = (f(x + d) - f(x - d)) / (2 * h)
    return g


def _fd(analytic, f, x, what):
    e = G.relerr(analytic, _central(f, x))
    print("%-40s central-difference err %.3g" % (what, e))
    assert e < 1e-6, (what, e)


# ---------------------------------------------------------------------------------------------------- against the mirrors
def _tail_problem(rng, B, T, E, C):
    D = 2 * E
    p = dict(hist=rng.standard_normal((B, T, D)), item_eb=rng.standard_normal((B, D)), uv=rng.standard_normal((B, 2, E)),
             V=rng.standard_normal((C, E)), d_rel=rng.standard_normal((B, 1)), dU2=rng.standard_normal((B, E)),
             f1=rng.standard_normal((B, T, D)), f2=rng.standard_normal((B, T, D)), d_sum=rng.standard_normal((B, D)),
             d_prod=rng.standard_normal((B, D)), d_item_direct=rng.standard_normal((B, D)),
             d_ctx=rng.standard_normal((B * T, D + 3)), d_hist=rng.standard_normal((B, T, D)))
    p = {k: v.astype(F32) for k, v in p.items()}
    p["match_mask"] = rng.integers(0, 3, (B, 1)).astype(np.int64)
    p["cate_id"] = rng.integers(0, C, B).astype(np.int64)
    return p


def test_dmr_tail_against_the_cpu_mirror():
    import dmr_cpu_kernels as M
    rng = np.random.default_rng(1)
    B, T, E, C = 5, 7, 6, 11
    p = _tail_problem(rng, B, T, E, C)
    fw = [G.dmr_tail_fwd(p["hist"], p["item_eb"], p["uv"], p["match_mask"], p["V"], p["cate_id"], dt) for dt in (F64, F32)]
    hs, pr, rel = torch.zeros(B, 2 * E), torch.zeros(B, 2 * E), torch.zeros(B, 1)
    U2 = M.dmr_tail_fwd(_t(p["hist"]), _t(p["item_eb"]), _t(p["uv"]), _t(p["match_mask"]), _t(p["V"]), _t(p["cate_id"]), hs, pr,
                        rel, None)
    for name, got, a, b in zip(("hist_sum", "prod", "rel_u2i", "U2"), (hs, pr, rel, U2), fw[0], fw[1]):
        _mirror(got.numpy(), a, b, "tail fwd " + name)
    assert fw[0][4] == 0
    for dU2 in (p["dU2"], None):
        bm = [G.dmr_tail_bwd_match(dU2, p["d_rel"], p["uv"], p["match_mask"], p["V"], p["cate_id"], dt) for dt in (F64, F32)]
        dvr = torch.zeros(B, E)
        d_uv = M.dmr_tail_bwd_match(None if dU2 is None else _t(dU2), _t(p["d_rel"]), _t(p["uv"]), _t(p["match_mask"]),
                                    _t(p["V"]), _t(p["cate_id"]), dvr)
        _mirror(d_uv.numpy(), bm[0][0], bm[1][0], "tail bwd_match d_uv")
        _mirror(dvr.numpy(), bm[0][1], bm[1][1], "tail bwd_match dV_rows")
    hsum = fw[0][0].astype(F32)
    for f1, f2 in ((p["f1"], p["f2"]), (p["f1"], None), (None, p["f2"]), (None, None)):
        bh = [G.dmr_tail_bwd_hist(f1, f2, p["d_sum"], p["d_prod"], p["item_eb"], hsum, p["d_item_direct"], p["d_ctx"], p["d_hist"],
                                  dt) for dt in (F64, F32)]
        dh, di = _t(p["d_hist"].copy()), torch.zeros(B, 2 * E)
        M.dmr_tail_bwd_hist(None if f1 is None else _t(f1), None if f2 is None else _t(f2), _t(p["d_sum"]), _t(p["d_prod"]),
                            _t(p["item_eb"]), _t(hsum), _t(p["d_item_direct"]), _t(p["d_ctx"]), dh, di)
        _mirror(dh.numpy(), bh[0][0], bh[1][0], "tail bwd_hist d_hist")
        _mirror(di.numpy(), bh[0][1], bh[1][1], "tail bwd_hist d_item")


def test_dmr_tail_out_of_range_category_reads_zero_and_flags():
    rng = np.random.default_rng(2)
    p = _tail_problem(rng, 4, 2, 3, 5)
    p["cate_id"][:] = [-1, 2, 5, 0]
    *_, rel, U2, flag = G.dmr_tail_fwd(p["hist"], p["item_eb"], p["uv"], p["match_mask"], p["V"], p["cate_id"])
    assert flag == G.REC_FLAG_INDEX_OOB and rel[0, 0] == 0 and rel[2, 0] == 0 and rel[1, 0] != 0
    d_uv, dvr = G.dmr_tail_bwd_match(None, p["d_rel"], p["uv"], p["match_mask"], p["V"], p["cate_id"])
    assert not d_uv[:, 0].any() and not d_uv[0, 1].any() and not d_uv[2, 1].any() and d_uv[1, 1].all()
    assert np.array_equal(dvr, p["d_rel"].astype(F64) * p["uv"][:, 1].astype(F64))          # written for every sample


def test_att_feat_against_the_cpu_mirror():
    import dmr_cpu_kernels as M
    rng = np.random.default_rng(3)
    h, q = rng.standard_normal((3, 5, 4)).astype(F32), rng.standard_normal((3, 5, 4)).astype(F32)
    df, d0 = rng.standard_normal((15, 16)).astype(F32), rng.standard_normal((3, 5, 4)).astype(F32)
    a, b = (G.att_feat_fwd(h, q, dt) for dt in (F64, F32))
    _mirror(M.dien_att_feat_fwd(_t(h), _t(q)).numpy(), a, b, "att_feat fwd")
    a, b = (G.att_feat_bwd(h, q, df, dt) for dt in (F64, F32))
    for acc in (True, False):
        dh = _t(d0.copy())
        dq = M.dien_att_feat_bwd(_t(h), _t(q), _t(df), dh, accumulate=acc)
        _mirror(dh.numpy(), a[0] + (d0 if acc else 0), b[0] + (d0 if acc else 0), "att_feat bwd d_hist acc=%d" % acc)
        _mirror(dq.numpy(), a[1], b[1], "att_feat bwd d_q")


def test_softmax_weight_against_torch():
    """There is no CPU mirror of the softmax pieces alone; torch's float64 softmax stands in."""
    rng = np.random.default_rng(4)
    B, T, E = 3, 9, 4
    s, h = rng.standard_normal((B, T)).astype(F32) * 50, rng.standard_normal((B, T, E)).astype(F32)
    m = np.where(np.arange(T)[None] < np.array([T, 4, 1])[:, None], 0.0, -1e9).astype(F32)
    w, x = G.softmax_weight_fwd(s, m, h, 0.5)
    want = torch.softmax((_t(s).double() + _t(m).double()) * 0.5, 1).numpy()
    assert G.relerr(w, want) < 1e-14 and G.relerr(x, want[:, :, None] * h) < 1e-14
    assert w[2, 0] == 1.0 and not w[2, 1:].any() and np.allclose(w.sum(1), 1, atol=1e-14)


def test_bce_sgd_copy_against_the_cpu_mirror():
    import cpu_kernels as M
    rng = np.random.default_rng(5)
    z = (3 * rng.standard_normal((37, 1))).astype(F32)
    t = rng.integers(0, 2, (37, 1)).astype(F32)
    a, b = (G.bce(z, t, 0, dt) for dt in (F64, F32))
    for name, got, r64, r32 in zip(("pred", "dz", "loss"), M.bce_with_logits(_t(z), _t(t), None), a, b):
        _mirror(got.numpy(), r64, r32, "bce " + name)
    a3 = G.bce(z, t, 3 * 37)
    assert G.relerr(a3[1] * 3, a[1]) < 1e-15 and G.relerr(a3[2] * 3, a[2]) < 1e-15 and np.array_equal(a3[0], a[0])
    big = np.array([30, -30, 100, -100, 1e4, -1e4], F32)                       # saturation: cost = |z| on the wrong side
    for dt in (F64, F32):
        assert np.isfinite(G.bce(big, (big < 0).astype(F32), 0, dt)[2]).all()
        assert G.relerr(G.bce_cost(big, (big < 0).astype(F32), dt), np.abs(big)) < 1e-6
        assert G.bce_cost(big[2:], (big[2:] > 0).astype(F32), dt).max() < 1e-40
    p, g = rng.standard_normal(301).astype(F32), rng.standard_normal(301).astype(F32)
    for lr in (0.85, -1.0, 0.0):
        pt = _t(p.copy())
        M.sgd_dense(pt, _t(g), lr)
        _mirror(pt.numpy(), G.sgd_dense(p, g, lr), G.sgd_dense(p, g, lr, F32), "sgd_dense lr=%g" % lr)
    assert np.array_equal(G.sgd_dense(p, g, 0.0, F32).view(np.uint32), p.view(np.uint32))
    src = rng.standard_normal(40).astype(F32)
    src.view(np.uint32)[:2] = [0x7FC00001, 0xFFC12345]                         # NaN payloads travel
    dst = torch.zeros(40)
    M.copy_f32(dst, _t(src))
    assert np.array_equal(dst.numpy().view(np.uint32), G.copy_f32(src).view(np.uint32))


def test_record_gather_against_the_cpu_mirror(engine_lib):
    import cpu_kernels as M
    rng = np.random.default_rng(6)
    init = lambda seed, row, d, r: F32(engine_lib.rec_ps_init_value_host(seed, row, d, r))
    N, D = 23, 8
    tab = M.PsTable(N, D, torch.device("cpu"), kind="deepfm", initial_range=0.25, embed_zero_init=False, seed=77, row_mul=4,
                    row_add=3)
    rec = tab.rec.numpy()
    rec[:] = rng.standard_normal(rec.shape).astype(F32)
    rec[::3] = 0                                                               # unborn: zero memory, state float included
    before = rec.copy()
    rows = rng.integers(0, N, 50)
    for table in (None, tab):
        ow, ow1 = torch.zeros(50, D), torch.zeros(50)
        M.record_gather(_t(rows), tab.rec, D, ow, ow1, None, table=table)
        kw = {} if table is None else dict(init_value=init, state_col=tab.state_col, initial_range=0.25, seed=77, row_mul=4,
                                           row_add=3)
        W, W1, flag = G.record_gather(rows, rec, D, **kw)
        assert flag == 0 and np.array_equal(ow.numpy(), W) and np.array_equal(ow1.numpy(), W1)
    unborn = rows % 3 == 0
    assert unborn.any() and W1[unborn].all() and (np.abs(W1[unborn]) <= 0.25).all() and not W[unborn].any()
    Wx, W1x, _ = G.record_gather(rows, rec, D, init_value=init, state_col=tab.state_col, initial_range=0.25, seed=77, row_mul=4,
                                 row_add=3, init_embedx=True)
    i = int(np.flatnonzero(unborn)[0])
    assert np.array_equal(W1x, W1) and Wx[i, 2] == init(77, int(rows[i]) * 4 + 3, 3, 0.25) and np.array_equal(Wx[~unborn], W[~unborn])
    W, W1, flag = G.record_gather(np.array([-1, 1, N]), rec, D)
    assert flag == G.REC_FLAG_INDEX_OOB and not W[[0, 2]].any() and not W1[[0, 2]].any() and np.array_equal(W[1], rec[1, :D])
    assert np.array_equal(rec, before)


def test_splitmix_uniform_is_the_published_generator():
    """splitmix64's published first outputs from state 0 (Vigna's splitmix64.c: each call adds the golden-ratio increment, then
    mixes): _splitmix64(k * increment) is output k + 1."""
    inc = 0x9E3779B97F4A7C15
    with np.errstate(over="ignore"):
        got = G._splitmix64(np.array([0, inc, (2 * inc) % 2 ** 64], np.uint64))
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    v = G.splitmix_uniform(1000, -0.1, 0.3, 9)
    assert v.min() >= F32(-0.1) and v.max() < F32(0.3) and 0.05 < v.mean() < 0.15
    assert np.array_equal(G.splitmix_uniform(10, -0.1, 0.3, 9), v[:10]) and not np.array_equal(G.splitmix_uniform(10, -0.1, 0.3, 8), v[:10])
    assert G.relerr(G.splitmix_uniform(1000, -0.1, 0.3, 9, F32), v) < 1e-6


# ---------------------------------------------------------------------------------------------------- central differences
def test_bce_gradient_against_central_differences():
    rng = np.random.default_rng(7)
    z, t = 2 * rng.standard_normal(9), rng.random(9)
    for mean_over in (0, 27):
        _fd(G.bce(z, t, mean_over)[1].reshape(-1), lambda x: float(G.bce(x, t, mean_over)[2][0]), z, "bce dz mean_over=%d" % mean_over)


def test_dmr_tail_gradients_against_central_differences():
    rng = np.random.default_rng(8)
    B, T, E, C = 3, 4, 2, 5
    p = {k: (v.astype(F64) if v.dtype == F32 else v) for k, v in _tail_problem(rng, B, T, E, C).items()}
    p["cate_id"][:] = [4, 0, 2]                                                # distinct: dV_rows are the rows of dV
    mm, cid = p["match_mask"], p["cate_id"]

    def match(uv, V):
        _, _, rel, U2, _ = G.dmr_tail_fwd(p["hist"], p["item_eb"], uv, mm, V, cid)
        return float((p["dU2"] * U2).sum() + (p["d_rel"] * rel).sum())

    d_uv, dvr = G.dmr_tail_bwd_match(p["dU2"], p["d_rel"], p["uv"], mm, p["V"], cid)
    dV = np.zeros_like(p["V"])
    dV[cid] = dvr
    _fd(d_uv, lambda x: match(x, p["V"]), p["uv"], "tail bwd_match d_uv")
    _fd(dV, lambda x: match(p["uv"], x), p["V"], "tail bwd_match dV")

    ctx = p["d_ctx"][:, :2 * E].reshape(B, T, 2 * E)

    def hist_side(hist, item):
        hs, pr, _, _, _ = G.dmr_tail_fwd(hist, item, p["uv"], mm, p["V"], cid)
        return float((p["d_sum"] * hs).sum() + (p["d_prod"] * pr).sum() + ((p["f1"] + p["f2"]) * hist).sum()
                     + (p["d_item_direct"] * item).sum() + (ctx * item[:, None, :]).sum())

    hs = G.dmr_tail_fwd(p["hist"], p["item_eb"], p["uv"], mm, p["V"], cid)[0]
    dh, di = G.dmr_tail_bwd_hist(p["f1"], p["f2"], p["d_sum"], p["d_prod"], p["item_eb"], hs, p["d_item_direct"], p["d_ctx"],
                                 np.zeros_like(p["hist"]))
    _fd(dh, lambda x: hist_side(x, p["item_eb"]), p["hist"], "tail bwd_hist d_hist")
    _fd(di, lambda x: hist_side(p["hist"], x), p["item_eb"], "tail bwd_hist d_item")


def test_att_feat_gradient_against_central_differences():
    rng = np.random.default_rng(9)
    h, q, df = rng.standard_normal((2, 3, 4)), rng.standard_normal((2, 3, 4)), rng.standard_normal((6, 16))
    dh, dq = G.att_feat_bwd(h, q, df)
    _fd(dh, lambda x: float((df * G.att_feat_fwd(x, q)).sum()), h, "att_feat d_hist")
    _fd(dq, lambda x: float((df * G.att_feat_fwd(h, x)).sum()), q, "att_feat d_q")


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_softmax_weight_gradient_against_central_differences(scale):
    rng = np.random.default_rng(10)
    B, T, E = 3, 5, 4
    s, h, dx = 2 * rng.standard_normal((B, T)), rng.standard_normal((B, T, E)), rng.standard_normal((B, T, E))
    m = np.where(np.arange(T)[None] < np.array([T, 3, 1])[:, None], 0.0, -1e9)
    w = G.softmax_weight_fwd(s, m, h, scale)[0]
    ds, dh = G.softmax_weight_bwd(w, h, dx, scale)
    _fd(ds, lambda x: float((dx * G.softmax_weight_fwd(x, m, h, scale)[1]).sum()), s, "softmax_weight dscore")
    assert not ds[1, 3:].any() and not ds[2].any()                              # masked positions, and a one-position softmax
    # d_hist = w * dx_att is the gradient with w held fixed (hist also feeds the score through the attention MLP; that path
    # returns through dscore)
    _fd(dh, lambda x: float((dx * (w[:, :, None] * x)).sum()), h, "softmax_weight d_hist")
