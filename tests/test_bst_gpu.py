"""BST on the GPU: the new kernels of csrc/bst_ops.hip against tests/bst_ref.py in float64, whole train steps against the
goldens and the restatement, dropout, inference, and the trainer.

Tolerance, everywhere: err = max|got - ref64| / max|ref64| per tensor against bst_ref.py in float64; the bound is 8 x the same
error of bst_ref.py evaluated in float32 on the same inputs, floor 1e-6 (the factor 8: a different summation order).  Both
errors are printed.  Parameters after Adagrad go through test_bst.param_bounds (test_bst.py says why, and why
bst.k_liner.bias is only held to a noise bound and to what one step can move).

Tiles, and the sizes one past them:
  * attention: a block is 64 rows (queries; keys in the dK / dV pass) of one (sample, head) and walks the other side in LDS
    tiles of 64: L 1, 2, 3, 63, 64, 65 (= K - 1, K, K + 1 and Q + 1), 129 (2 K + 1); a head row is 4 lanes x up to 4 float4
    chunks: (d_k, d_v) (4, 4) = one lane busy, (8, 12) = uneven lanes and d_k != d_v, (48, 48) = the net's, 3 chunks a lane,
    (64, 64) = the limit; heads 1, 3, 6; B 1, 5 and 65 x 6 = 390 (sample, head) pairs x 1 row tile — more blocks than the
    32 CUs of an XCD hold at the kernels' 4 to 5 blocks per CU; q / k / v as column ranges of one packed matrix whose row
    stride is 4 floats wider than its columns, and as three matrices; scale 1 and 0.25;
  * add + layer norm: one wave per row, 4 rows a block, columns in strides of 64: widths 1, 4, 12, 64, 65, 288, 290, 1025;
    rows 1, 6, 37;
  * LeakyReLU / add / the glue: 256-thread grid-stride or per-sample loops; B 1, 5, 65 and T 1, 7."""
import os

import numpy as np
import pytest
import torch

import bst_ref as R
from conftest import GOLDEN
from test_bst import bound_of, param_bounds

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
F32_EPS = float(np.finfo(np.float32).eps)
WORST = {}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _close(name, got, ref64, ref32):
    got = _n(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert np.isfinite(got).all(), name
    e, e32 = R.relerr(got, ref64), R.relerr(ref32, ref64)
    print("%-44s err %.3g  float32-ref err %.3g" % (name, e, e32))
    assert e <= max(8 * e32, 1e-6), (name, e, e32)
    WORST["err"] = max(WORST.get("err", 0.0), e)
    return e


@pytest.fixture(scope="module")
def ops(engine_lib):
    from paddlerec_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ attention
def _mha_case(ops, rng, B, L, H, dk, dv, packed, scale, p=0.0, amp=1.0, seed=77, stream=5):
    tag = "B%d L%d H%d d%d/%d %s s%g p%g" % (B, L, H, dk, dv, "packed" if packed else "split", scale, p)
    wk, wv = H * dk, H * dv
    if packed:
        M = (rng.standard_normal((B * L, 2 * wk + wv + 4)) * amp).astype(F32)
        tM = _t(M)
        cut = lambda a: (a[:, :wk], a[:, wk:2 * wk], a[:, 2 * wk:2 * wk + wv])
        (q, k, v), (tq, tk, tv) = cut(M), cut(tM)
    else:
        q, k = ((rng.standard_normal((B * L, wk)) * amp).astype(F32) for _ in range(2))
        v = (rng.standard_normal((B * L, wv)) * amp).astype(F32)
        tq, tk, tv = _t(q), _t(k), _t(v)
    mask = None
    if p:                                                      # the mask comes from the EXISTING rec_dropout on ones
        mask = _n(ops.dropout(torch.ones(B * H * L, L, device=DEV), p, seed, stream))
        assert set(np.unique(mask).tolist()) <= {0.0, float(F32(1) / (F32(1) - F32(p)))}
    o64, l64, _ = R.mha_fwd(q, k, v, B, L, H, scale, mask)
    o32, l32, _ = R.mha_fwd(q, k, v, B, L, H, scale, mask, dtype=F32)
    out, lse = ops.mha_fwd(tq, tk, tv, B, L, H, scale, p, seed, stream)
    _close(tag + " out", out, o64, o32)
    _close(tag + " lse", lse, l64, l32)
    out2, lse2 = ops.mha_fwd(tq, tk, tv, B, L, H, scale, p, seed, stream)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)                        # bit-identical rerun
    d_out = rng.standard_normal((B * L, wv)).astype(F32)
    g64 = R.mha_bwd(q, k, v, B, L, H, d_out, scale, mask)
    g32 = R.mha_bwd(q, k, v, B, L, H, d_out, scale, mask, dtype=F32)
    t_do = _t(d_out)
    if packed:
        gM = torch.full((B * L, 2 * wk + wv + 4), 7.0, device=DEV)
        grads = (gM[:, :wk], gM[:, wk:2 * wk], gM[:, 2 * wk:2 * wk + wv])
    else:
        gM, grads = None, None
    got = ops.mha_bwd(tq, tk, tv, B, L, H, out, lse, t_do, scale, p, seed, stream, grads=grads)
    for n, a, b64, b32 in zip(("dq", "dk", "dv"), got, g64, g32):
        _close(tag + " " + n, a, b64, b32)
    if packed:
        assert (gM[:, 2 * wk + wv:] == 7).all()
    got2 = ops.mha_bwd(tq, tk, tv, B, L, H, out, lse, t_do, scale, p, seed, stream)
    assert all(torch.equal(a, b) for a, b in zip(got, got2))
    return (tq, tk, tv), out, lse, got


HEADS = ((4, 4), (48, 48), (64, 64), (8, 12))


@pytest.mark.parametrize("L", [1, 2, 3, 63, 64, 65, 129])
def test_attention_against_float64(ops, L):
    rng = np.random.default_rng(500 + L)
    for i, (dk, dv) in enumerate(HEADS):
        H, B = (1, 3, 6)[(i + L) % 3], (1, 5)[(i + L // 2) % 2]
        _mha_case(ops, rng, B, L, H, dk, dv, packed=bool((i + L) % 2), scale=(1.0, 0.25)[(i + L // 3) % 2])
    _mha_case(ops, rng, 5, L, 6, 48, 48, packed=True, scale=1.0)                   # the net's head shape at every L


def test_attention_more_blocks_than_an_xcd_holds(ops):
    rng = np.random.default_rng(7)
    _mha_case(ops, rng, 65, 9, 6, 8, 12, packed=True, scale=1.0)
    _mha_case(ops, rng, 65, 65, 6, 4, 4, packed=False, scale=0.25)


def test_attention_large_scores_need_the_running_maximum(ops):
    rng = np.random.default_rng(8)
    (tq, tk, _), out, lse, grads = _mha_case(ops, rng, 2, 129, 3, 48, 48, packed=True, scale=1.0, amp=5.4)
    s = (tq[:129, :48] @ tk[:129, :48].t()).abs().max().item()
    assert s > 150, s                                           # exp(s) overflows float32 without the subtraction
    assert all(torch.isfinite(t).all() for t in (out, lse) + tuple(grads))


@pytest.mark.parametrize("L,H,dk,dv,packed", [(65, 3, 48, 48, True), (129, 6, 8, 12, False), (3, 1, 64, 64, True)])
def test_attention_dropout_matches_rec_dropout_masks(ops, L, H, dk, dv, packed):
    rng = np.random.default_rng(900 + L)
    _mha_case(ops, rng, 5, L, H, dk, dv, packed=packed, scale=1.0, p=0.2, seed=1234, stream=(1 << 33) + L)


def test_attention_p_zero_is_the_call_without_dropout(ops):
    rng = np.random.default_rng(9)
    B, L, H, d = 5, 65, 3, 48
    q, k, v = (_t(rng.standard_normal((B * L, H * d)).astype(F32)) for _ in range(3))
    o0, l0 = ops.mha_fwd(q, k, v, B, L, H)
    o1, l1 = ops.mha_fwd(q, k, v, B, L, H, 1.0, 0.0, 999, 42)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    do = _t(rng.standard_normal((B * L, H * d)).astype(F32))
    g0 = ops.mha_bwd(q, k, v, B, L, H, o0, l0, do)
    g1 = ops.mha_bwd(q, k, v, B, L, H, o0, l0, do, 1.0, 0.0, 999, 42)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    o2, _ = ops.mha_fwd(q, k, v, B, L, H, 1.0, 0.2, 999, 42)
    assert not torch.equal(o0, o2)


def test_attention_refuses_what_it_cannot_take(ops):
    from paddlerec_amd._lib import RecError
    q = torch.zeros(8, 12, device=DEV)
    with pytest.raises(RecError):
        ops.mha_fwd(q[:, :6], q[:, :6], q[:, 6:], 1, 8, 1)                         # d_k 6
    with pytest.raises(RecError):
        ops.mha_fwd(q, q, q, 1, 8, 5)                                              # 12 columns, 5 heads
    big = torch.zeros(8193, 4, device=DEV)
    with pytest.raises(RecError, match="8192"):
        ops.mha_fwd(big, big, big, 1, 8193, 1)


# ------------------------------------------------------------------------------------------------ add + layer norm
@pytest.mark.parametrize("n", [1, 4, 12, 64, 65, 288, 290, 1025])
def test_add_layer_norm_against_float64(ops, n):
    rng = np.random.default_rng(40 + n)
    for m in (1, 6, 37):
        for with_r in (False, True):
            xw = rng.standard_normal((m, n + 3)).astype(F32) * 2 + 0.5             # x as a strided view
            x, r = xw[:, :n], (rng.standard_normal((m, n)).astype(F32) if with_r else None)
            if m == 37:                                                            # a constant row: variance 0
                x[5] = 0.25
                if with_r:
                    r[5] = 0.25
            tx, tr = _t(xw)[:, :n], (_t(r) if with_r else None)
            y64, mu64, rs64 = R.add_layer_norm_fwd(x, r)
            y32, mu32, rs32 = R.add_layer_norm_fwd(x, r, dtype=F32)
            tag = "ln m%d n%d r%d" % (m, n, with_r)
            frame = torch.full((m, n + 2), 7.0, device=DEV)
            y, mu, rs = ops.add_layer_norm_fwd(tx, tr, out=frame[:, :n])
            if n > 1:
                _close(tag + " y", y, y64, y32)
            else:
                assert not _n(y).any()                                             # width 1: the row is its own mean
            _close(tag + " mean", mu, mu64, mu32)
            _close(tag + " rstd", rs, rs64, rs32)
            assert (frame[:, n:] == 7).all()
            if m == 37:
                assert not _n(y)[5].any() and abs(_n(rs)[5] - 1e-5 ** -0.5) < 1e-2
            y2, mu2, rs2 = ops.add_layer_norm_fwd(tx, tr)
            assert torch.equal(y2, y) and torch.equal(mu2, mu) and torch.equal(rs2, rs)
            dy = rng.standard_normal((m, n)).astype(F32)
            d64 = R.add_layer_norm_bwd(y64, rs64, dy)
            d32 = R.add_layer_norm_bwd(y32, rs32, dy, dtype=F32)
            dx = ops.add_layer_norm_bwd(y, rs, _t(dy))
            assert torch.isfinite(dx).all()
            if n > 1:
                _close(tag + " dx", dx, d64, d32)
            else:
                assert not _n(dx).any()
            assert torch.equal(ops.add_layer_norm_bwd(y, rs, _t(dy)), dx)
            t_dy = _t(dy)
            assert ops.add_layer_norm_bwd(y, rs, t_dy, out=t_dy) is t_dy and torch.equal(t_dy, dx)       # in place on dy


def test_add_layer_norm_writes_rows_one_onwards_of_the_tower_input(ops):
    rng = np.random.default_rng(41)
    B, L, n = 5, 8, 12
    x, r = (rng.standard_normal((B * L, n)).astype(F32) for _ in range(2))
    Z = torch.full((B, L + 1, n), 7.0, device=DEV)
    y, _, rs = ops.add_layer_norm_fwd(_t(x), _t(r), out=Z, out_group=L)
    flat, _, _ = ops.add_layer_norm_fwd(_t(x), _t(r))
    assert y is Z and (Z[:, 0] == 7).all() and torch.equal(Z[:, 1:].reshape(B * L, n), flat)
    dy = _t(rng.standard_normal((B * L, n)).astype(F32))
    assert torch.equal(ops.add_layer_norm_bwd(Z, rs, dy, y_group=L), ops.add_layer_norm_bwd(flat, rs, dy))


# ------------------------------------------------------------------------------------------------ LeakyReLU, add
def test_leaky_relu_zeros_in_place_and_strided(ops):
    rng = np.random.default_rng(42)
    for m, n in ((1, 1), (37, 130), (6, 288)):
        xw = rng.standard_normal((m, n + 2)).astype(F32)
        xw[0, 0] = 0.0
        xw[-1, n - 1] = -0.0
        if n > 4:
            xw[m // 2, 3], xw[m // 2, 4] = -0.0, 0.0
        x = xw[:, :n]
        tw = _t(xw)
        y = ops.leaky_relu_fwd(tw[:, :n], 0.01, out=torch.empty(m, n, device=DEV))                 # out of place
        want = R.leaky_relu_fwd(x, 0.01, dtype=F32)
        assert np.array_equal(_n(y), want) and np.array_equal(np.signbit(_n(y)), np.signbit(want))  # -0 * slope = -0
        dy = rng.standard_normal((m, n)).astype(F32)
        dx = ops.leaky_relu_bwd(y, _t(dy), 0.01, out=torch.empty(m, n, device=DEV))
        want_dx = np.where(x > 0, dy, F32(0.01) * dy)                                              # x > 0 ? 1 : slope
        assert np.array_equal(_n(dx), want_dx)
        assert _n(dx)[0, 0] == F32(0.01) * dy[0, 0] and _n(dx)[-1, n - 1] == F32(0.01) * dy[-1, n - 1]
        assert ops.leaky_relu_fwd(tw[:, :n], 0.01) is not None and np.array_equal(_n(tw[:, :n]), want)   # in place, strided
        assert np.array_equal(_n(tw[:, n:]), xw[:, n:])
        t_dy = _t(dy)
        ops.leaky_relu_bwd(tw[:, :n], t_dy, 0.01)                                                  # in place on dy
        assert np.array_equal(_n(t_dy), want_dx)
        a, b = _t(xw)[:, :n], _t(dy)
        s = ops.bst_add(a, b, out=torch.empty(m, n, device=DEV))
        assert np.array_equal(_n(s), x + dy) and np.array_equal(_n(ops.bst_add(a, None, out=torch.empty(m, n, device=DEV))), x)


# ------------------------------------------------------------------------------------------------ glue
@pytest.mark.parametrize("B", [1, 5, 65])
@pytest.mark.parametrize("T", [1, 7])
def test_tail_glue(ops, B, T):
    rng = np.random.default_rng(B * 10 + T)
    w = (4, 8, 4)
    dm, L = sum(w), T + 1
    counts = (9, 5, 6, 9, 5, 6, 11)
    tables = [rng.standard_normal((c, x)).astype(F32) for c, x in zip(counts, w + w + (dm,))]
    feed = np.concatenate([rng.integers(0, c, (B, T if i < 3 else 1)) for i, c in enumerate(counts)], 1).astype(np.int64)
    t_feed = _t(feed)                                                              # the ids as column ranges of one feed matrix
    cols = np.cumsum([0, T, T, T, 1, 1, 1, 1])
    ids = [t_feed[:, cols[i]:cols[i + 1]] for i in range(7)]
    nid = [feed[:, cols[i]:cols[i + 1]] for i in range(7)]
    X, Z = torch.full((B * L, dm), 7.0, device=DEV), torch.full((B, L + 1, dm), 7.0, device=DEV)
    status = ops.new_status(torch.device(DEV))
    ops.bst_embed_fwd(ids, [_t(t) for t in tables], X, Z, status)
    hist = np.concatenate([tables[i][nid[i]] for i in range(3)], 2)
    tgt = np.concatenate([tables[i][nid[i]] for i in range(3, 6)], 2)
    assert np.array_equal(_n(X), np.concatenate([hist, tgt], 1).reshape(B * L, dm))
    assert np.array_equal(_n(Z[:, 0]), tables[6][nid[6][:, 0]]) and (Z[:, 1:] == 7).all() and int(status.item()) == 0
    bad = feed.copy()
    bad[0, cols[1]] = counts[1]                                                    # one past the cat table
    t_bad = _t(bad)
    ops.bst_embed_fwd([t_bad[:, cols[i]:cols[i + 1]] for i in range(7)], [_t(t) for t in tables], X, Z, status)
    assert int(status.item()) != 0 and not _n(X)[0, w[0]:w[0] + w[1]].any()
    dX = rng.standard_normal((B * L, dm + 1)).astype(F32)
    got = ops.bst_embed_bwd(_t(dX)[:, :dm], B, T, w)
    d3, c = dX[:, :dm].reshape(B, L, dm), 0
    for s in range(3):
        assert np.array_equal(_n(got[s]), d3[:, :T, c:c + w[s]].reshape(B * T, w[s]))
        assert np.array_equal(_n(got[s + 3]), d3[:, T, c:c + w[s]])
        c += w[s]
    z = rng.standard_normal((B * (L + 1), 1)).astype(F32)
    bias = np.asarray([0.3], F32)
    y = ops.bst_possum_fwd(_t(z), _t(bias), B)
    y64 = z.astype(np.float64).reshape(B, L + 1).sum(1, keepdims=True) + 0.3
    _close("possum B%d T%d" % (B, T), y, y64, (z.reshape(B, L + 1).sum(1, keepdims=True, dtype=F32) + bias).astype(F32))
    dy = rng.standard_normal((B, 1)).astype(F32)
    db = torch.zeros(1, device=DEV)
    dz = ops.bst_possum_bwd(_t(dy), L + 1, db)
    assert np.array_equal(_n(dz), np.repeat(dy, L + 1, 1).reshape(-1, 1))
    _close("possum dbias", db, dy.astype(np.float64).sum().reshape(1), dy.sum(dtype=F32).reshape(1))
    db2 = torch.zeros(1, device=DEV)
    ops.bst_possum_bwd(_t(dy), L + 1, db2)
    assert torch.equal(db, db2)


# ------------------------------------------------------------------------------------------------ whole steps
@pytest.fixture(scope="module", params=("bst_da.npz", "bst_n.npz"))
def gold(request):
    g, p, feeds, cfg = R.load_golden(os.path.join(GOLDEN, request.param))
    return dict(name=request.param, g=g, p=p, feeds=feeds, cfg=cfg)


def _layer(gold, **kw):
    from paddlerec_amd.bst import BSTLayer
    p, cfg = gold["p"], gold["cfg"]
    tab = lambda n: p["bst.%s.weight" % n].shape
    fc = [p["bst.dnn_linear_%d.weight" % i].shape[1] for i in range(R.num_dnn(p) - 1)]
    args = dict(dropout_rate=0.0, prepostprocess_dropout=0.0)
    args.update(kw)
    m = BSTLayer(tab("userid_attr")[0], tab("hist_item_emb_attr")[1], tab("hist_cat_emb_attr")[1],
                 tab("hist_position_emb_attr")[1], "relu", True, True, tab("hist_item_emb_attr")[0], tab("hist_cat_emb_attr")[0],
                 tab("hist_position_emb_attr")[0], 1, tab("userid_attr")[1], cfg["d_key"], cfg["d_value"], cfg["n_head"],
                 args["dropout_rate"], cfg["post"], cfg["pre"], args["prepostprocess_dropout"], p["bst.hid_l.weight"].shape[1],
                 0.0, fc, device=DEV)
    m.set_dict(p)
    return m


def _feeds(gold):
    f = gold["feeds"]
    return [_t(f[k]) for k in ("userid", "hist_item", "hist_cat", "hist_position", "target_item", "target_cat",
                               "target_position")], _t(f["label"])


def test_layer_three_train_steps_and_infer(engine_lib, gold):
    """Each step is checked from the state the device is in: the restatement takes the layer's parameters and accumulators,
    so a sign-like first step (|g| near epsilon) cannot desynchronise the later comparisons.

    The gradients of bst.q_liner.* in bst_da are the sensitive ones: sum_j dS_ij k_j with sum_j dS_ij = 0 and keys dominated
    by their common part k_liner.bias, 1e-5 of the terms left.  They hold because rec_mha_bwd divides D_i by the recomputed
    weights' own sum (with dO . O, or without the division, q_liner.bias missed the bound at the third step: 2.58e-05 and
    4.72e-05 against 8 x 3.18e-06; now 1.81e-05)."""
    g, cfg, fd = gold["g"], gold["cfg"], gold["feeds"]
    m = _layer(gold)
    feeds, label = _feeds(gold)
    B, T = fd["hist_item"].shape
    for step in range(3):
        p_now = {k: _n(v).astype(np.float64) for k, v in m.state_dict().items()}
        acc = {k: _n(v).astype(np.float64) for k, v in m._acc.items()}
        r64 = R.train_step(p_now, acc, fd, cfg, None, R.LR)
        r32 = R.train_step(p_now, acc, fd, cfg, None, R.LR, dtype=F32)
        loss, pred = m.train_step(feeds, label)
        _close("step %d pred" % step, pred, r64[0], r32[0])
        _close("step %d loss" % step, loss, r64[1], r32[1])
        grads = m.last_gradients()
        noise = 32 * F32_EPS * R.kbias_noise_scale(R.forward_backward(p_now, fd, cfg)[3], B, T + 1, cfg["n_head"])
        pb = param_bounds(r64, r32, p_now, acc=acc)
        sd = m.state_dict()
        for k in p_now:
            if k in R.STRUCTURAL_ZERO:
                gk = np.abs(_n(grads[k])).max()
                print("step %d %-34s |g| %.3g  noise bound %.3g" % (step, k, gk, noise))
                assert gk <= noise and np.abs(_n(sd[k]) - p_now[k]).max() <= R.LR * (1 + 1e-3), k
                continue
            _close("step %d g_%s" % (step, k), grads[k], r64[2][k], r32[2][k])
            over = np.abs(_n(sd[k]).astype(np.float64) - r64[3][k]) - pb[k]
            assert (over <= 0).all(), (step, k, float(over.max()))
        if step == 0:                                                               # the golden itself
            for k, got, i in (("pred", pred, 0), ("loss", loss, 1)):
                assert R.relerr(_n(got), g[k]) <= bound_of(r32[i], r64[i]) + R.relerr(r64[i], g[k]), k
    assert int(m.status.item()) == 0 and m.step_count == 3
    m.eval()
    now = {k: _n(v) for k, v in m.state_dict().items()}
    pred = m(*feeds)
    _close("infer pred", pred, R.forward_backward(now, fd, cfg, want_grads=False)[0],
           R.forward_backward(now, fd, cfg, dtype=F32, want_grads=False)[0])


def test_layer_train_step_with_dropout_follows_rec_dropout_masks(engine_lib, ops, gold):
    cfg, fd = gold["cfg"], gold["feeds"]
    m = _layer(gold, dropout_rate=0.2, prepostprocess_dropout=0.2)
    feeds, label = _feeds(gold)
    B, T = fd["hist_item"].shape
    L, H = T + 1, cfg["n_head"]
    streams = m.dropout_streams(1)
    assert sorted(streams) == sorted(R.dropout_sites(cfg) + ["att", "ffn"])
    masks = {s: _n(ops.dropout(torch.ones((B * H * L, L) if s == "att" else (B * L, m.d_model), device=DEV), 0.2,
                               m.dropout_seed, st)) for s, st in streams.items()}
    assert all(0.5 < (v != 0).mean() < 0.97 for v in masks.values())
    r64 = R.forward_backward(gold["p"], fd, cfg, masks)
    r32 = R.forward_backward(gold["p"], fd, cfg, masks, dtype=F32)
    loss, pred = m.train_step(feeds, label)
    _close("dropout pred", pred, r64[0], r32[0])
    _close("dropout loss", loss, r64[1], r32[1])
    assert R.relerr(r64[0], R.forward_backward(gold["p"], fd, cfg, want_grads=False)[0]) > 1e-4      # the masks act
    grads = m.last_gradients()
    for k in gold["p"]:
        if k not in R.STRUCTURAL_ZERO:
            _close("dropout g_" + k, grads[k], r64[2][k], r32[2][k])
    m.eval()
    _close("eval pred after a dropout step", m(*feeds),
           R.forward_backward({k: _n(v) for k, v in m.state_dict().items()}, fd, cfg, want_grads=False)[0],
           R.forward_backward({k: _n(v) for k, v in m.state_dict().items()}, fd, cfg, dtype=F32, want_grads=False)[0])


def test_trainer_model_bst_trains_on_the_sample(engine_lib, tmp_path, monkeypatch):
    """--model bst on the sample lines: one epoch of three batches of 4 (L = 101 + 1 from the pre-scan), a checkpoint under
    the reference's names, a finite loss and an AUC."""
    import pickle
    import shutil
    from paddlerec_amd import trainer
    d = tmp_path / "bst"
    (d / "data").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "bst_sample.txt"), d / "data" / "sample.txt")
    monkeypatch.chdir(d)
    out = str(tmp_path / "out")
    (d / "config.yaml").write_text(
        "runner:\n  train_data_dir: data\n  train_batch_size: 4\n  epochs: 1\n  print_interval: 1\n  use_auc: True\n"
        "  model_save_path: %s\nhyper_parameters:\n  optimizer:\n    class: SGD\n    learning_rate: 0.0001\n"
        "  item_emb_size: 8\n  cat_emb_size: 8\n  position_emb_size: 8\n  item_count: 63001\n  user_count: 192403\n"
        "  cat_count: 801\n  position_count: 5001\n  n_encoder_layers: 1\n  d_model: 24\n  d_key: 8\n  d_value: 8\n  n_head: 3\n"
        "  dropout_rate: 0.2\n  postprocess_cmd: \"da\"\n  preprocess_cmd: \"n\"\n  prepostprocess_dropout: 0.2\n"
        "  d_inner_hid: 16\n  relu_dropout: 0.2\n  act: \"relu\"\n  fc_sizes: [32, 16]\n" % out)
    config = trainer.load_yaml(str(d / "config.yaml"))
    assert trainer.guess_model(str(d / "config.yaml")) == "bst"
    summaries, model = trainer.train(config, "bst")
    assert (model.preprocess_cmd, model.postprocess_cmd) == ("da", "da") and model.step_count == 3
    assert len(summaries) == 1 and summaries[0]["batches"] == 3 and summaries[0]["samples"] == 12
    assert np.isfinite(summaries[0]["loss"]) and 0.0 <= summaries[0]["auc"] <= 1.0
    with open(os.path.join(out, "0", "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert "bst.q_liner.weight" in sd and sd["bst.k_liner.weight"].shape == (24, 24) and "bias" in sd
    assert all(np.isfinite(v).all() for v in sd.values())


def test_worst_kernel_error_is_reported():
    print("worst kernel error of this run: %.3g" % WORST.get("err", 0.0))
