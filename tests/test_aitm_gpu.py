"""The AITM kernels (csrc/aitm_ops.hip) and the layer (paddlerec_amd/aitm.py) on the GPU against tests/aitm_ref.py.

Gather: a copy, so the output is compared BIT FOR BIT with NumPy; (B, F, D) below / across a block's pairs, D 5 (scalar, 8 lanes
a pair, 3 idle) and D 8 (float4 when the row stride of `out` allows), tables of 1 and 3 rows, ids 0 and vocab - 1, an id equal
to its field's vocab (inside the buffer: the next field's first row, or the NaN guard rows behind the last field) and a
negative id.  AIT and head: err = max|got - ref64| / max|ref64| per output, bound max(8 x the float32 restatement's error on the
same inputs, 1e-6) (aitm_checks.py).  Wide AUC histogram: integer counts, equal to NumPy's."""
import numpy as np
import pytest
import torch

import aitm_checks as K
import aitm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

VOCABS = {1: [3], 5: [7, 1, 14, 3, 4], 18: [3, 1, 14, 3, 8, 4, 4, 3, 5, 50, 29, 42, 99, 88, 30, 78, 48, 4]}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _close(got, ref64, ref32, what):
    e, b = R.relerr(got.cpu().numpy(), ref64), K.bound_of(ref32, ref64)
    print("%-44s err %.3g  float32-ref err %.3g" % (what, e, b / 8))
    assert e <= b, (what, e, b)


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("ld_kind", ["packed", "wider_mult4", "wider_odd"])
@pytest.mark.parametrize("B,F,D", [(1, 1, 5), (7, 5, 5), (257, 18, 5), (7, 5, 8)])
def test_field_gather(engine_lib, B, F, D, ld_kind):
    from paddlerec_amd import ops
    vocab = VOCABS[F]
    fb = R.field_begin_of(vocab)
    N = int(fb[-1])
    rng = np.random.default_rng(B * 100 + F * 10 + D)
    W = rng.standard_normal((N, D)).astype(np.float32)
    Wbuf = torch.full((N + 2, D), NAN, dtype=torch.float32, device=DEV)          # two guard rows behind the last field
    Wbuf[:N] = _t(W)
    packed = F * D
    pad = {"packed": 0, "wider_mult4": 8 - packed % 4, "wider_odd": 3 if packed % 2 == 0 else 4}[ld_kind]
    assert (packed + pad) % 4 == 0 if ld_kind == "wider_mult4" else ld_kind == "packed" or (packed + pad) % 2 == 1
    clean = np.stack([rng.integers(0, n, B) for n in vocab], 1).astype(np.int64)
    clean[0, :] = [n - 1 for n in vocab]                                         # the last row of every table
    if B > 1:
        clean[1, :] = 0                                                          # id 0 is an ordinary row
        clean[3, :] = clean[2, :]                                                # duplicates
    high, neg = clean.copy(), clean.copy()
    high[0, min(1, F - 1)] = vocab[min(1, F - 1)]                                # == vocab: the next field's first row / a guard row
    neg[B - 1, F - 1] = -1
    both = high.copy()
    both[B - 1, F - 1] = -1 if B * F > 1 else both[B - 1, F - 1]
    fbt = _t(fb)
    for ids, want_flag in ((clean, 0), (high, 1), (neg, 1), (both, 1)):
        outs = []
        for _ in range(2):
            buf = torch.full((B, packed + pad), NAN, dtype=torch.float32, device=DEV)
            out = buf[:, :packed]
            rows = torch.full((B * F,), -7, dtype=torch.int64, device=DEV)
            got, got_rows, status = ops.field_gather_fwd(_t(ids), Wbuf[:N], fbt, out=out, rows_out=rows)
            assert got.data_ptr() == out.data_ptr() and got_rows.data_ptr() == rows.data_ptr()
            assert int(status.item()) == want_flag
            assert pad == 0 or bool(torch.isnan(buf[:, packed:]).all())                # the guard columns stay NaN
            outs.append((out.clone(), rows.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        want, want_rows, flagged = R.gather(W, fb, ids, dtype=np.float32)
        assert flagged == bool(want_flag)
        assert np.array_equal(outs[0][0].cpu().numpy().view(np.uint32), want.view(np.uint32))       # a refused id: +0, never NaN
        assert np.array_equal(outs[0][1].cpu().numpy(), want_rows)
    f = min(1, F - 1)
    assert not outs[0][0][0, f * D:(f + 1) * D].any() and int(outs[0][1][f]) == -1                    # flagged: zero row, row -1
    if B * F > 1:
        assert int(outs[0][1][B * F - 1]) == -1 and not outs[0][0][B - 1, (F - 1) * D:].any()      # the negative id
    got, rows, status = ops.field_gather_fwd(_t(clean), Wbuf[:N], fbt)                                # everything allocated
    assert got.is_contiguous() and tuple(got.shape) == (B, packed) and tuple(rows.shape) == (B * F,) and int(status.item()) == 0
    assert np.array_equal(rows.cpu().numpy(), (clean + fb[None, :-1]).reshape(-1))


def test_gathered_rows_are_what_the_grouping_takes_and_minus_one_is_dropped(engine_lib):
    """rows_out -> ops.ids_group(rows, total_rows, padding_idx=None): a refused id's -1 is in no group, so no row moves for it."""
    from paddlerec_amd import ops
    vocab = VOCABS[5]
    fb = R.field_begin_of(vocab)
    ids = np.array([[6, 0, 13, 3, 0], [0, 0, 2, 1, -1], [6, 1, 2, 1, 3]], np.int64)        # (0,3): 3 == vocab; (1,4): -1; (2,1): 1 == vocab
    _, rows, status = ops.field_gather_fwd(_t(ids), torch.zeros(int(fb[-1]), 5, device=DEV), _t(fb))
    assert int(status.item()) == 1 and rows.cpu().tolist().count(-1) == 3
    groups, _ = ops.ids_group(rows, int(fb[-1]), None, ops.Workspace(DEV))
    spos, uniq, offs = groups.host()
    keep = np.nonzero(rows.cpu().numpy() >= 0)[0]
    assert sorted(spos.tolist()) == keep.tolist() and (uniq >= 0).all() and uniq.tolist() == sorted(set(rows.cpu().numpy()[keep].tolist()))
    assert int(offs[-1]) == len(keep)


# ------------------------------------------------------------------------------------------------ AIT
AIT_CASES = [(1, 2, 32, 0), (7, 2, 32, 0), (130, 2, 32, 0), (5, 1, 32, 0), (9, 3, 5, 0), (6, 2, 72, 0), (7, 2, 32, 8), (9, 3, 5, 3),
             (3, 8, 256, 0), (3, 8, 255, 0)]


@pytest.mark.parametrize("B,T,d,pad", AIT_CASES)
def test_ait_fwd_bwd(engine_lib, B, T, d, pad):
    """(130, 2, 32): 8 lanes a sample, 32 samples a block, a ragged fifth block; (9, 3, 5) the scalar form; (6, 2, 72): 18
    chunks on 32 lanes; (3, 8, 256 / 255): the limits, 64 lanes, and four scalar column passes; pad: row strides wider than
    3 d, with NaN guard columns.  Sample 0 has scores of magnitude ~80."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(B * 1000 + T * 100 + d)
    qkv = rng.standard_normal((B * T, 3 * d)).astype(np.float32)
    qkv[0, :2 * d] = np.sqrt(80.0 / np.sqrt(d))                                   # token 0 of sample 0: <Q, K> / sqrt(d) = +80
    if T > 1:
        qkv[1, :d], qkv[1, d:2 * d] = np.sqrt(80.0 / np.sqrt(d)), -np.sqrt(80.0 / np.sqrt(d))      # token 1: -80
    g = rng.standard_normal((B, d)).astype(np.float32)
    buf = torch.full((B * T, 3 * d + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :3 * d] = _t(qkv)
    x = buf[:, :3 * d]
    gbuf = torch.full((B, d + pad), NAN, dtype=torch.float32, device=DEV)
    gbuf[:, :d] = _t(g)
    gv = gbuf[:, :d]
    runs = []
    for _ in range(2):
        obuf = torch.full((B, d + pad), NAN, dtype=torch.float32, device=DEV)
        out, prob = ops.ait_fwd(x, T, out=obuf[:, :d])
        dbuf = torch.full((B * T, 3 * d + pad), NAN, dtype=torch.float32, device=DEV)
        dq = ops.ait_bwd(x, prob, gv, T, out=dbuf[:, :3 * d])
        assert pad == 0 or bool(torch.isnan(obuf[:, d:]).all() and torch.isnan(dbuf[:, 3 * d:]).all())
        runs.append((out.clone(), prob.clone(), dq.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                                   # a second run is bit-identical
    out, prob, dq = runs[0]
    assert bool(torch.isfinite(out).all() and torch.isfinite(prob).all() and torch.isfinite(dq).all())
    ref = {dt: R.ait_fwd(qkv, T, dtype=dt) for dt in (np.float64, np.float32)}
    what = "ait B%d T%d d%d pad%d " % (B, T, d, pad)
    _close(out, ref[np.float64][0], ref[np.float32][0], what + "out")
    _close(prob, ref[np.float64][1], ref[np.float32][1], what + "prob")
    # the backward from the DEVICE's prob, as the layer calls it; the float32 restatement from its own
    rb = {dt: R.ait_bwd(qkv, ref[dt][1], g, T, dtype=dt) for dt in (np.float64, np.float32)}
    for name, c0 in (("dQ", 0), ("dK", d), ("dV", 2 * d)):
        _close(dq[:, c0:c0 + d], rb[np.float64][:, c0:c0 + d], rb[np.float32][:, c0:c0 + d], what + name)
    if T == 1:
        assert not dq[:, :2 * d].any() and bool((prob == 1).all())               # one token: dQ and dK are exactly zero
    if T > 1:
        assert float(prob[0, 0]) == 1.0 and float(prob[0, 1]) < 1e-30           # exp(-160) in float32
    zero = ops.ait_bwd(x, prob, torch.zeros(B, d, device=DEV), T)
    assert not zero.any() and zero.is_contiguous() and tuple(zero.shape) == (B * T, 3 * d)
    o2, p2 = ops.ait_fwd(x, T)
    assert torch.equal(o2, out) and o2.is_contiguous()


# ------------------------------------------------------------------------------------------------ head
def _head_inputs(B, d, rng):
    tc, ait = rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)
    w = [(rng.standard_normal(d) / np.sqrt(d)).astype(np.float32) for _ in range(2)]
    b = [np.asarray([v], np.float32) for v in (0.3, -0.2)]
    click = rng.integers(0, 2, B).astype(np.int64)
    buy = (click & rng.integers(0, 2, B)).astype(np.int64)
    return tc, ait, w, b, click, buy


def _strided(a, pad):
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _t(a)
    return buf[:, :a.shape[1]]


@pytest.mark.parametrize("B,d,pad", [(1, 32, 0), (7, 32, 0), (300, 32, 0), (7, 32, 4), (300, 32, 3), (7, 5, 0), (5, 72, 0)])
def test_aitm_head(engine_lib, B, d, pad):
    """B 300: 8 lanes a sample, 32 samples a block, ten blocks; pad 3: the scalar form; logits of order 1, samples on both
    sides of the hinge; grad_scale 1 and 1 / B; dz == NULL."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(B * 10 + d + pad)
    tc, ait, w, b, click, buy = _head_inputs(B, d, rng)
    if B > 1:
        u0, u1 = 1.5 * w[0] / (w[0] @ w[0]), 1.5 * w[1] / (w[1] @ w[1])          # <u, w> = 1.5
        tc[0], ait[0] = u0, -u1                                                  # pCTR above pCVR ...
        tc[1], ait[1] = -u0, u1                                                  # ... and below
    args = (_strided(tc, pad), _strided(ait, pad), _t(w[0]).reshape(d, 1), _t(b[0]), _t(w[1]), _t(b[1]), _t(click), _t(buy))
    for scale in (1.0, 1.0 / B):
        ref = {dt: R.head(tc, ait, w[0], b[0], w[1], b[1], click, buy, 0.6, scale, dtype=dt) for dt in (np.float64, np.float32)}
        got = ops.aitm_head(*args, 0.6, scale)
        again = ops.aitm_head(*args, 0.6, scale)
        for x, y in zip(got, again):
            assert torch.equal(x, y)                                               # a second run is bit-identical
        assert tuple(got[0].shape) == (B, 2) and tuple(got[1].shape) == (B, 3) and tuple(got[2].shape) == (B, 2)
        for i, what in enumerate(("pred", "cost", "dz")):
            _close(got[i], ref[np.float64][i], ref[np.float32][i], "head B%d d%d pad%d scale %.3g %s" % (B, d, pad, scale, what))
        if B > 1:
            over = got[0][:, 1] > got[0][:, 0]
            assert bool(over[1]) and not bool(over[0]) and float(got[1][0, 2]) == 0.0 and float(got[1][1, 2]) > 0.5
        no_hinge = {dt: R.head(tc, ait, w[0], b[0], w[1], b[1], click, buy, 0.0, scale, dtype=dt)[2] for dt in (np.float64, np.float32)}
        _close(ops.aitm_head(*args, 0.0, scale)[2], no_hinge[np.float64], no_hinge[np.float32], "head no hinge dz")
    # the hinge's share of dz alone: with grad_scale 0 the BCE share is exactly 0 (its factor is finite: p (1 - p) is floored)
    pure = R.head(tc, ait, w[0], b[0], w[1], b[1], click, buy, 0.6, 0.0)[2]
    pure32 = R.head(tc, ait, w[0], b[0], w[1], b[1], click, buy, 0.6, 0.0, dtype=np.float32)[2]
    _close(ops.aitm_head(*args, 0.6, 0.0)[2], pure, pure32, "head hinge-only dz")
    pred, cost, none = ops.aitm_head(*args, 0.6, 1.0 / B, want_grad=False)                            # dz = NULL
    assert none is None and torch.equal(pred, got[0]) and torch.equal(cost, got[1])


def test_aitm_head_hinge_gradient_does_not_depend_on_grad_scale(engine_lib):
    """The hinge is a batch SUM beside two means: its share of dz, dz(constraint_w) - dz(0), is the same at grad_scale 1 and
    1 / B, namely the dz of grad_scale 0 (there the BCE share is exactly 0).  Rounding: dz(constraint_w) rounds the sum of the
    two shares and the product with p (1 - p), dz(0) and the pure hinge round one product each, every rounding within 2^-24
    of its result, and |pure| <= |dz_a| + |dz_b|: the difference is within 3 * 2^-24 (|dz_a| + |dz_b|) of the pure hinge."""
    from paddlerec_amd import ops
    B, d = 64, 32
    rng = np.random.default_rng(3)
    tc, ait, w, b, click, buy = _head_inputs(B, d, rng)
    args = (_t(tc), _t(ait), _t(w[0]), _t(b[0]), _t(w[1]), _t(b[1]), _t(click), _t(buy))
    pure = ops.aitm_head(*args, 0.6, 0.0)[2].double()
    assert bool((pure[:, 1] >= 0).all() and (pure[:, 0] <= 0).all() and (pure[:, 1] > 0).any() and (pure[:, 1] == 0).any())
    for scale in (1.0, 1.0 / B):
        dz_a, dz_b = ops.aitm_head(*args, 0.6, scale)[2].double(), ops.aitm_head(*args, 0.0, scale)[2].double()
        lim = 3 * 2.0 ** -24 * (dz_a.abs() + dz_b.abs())
        assert bool(((dz_a - dz_b - pure).abs() <= lim).all()), scale


def test_aitm_head_saturated_sigmoids(engine_lib):
    """Logits of exactly +-20 and +-100 (w = e_0, b = 0, x[:, 0] = the logit; the other columns meet zero weights): in float32
    sigmoid(20) is 1 and exp(100) overflows, so p is 0, 1 or exp(-20) to a few ulp on any float32 evaluation.  The cost is
    finite and at most 100 (the clamp), and cost and dz equal the restated chain evaluated in float32 to 1e-6 of the
    tensor's scale — exact values or a few ulp of 2^-24 ~ 6e-8 — where the float64 chain has another p entirely
    (1 - 2e-9), which is why this case is held against the float32 restatement and not under the 8 x rule."""
    from paddlerec_amd import ops
    d = 32
    logit = np.array([[20, -20], [-20, 20], [100, -100], [-100, 100], [100, 100], [-100, -100], [20, 100], [0.5, -0.5]], np.float32)
    B = len(logit)
    rng = np.random.default_rng(9)
    tc, ait = rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)
    tc[:, 0], ait[:, 0] = logit[:, 0], logit[:, 1]
    e0 = np.zeros(d, np.float32)
    e0[0] = 1
    zero = np.zeros(1, np.float32)
    for click, buy in ((np.zeros(B, np.int64), np.zeros(B, np.int64)), (np.ones(B, np.int64), np.ones(B, np.int64))):
        for scale in (1.0, 1.0 / B):
            pred, cost, dz = ops.aitm_head(_t(tc), _t(ait), _t(e0), _t(zero), _t(e0), _t(zero), _t(click), _t(buy), 0.6, scale)
            assert bool(torch.isfinite(pred).all() and torch.isfinite(cost).all() and torch.isfinite(dz).all())
            assert float(cost.max()) <= 100.0 and float(cost[:, :2].max()) == 100.0
            r = R.head(tc, ait, e0, zero, e0, zero, click, buy, 0.6, scale, dtype=np.float32)
            for got, want, what in zip((pred, cost, dz), r, ("pred", "cost", "dz")):
                e = R.relerr(got.cpu().numpy(), want)
                print("saturated %s scale %.3g err %.3g" % (what, scale, e))
                assert e <= 1e-6, (what, e)
            assert float(pred[2, 0]) == 1.0 and float(pred[2, 1]) == 0.0 and not dz[2:6].any()      # p (1 - p) = 0: no gradient


# ------------------------------------------------------------------------------------------------ wide AUC histogram
@pytest.mark.parametrize("T", [100000, 16000])
@pytest.mark.parametrize("B", [1, 1000])
def test_auc_histogram_wide(engine_lib, B, T):
    from paddlerec_amd import ops
    rng = np.random.default_rng(B + T)
    pred = rng.random((B, 2)).astype(np.float32)
    pred[0, 1] = 1.0
    if B > 1:
        pred[1, 1], pred[2, 1], pred[3, 1] = 0.0, 1.0, pred[4, 1]               # exactly 0 and 1, a shared bucket
    label = rng.integers(0, 2, B).astype(np.int64)
    pt, lt = _t(pred), _t(label)
    pos, neg = (torch.zeros(T + 1, dtype=torch.int64, device=DEV) for _ in range(2))
    want_pos, want_neg = R.auc_histogram(pred[:, 1], label, T)
    for n in (1, 2):                                                             # the counts accumulate
        ops.auc_histogram_wide(pt[:, 1], lt, pos, neg, T)                        # a column view: no copy
        assert np.array_equal(pos.cpu().numpy(), n * want_pos) and np.array_equal(neg.cpu().numpy(), n * want_neg)
    assert int(pos.sum() + neg.sum()) == 2 * B and int((pos + neg)[T]) >= 2
    pos2, neg2 = (torch.zeros(T + 1, dtype=torch.int64, device=DEV) for _ in range(2))
    ops.auc_histogram_wide(pt[:, 1].contiguous(), lt, pos2, neg2, T)
    assert torch.equal(2 * pos2, pos) and torch.equal(2 * neg2, neg)
    from paddlerec_amd._lib import RecError
    with pytest.raises(RecError):                                                # the LDS histogram keeps its limit
        ops.auc_histogram(pt[:, 1].contiguous(), lt, pos2, neg2, T)


def test_refusals_return_before_any_launch(engine_lib):
    import test_aitm_abi as A
    A.test_field_gather_refusals_without_gpu(engine_lib)
    A.test_ait_refusals_without_gpu(engine_lib)
    A.test_aitm_head_refusals_without_gpu(engine_lib)
    A.test_auc_histogram_wide_refusals_without_gpu(engine_lib)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the layer
def test_both_recorded_steps_of_the_golden(engine_lib):
    G = K.gold()
    m = K.layer_of(G, DEV, None)
    K.check_layer(G, m, "gpu")
    m2 = K.layer_of(G, DEV, None)                                                # bit-identical on a rerun from the same state
    m2.set_dict(G["p"])
    for s in range(G["steps"]):
        m2.train_step(*K.feeds(G, s, DEV), G["lr"])
    for key, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[key]), key


def test_one_step_with_dropout_under_rebuilt_masks(engine_lib):
    from paddlerec_amd import ops
    G = K.gold()
    m = K.layer_of(G, DEV, None, drop_prob=(0.1, 0.3, 0.3))
    masks = K.masks_of(m, 1, 7, ops.dropout)
    assert sorted(masks) == sorted(R.SITES)
    for site, v in masks.items():                                                # 0 or 1 / (1 - p) of the site's rate
        kept = v[v != 0]
        assert (v == 0).any() and np.allclose(kept, 1 / (1 - (0.1 if site.endswith("0") else 0.3)), rtol=1e-6), site
    K.check_layer(G, m, "gpu dropout", steps=1, dropout=ops.dropout)
    a = m.predict(K.feeds(G, 0, DEV)[0])                                         # predictions never see Dropout
    assert torch.equal(a, m.predict(K.feeds(G, 0, DEV)[0]))


def test_an_out_of_field_id_cannot_move_a_neighbouring_table(engine_lib):
    """Id 3 in field 1 (3 rows) is field 2's first row inside the buffer.  With the status check skipped, the step is the
    reference's step without that lookup: field 2's gradient and new rows are those of aitm_ref, which drops it."""
    from helpers import assert_adam_weights_close
    G = K.gold()
    g = G["g"]
    ids = g["ids_0"].copy()
    ids[2, 1] = 3
    m = K.layer_of(G, DEV, None)
    m.set_dict(G["p"])
    _, click, buy = K.feeds(G, 0, DEV)
    m.train_step(_t(ids), click, buy, G["lr"])
    assert int(m.status.item()) == 1
    r64, r32 = K.ref_step(G["p"], None, ids, g["click_0"], g["buy_0"], G["lr"])
    grads = m.last_gradients()
    for k in ("embedding_dict.1.weight", "embedding_dict.2.weight"):
        _close(grads[k], r64["g"][k], r32["g"][k], "oob " + k)
    for k, v in m.state_dict().items():
        assert_adam_weights_close(v.cpu().numpy(), r64["n"][k], G["lr"], 1, err_msg=k)
    # the wrong reading, the lookup landing on field 2's row 0, is far outside that bound
    wrong = r64["g"]["embedding_dict.2.weight"].copy()
    wrong[0] += R.train_step(G["p"], ids, g["click_0"], g["buy_0"], G["lr"])[0]["dX"][2, 5:10]
    assert R.relerr(wrong, r64["g"]["embedding_dict.2.weight"]) > 100 * K.bound_of(r32["g"]["embedding_dict.2.weight"], r64["g"]["embedding_dict.2.weight"])


def test_one_train_step_at_the_shipped_config_sizes(engine_lib, tmp_path):
    """aitm/config.yaml: the 18 real vocabularies (1.35 M rows in all), D 5, dims [128, 64, 32], drop_prob [0.1, 0.3, 0.3]."""
    from paddlerec_amd import trainer
    torch.manual_seed(1)
    sizes = [238635, 98, 14, 3, 8, 4, 4, 3, 5, 467298, 6929, 263942, 106399, 5888, 104830, 51878, 37148, 4]
    cfg = K.aitm_config(tmp_path, feature_vocabulary=[[str(i), n] for i, n in enumerate(sizes)])
    dm = trainer._dygraph_model("aitm")
    m = dm.create_model(cfg, DEV)
    B = 64
    assert tuple(m.emb.shape) == (sum(sizes), 5)
    gen = torch.Generator().manual_seed(2)
    ids = torch.stack([torch.randint(0, n, (B,), generator=gen) for n in sizes], 1)
    ids[0] = torch.tensor(sizes) - 1
    click = torch.randint(0, 2, (B,), generator=gen)
    buy = click & torch.randint(0, 2, (B,), generator=gen)
    before = m.emb.clone()
    metrics, names = dm.create_metrics(DEV)
    loss, metrics, _ = dm.train_forward(m, metrics, (ids, click, buy), cfg)
    assert names == ["click_auc", "purchase_auc"] and np.isfinite(loss.item()) and int(m.status.item()) == 0
    moved = (before != m.emb).any(1).float().mean()
    assert float(moved) > 0.99 and not torch.isnan(m.emb).any()                 # non-lazy Adam with L2: every row moves
    for mt in metrics:
        assert int(mt[0].sum() + mt[1].sum()) == B


def test_trainer_trains_and_infers_on_the_sample(engine_lib, tmp_path):
    from paddlerec_amd import trainer
    cfg = K.aitm_config(tmp_path)
    out, m = trainer.train(cfg, "aitm", device=DEV)
    res = trainer.infer(cfg, "aitm", device=DEV)
    assert len(out) == 2 and out[1]["batches"] == 3 and np.isfinite(out[1]["loss"]) and m.step_count == 6
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 12
    for n in ("click_auc", "purchase_auc"):
        assert 0.0 <= out[1][n] <= 1.0 and 0.0 <= res[1][n] <= 1.0
