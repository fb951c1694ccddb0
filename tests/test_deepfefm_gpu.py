"""DeepFEFM on the HIP kernels (csrc/fefm_ops.hip), the row updates with the L2 term (csrc/sparse_update.hip) and the
layer / trainer on top, against the float64 torch restatement (tests/deepfefm_ref.py) and oracle/deepfm_ref.py."""
import numpy as np
import pytest
import torch

import deepfefm_ref as FR
from helpers import assert_adam_weights_close, assert_close_scaled, load_golden
from oracle import deepfm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_FULL = 1100005            # deepfefm/config.yaml sparse_feature_number


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _problem(B, S, Dn, D, N, seed, stride=None, lo=2, hi=100):
    """Random kernel inputs.  The dense values are shifted (-10 + u * 1e-3 scaled to ids lo..hi) so that the derived ids
    fall inside a small table; padding ids and duplicated rows in every batch."""
    rng = np.random.default_rng(seed)
    F = S + Dn
    P = F * (F - 1) // 2
    stride = stride or (D + 3) // 4 * 4
    W = np.zeros((N, stride), np.float32)
    W[:, :D] = rng.normal(0, 0.3, (N, D)).astype(np.float32)
    W[0] = 0.0
    p = dict(W=W, W1=rng.normal(0, 0.1, (N, 1)).astype(np.float32), dense_w_one=rng.normal(0, 0.5, Dn).astype(np.float32),
             FE=rng.normal(0, 0.3, (P, D, D)).astype(np.float32))
    p["W1"][0] = 0.0
    ids = rng.integers(1, N, (B, S), dtype=np.int64)
    ids[rng.random((B, S)) < 0.1] = 0
    if B > 1:
        ids[1::2, : S // 2] = ids[0::2, : S // 2][: ids[1::2].shape[0]]
    dense = (np.float32(-10.0) + rng.random((B, Dn), dtype=np.float32) * np.float32(1e-3 * (hi - lo) / 100)).astype(np.float32)
    dz = rng.normal(0, 1, B).astype(np.float32)
    d_dnn_in = rng.normal(0, 1, (B, S * D + Dn + P)).astype(np.float32)
    return p, ids, dense, dz, d_dnn_in


def _run(p, ids, dense, dz, d_dnn_in, D, want_d_fe, grad_stride=None, status=None):
    from paddlerec_amd import ops
    W = _t(p["W"])
    S = ids.shape[1]
    st = status if status is not None else ops.new_status(DEV)
    ws = ops.Workspace(DEV)
    y1, y2, dnn_in, ids_all, _ = ops.fefm_fwd(_t(ids), _t(dense), W, _t(p["W1"]), _t(p["dense_w_one"]), _t(p["FE"]), D,
                                              ws, status=st)
    rg, dw1, dfe = ops.fefm_bwd(ids_all, _t(dense), W, _t(p["FE"]), _t(dz), _t(d_dnn_in), S, D, ws,
                                want_d_fe=want_d_fe, status=st, grad_stride=grad_stride)
    torch.cuda.synchronize()
    out = dict(y1=y1, y2=y2, dnn_in=dnn_in, ids_all=ids_all, row_grad=rg, d_dense_w_one=dw1)
    if want_d_fe:
        out["d_FE"] = dfe
    else:
        assert dfe is None
    return {k: v.cpu().numpy() for k, v in out.items()}, int(st.item())


def _reference(p, ids, dense, dz, d_dnn_in, D, dtype=torch.float64, chunk=512):
    """kernel_reference over the batch in chunks (the [B, P, D] gathers of a D 48 batch do not fit at once)."""
    B = len(ids)
    parts = [FR.kernel_reference(ids[a:a + chunk], dense[a:a + chunk], p, D, dz[a:a + chunk], d_dnn_in[a:a + chunk], dtype)
             for a in range(0, B, chunk)]
    o = {k: np.concatenate([q[k] for q in parts]) for k in ("y1", "y2", "dnn_in", "ids_all", "row_grad")}
    o["d_dense_w_one"] = sum(q["d_dense_w_one"] for q in parts)
    o["d_FE"] = sum(q["d_FE"] for q in parts)
    return o


KEYS = ("y1", "y2", "dnn_in", "row_grad", "d_dense_w_one", "d_FE")


def _scaled_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got.reshape(want.shape) - want) / (np.abs(want) + np.abs(want).max() + 1e-300)).max())


def _check(p, ids, dense, dz, d_dnn_in, D, want_d_fe, rel=2e-5, grad_stride=None):
    got, st = _run(p, ids, dense, dz, d_dnn_in, D, want_d_fe, grad_stride)
    assert st == 0
    want = _reference(p, ids, dense, dz, d_dnn_in, D)
    assert np.array_equal(got["ids_all"], want["ids_all"])
    rg = got["row_grad"]
    assert not rg[:, D:].any(), "pad columns of row_grad must be written 0"
    assert not rg[(want["ids_all"] == 0).reshape(-1)].any(), "rows of padding positions must be 0"
    got["row_grad"] = rg[:, :D]
    for k in KEYS:
        if k in got and want[k].size:
            err = _scaled_err(got[k], want[k])
            print("D=%d B=%d %s scaled err %.3e" % (D, len(ids), k, err))
            assert_close_scaled(got[k], want[k], rel, k)
    return got, want


@pytest.mark.parametrize("want_d_fe", [False, True])
@pytest.mark.parametrize("B", [1, 7, 4096])
@pytest.mark.parametrize("D", [1, 4, 9, 16])
def test_fefm_kernels_vs_float64(engine_lib, D, B, want_d_fe):
    """39 fields; padding ids, duplicated rows, a row stride and a gradient stride larger than D."""
    p, ids, dense, dz, dd = _problem(B, 26, 13, D, 160, seed=D * 100 + B, stride=(D + 3) // 4 * 4 + 4)
    assert (ids == 0).any() or B == 1
    _check(p, ids, dense, dz, dd, D, want_d_fe, grad_stride=(D + 3) // 4 * 4 + 8)


@pytest.mark.parametrize("S,Dn,D", [(2, 0, 9), (1, 2, 9), (3, 1, 64), (5, 3, 33), (60, 4, 9)])
def test_fefm_odd_field_counts(engine_lib, S, Dn, D):
    p, ids, dense, dz, dd = _problem(133, S, Dn, D, 160, seed=S * 10 + Dn)
    _check(p, ids, dense, dz, dd, D, True)


@pytest.mark.parametrize("B", [1, 7, 4096])
def test_fefm_dim48(engine_lib, B):
    """config_bigdata.yaml's D 48: every t[b,p] sums 2304 products and the gradients more.  The bound is not picked in
    advance: the float32 restatement's largest scaled error |err| / (|want| + max|want|) against float64 is measured on
    the same inputs at run time, the largest over the six outputs is taken, and the kernel gets 4x that (same precision,
    different summation order).  The float32 restatement runs on ONE CPU thread (its own error depends on how many threads
    torch sums with), so the bound is the same on every machine.  Measured for these seeds: restatement 1.4e-7 at B 1,
    1.5e-7 at B 7, 2.2e-7 at B 4096, i.e. bounds 5.5e-7, 6.0e-7 and 8.8e-7; the kernels' largest error was 1.2e-7
    (row_grad), 1.5e-7 (row_grad) and 3.9e-7 (d_FE).  The test prints every figure."""
    D = 48
    p, ids, dense, dz, dd = _problem(B, 26, 13, D, 160, seed=4800 + B)
    got, st = _run(p, ids, dense, dz, dd, D, True)
    assert st == 0
    want = _reference(p, ids, dense, dz, dd, D)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                 # the float32 restatement's own error depends on how many threads sum
    try:
        w32 = _reference(p, ids, dense, dz, dd, D, torch.float32)
    finally:
        torch.set_num_threads(threads)
    got["row_grad"] = got["row_grad"][:, :D]
    floor = max(_scaled_err(w32[k], want[k]) for k in KEYS)
    bound = 4.0 * floor
    print("D=48 B=%d float32 restatement scaled err %.3e -> bound %.3e" % (B, floor, bound))
    for k in KEYS:
        err = _scaled_err(got[k], want[k])
        print("D=48 B=%d %s kernel scaled err %.3e" % (B, k, err))
        assert err <= bound, (k, err, bound)


def _golden_params():
    g = load_golden("deepfefm_D9")
    n = len(g["fc"]) + 1
    p = {"W": g["W"], "W1": g["W1"], "dense_w_one": g["dense_w_one"], "FE": g["FE"],
         "lin_w": [g["lin_w%d" % i] for i in range(n)], "lin_b": [g["lin_b%d" % i] for i in range(n)]}
    return g, p


def test_fefm_kernels_on_fixture(engine_lib):
    g, p = _golden_params()
    B, S = g["ids"].shape
    rng = np.random.default_rng(0)
    dz = rng.normal(0, 1, B).astype(np.float32)
    dd = rng.normal(0, 1, (B, S * 9 + 13 + 741)).astype(np.float32)
    pk = dict(p, W=np.pad(g["W"], ((0, 0), (0, 3))))
    got, _ = _check(pk, g["ids"], g["dense"], dz, dd, 9, True)
    assert np.array_equal(got["ids_all"][:, S:], g["dense_ids"])
    assert_close_scaled(got["dnn_in"][:, S * 9 + 13:], g["t"], 2e-5, "t")
    assert_close_scaled(got["y1"], g["y1"], 2e-5, "y1")
    assert_close_scaled(got["y2"], g["y2"], 2e-5, "y2")


@pytest.mark.parametrize("draw", ["even", "uniform"])
def test_dense_id_formula_exact_on_a_million_values(engine_lib, draw):
    """int64(dense * 1e5 + 1e6 + 2) as three rounded f32 operations: 1 040 000 evenly spaced values covering [0, 1],
    both ends included, against numpy — every id equal, no tolerance.  A second case draws as many uniform values:
    on those a contracted multiply-add is known to land on other rows (a few per thousand), on the even grid it is not."""
    from paddlerec_amd import ops
    Dn, B = 13, 80000
    if draw == "even":
        dense = np.linspace(0.0, 1.0, B * Dn, dtype=np.float64).astype(np.float32).reshape(B, Dn)
    else:
        dense = np.random.default_rng(1).random((B, Dn), dtype=np.float32)
        dense[0, 0], dense[-1, -1] = 0.0, 1.0
        one_fma = ((dense.astype(np.float64) * 1e5 + 1e6).astype(np.float32) + np.float32(2)).astype(np.int64)
        assert (FR.derived_ids(dense) != one_fma).sum() > 1000
    assert dense[0, 0] == 0.0 and dense[-1, -1] == 1.0
    want = FR.derived_ids(dense)
    W = torch.zeros(N_FULL, 4, device=DEV)
    st = ops.new_status(DEV)
    ids = torch.ones(B, 1, dtype=torch.int64, device=DEV)
    _, _, _, ids_all, _ = ops.fefm_fwd(ids, _t(dense), W, torch.zeros(N_FULL, 1, device=DEV), torch.zeros(Dn, device=DEV),
                                       torch.zeros(Dn * (Dn + 1) // 2, 1, 1, device=DEV), 1, ops.Workspace(DEV), status=st)
    got = ids_all.cpu().numpy()
    assert int(st.item()) == 0
    assert np.array_equal(got[:, 1:], want)
    assert want.min() == 1000002 and want.max() == 1100002


def test_out_of_range_and_nan_dense_values_raise_the_flag(engine_lib):
    """Derived ids outside the table (negative, beyond N, NaN, inf) and sparse ids outside it are flagged and read as a
    zero row; outputs stay finite and equal the restatement with those positions zeroed."""
    from paddlerec_amd import ops
    D, N = 9, 160
    p, ids, dense, dz, dd = _problem(64, 26, 13, D, N, seed=77)
    got0, st0 = _run(p, ids, dense, dz, dd, D, True)
    assert st0 == 0
    bad_dense = dense.copy()
    bad_dense[3, 0], bad_dense[5, 2], bad_dense[7, 4], bad_dense[9, 12], bad_dense[11, 1] = np.nan, np.inf, -1e30, 0.5, -11.0
    bad_ids = ids.copy()
    bad_ids[2, 1], bad_ids[4, 25], bad_ids[6, 0] = -1, N, 10 ** 12
    st = ops.new_status(DEV)
    got, s = _run(p, bad_ids, bad_dense, dz, dd, D, True, status=st)
    assert s & 1
    for k in KEYS:
        if k not in ("y1", "dnn_in", "d_dense_w_one"):        # those carry the NaN / inf dense value itself (d1 = dense * w)
            assert np.isfinite(got[k]).all(), k
    ia = got["ids_all"]
    assert ia[3, 26] == -1 and ia[5, 28] == -1 and ia[9, 38] == 1050002 and ia[11, 27] < 0
    safe = np.where((ia < 0) | (ia >= N), 0, ia)
    fin = np.where(np.isfinite(bad_dense), bad_dense, 0).astype(np.float32)
    want = FR.kernel_reference(bad_ids, fin, p, D, dz, dd, ids_all=safe)
    assert_close_scaled(got["y2"], want["y2"], 2e-5, "y2")
    assert_close_scaled(got["row_grad"][:, :D], want["row_grad"], 2e-5, "row_grad")
    assert_close_scaled(got["d_FE"], want["d_FE"], 2e-5, "d_FE")


def test_backward_batch_sums_bit_identical_reruns(engine_lib):
    p, ids, dense, dz, dd = _problem(5000, 26, 13, 9, 160, seed=5)
    a, _ = _run(p, ids, dense, dz, dd, 9, True)
    b, _ = _run(p, ids, dense, dz, dd, 9, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------ row updates with the L2 term
@pytest.mark.parametrize("width,stride", [(1, 1), (9, 12), (12, 12), (48, 48), (352, 352)])
@pytest.mark.parametrize("lazy", [True, False])
def test_row_updates_with_l2(engine_lib, width, stride, lazy):
    """rec_sparse_adam_rows_l2 / rec_adam_rows_all_l2 against the NumPy merge + L2Decay + Adam: touched rows only (lazy)
    or every row with g + coeff * w.  A large coefficient (1e-2) so that a missing term cannot hide in the tolerance."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(width + lazy)
    N, n, l2 = 700, 5000, 1e-2
    ids = rng.integers(0, N - 50, n, dtype=np.int64)        # the last 50 rows are never touched
    ids[rng.random(n) < 0.4] = 17
    grad = rng.normal(0, 1, (n, width)).astype(np.float32)
    P = np.zeros((N, stride), np.float32)
    P[:, :width] = rng.normal(0, 0.1, (N, width)).astype(np.float32)
    M, V = np.zeros_like(P), np.zeros_like(P)
    gfull = np.zeros((n, stride), np.float32)
    gfull[:, :width] = grad
    Pt, Mt, Vt, gt = _t(P), _t(M), _t(V), _t(gfull)
    groups, _ = ops.ids_group(_t(ids.reshape(-1, 1)), N, None, ops.Workspace(DEV))
    upd = ops.sparse_adam_rows if lazy else ops.adam_rows_all
    for step in (1, 2):
        pp = ops.segment_partials(groups, gt, stride)
        upd(groups, gt, 1, Pt, Mt, Vt, step, lr=1e-2, partials=pp, l2=l2)
        uniq, merged, _ = R.merge_rows(ids, np.ones(n, bool), gfull)
        if lazy:
            R.adam_update_rows(P, M, V, uniq, merged + np.float32(l2) * P[uniq], step, lr=1e-2)
        else:
            g = np.zeros_like(P)
            g[uniq] = merged
            R.adam_update(P, M, V, g + np.float32(l2) * P, step, lr=1e-2)
    torch.cuda.synchronize()
    for got, want, name in ((Mt, M, "m"), (Vt, V, "v"), (Pt, P, "P")):
        assert_close_scaled(got.cpu().numpy(), want, 1e-5, name)
    moved = np.abs(Pt.cpu().numpy()[-50:, :width] - P[-50:, :width]).max()
    assert moved == 0.0                                     # same as the reference either way ...
    assert (np.abs(M[-50:, :width]).max() > 0) == (not lazy)   # ... which moves untouched rows only when not lazy


@pytest.mark.parametrize("lazy", [True, False])
def test_l2_zero_is_the_old_entry_point_bit_for_bit(engine_lib, lazy):
    """rec_sparse_adam_rows_l2 / rec_adam_rows_all_l2 with a zero coefficient (l2=0.0 selects the _l2 symbol in the
    wrapper) against rec_sparse_adam_rows / rec_adam_rows_all (l2 left out): the C dispatch must run the kernels
    without the term, so every bit agrees."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(3)
    N, n, width = 300, 2000, 12
    ids = rng.integers(0, N, n, dtype=np.int64)
    grad = _t(rng.normal(0, 1, (n, width)).astype(np.float32))
    P0 = rng.normal(0, 0.1, (N, width)).astype(np.float32)
    groups, _ = ops.ids_group(_t(ids.reshape(-1, 1)), N, None, ops.Workspace(DEV))
    upd = ops.sparse_adam_rows if lazy else ops.adam_rows_all
    res = []
    for kw in ({}, {"l2": 0.0}):                           # the old symbol, then the _l2 symbol with coefficient 0
        Pt, Mt, Vt = _t(P0), torch.zeros(N, width, device=DEV), torch.zeros(N, width, device=DEV)
        upd(groups, grad, 1, Pt, Mt, Vt, 1, lr=1e-2, **kw)
        res.append([x.cpu().numpy() for x in (Pt, Mt, Vt)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ the layer
def _layer(p, D, N, fc, **kw):
    from paddlerec_amd.deepfefm import DeepFEFMLayer
    m = DeepFEFMLayer(N, D, 13, 26, fc, device=DEV, **kw)
    sd = {"fefm.embedding.weight": p["W"][:, :D], "fefm.embedding_one.weight": p["W1"],
          "fefm.dense_w_one": p["dense_w_one"], "fefm.field_embeddings": p["FE"]}
    for i, (w, b) in enumerate(zip(p["lin_w"], p["lin_b"])):
        sd["dnn.linear_%d.weight" % i], sd["dnn.linear_%d.bias" % i] = w, b
    m.set_dict(sd)
    return m


def test_layer_matches_fixture_gpu(engine_lib):
    import test_deepfefm
    test_deepfefm.check_layer_on_fixture(DEV, None, 2e-5)


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("train_fe", [False, True])
def test_train_mode_trajectory(engine_lib, lazy, train_fe):
    """5 steps with dropout on against the restatement (float64 gradients, the engine's mask generator, L2 + Paddle
    Adam): loss and prediction per step at 1e-5 as the FFM trajectories, final parameters by assert_adam_weights_close.
    Small table; dense inputs shifted so that the derived ids stay inside it."""
    g, p = _golden_params()
    N, D, fc, lr = g["W"].shape[0], 9, [int(x) for x in g["fc"]], 1e-2
    m = _layer(p, D, N, fc, dropout_rate=0.2, dropout_seed=77, train_field_embeddings=train_fe)
    m.lazy_mode = lazy
    tr = FR.Trainer(p, D, lazy=lazy, train_fe=train_fe, rate=0.2, seed=77)
    rng = np.random.default_rng(21)
    fe0 = m.dense.p["fefm.field_embeddings"].clone()
    for step in range(5):
        ids = rng.integers(0, N, (48, 26), dtype=np.int64)
        ids[:, 0] = 5
        dense = (np.float32(-10.0) + rng.random((48, 13), dtype=np.float32) * np.float32(1e-3)).astype(np.float32)
        label = (rng.random((48, 1)) < 0.4).astype(np.int64)
        loss, pred = m.train_step(_t(ids), _t(dense), _t(label), lr=lr)
        ol, op = tr.train_step(ids, dense, label, lr=lr)
        print("step %d loss %.7f ref %.7f" % (step, float(loss), ol))
        np.testing.assert_allclose(float(loss), ol, rtol=1e-5)
        np.testing.assert_allclose(pred.cpu().numpy(), op, rtol=1e-5, atol=1e-6)
    assert int(m.status.item()) == 0
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    assert_adam_weights_close(sd["fefm.embedding.weight"], tr.p["W"], lr=lr, steps=5, err_msg="W")
    assert_adam_weights_close(sd["fefm.embedding_one.weight"], tr.p["W1"], lr=lr, steps=5, err_msg="W1")
    assert_adam_weights_close(sd["fefm.dense_w_one"], tr.p["dense_w_one"], lr=lr, steps=5, err_msg="dense_w_one")
    for i in range(len(fc) + 1):
        assert_adam_weights_close(sd["dnn.linear_%d.weight" % i], tr.p["lin_w"][i], lr=lr, steps=5, err_msg="w%d" % i)
        assert_adam_weights_close(sd["dnn.linear_%d.bias" % i], tr.p["lin_b"][i], lr=lr, steps=5, err_msg="b%d" % i)
    assert float(sd["bias"][0]) == 0.0
    assert not sd["fefm.embedding.weight"][0].any() and not m.emb_table[:, D:].cpu().numpy().any()
    if train_fe:
        assert_adam_weights_close(sd["fefm.field_embeddings"], tr.p["FE"], lr=lr, steps=5, err_msg="FE")
        assert not torch.equal(fe0, m.dense.p["fefm.field_embeddings"])
    else:
        assert torch.equal(fe0, m.dense.p["fefm.field_embeddings"])          # frozen: bit-identical


@pytest.mark.parametrize("B", [16, 4096])
def test_full_size_step(engine_lib, B):
    """deepfefm/config.yaml: 1 100 005 rows, D 9, the [512, 256, 128, 32] tower, dense values in [0, 1] (derived ids
    1 000 002 ..).  One train step (dropout on, the dygraph default Adam over the whole table); its loss equals the
    restatement's on the same draw."""
    from paddlerec_amd.deepfefm import DeepFEFMLayer
    torch.manual_seed(5)
    fc = [512, 256, 128, 32]
    m = DeepFEFMLayer(N_FULL, 9, 13, 26, fc, device=DEV, dropout_rate=0.2, dropout_seed=9)
    rng = np.random.default_rng(B)
    ids = rng.integers(1, 1000000, (B, 26), dtype=np.int64)
    ids[rng.random((B, 26)) < 0.05] = 0
    dense = rng.random((B, 13), dtype=np.float32)
    dense[0, 0], dense[0, 1] = 0.0, 1.0
    label = (rng.random((B, 1)) < 0.3).astype(np.int64)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    p = {"W": sd["fefm.embedding.weight"], "W1": sd["fefm.embedding_one.weight"], "dense_w_one": sd["fefm.dense_w_one"],
         "FE": sd["fefm.field_embeddings"], "lin_w": [sd["dnn.linear_%d.weight" % i] for i in range(5)],
         "lin_b": [sd["dnn.linear_%d.bias" % i] for i in range(5)]}
    loss, pred = m.train_step(_t(ids), _t(dense), _t(label), lr=1e-3)
    assert int(m.status.item()) == 0
    q = FR.leaves(p, 9)
    with torch.no_grad():
        f = FR.forward(ids, dense, q, 9, drop=(0.2, 9, 1))
        want = float(FR.log_loss(f["pred"], label))
    print("B=%d loss %.7f ref %.7f" % (B, float(loss), want))
    assert np.isfinite(float(loss))
    np.testing.assert_allclose(float(loss), want, rtol=1e-5)
    np.testing.assert_allclose(pred.cpu().numpy(), f["pred"].numpy(), rtol=1e-5, atol=1e-6)
    moved = (m.embedding.cpu().numpy() != sd["fefm.embedding.weight"]).any(axis=1)
    assert moved[1:].mean() > 0.99 and not moved[0]          # L2 + non-lazy Adam: every row but the padding row moves
    del m


@pytest.mark.parametrize("lazy", [True, False])
def test_deepfefm_trainer_loops_gpu(engine_lib, tmp_path, lazy):
    import test_deepfefm
    test_deepfefm.run_trainer_loops(tmp_path, "cuda", None, lazy)
