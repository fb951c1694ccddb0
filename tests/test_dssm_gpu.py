"""DSSM on the GPU: the entry points of csrc/dssm_ops.hip and the layer (paddlerec_amd/dssm.py) on both routes against
tests/dssm_ref.py in float64, under the tolerance of tests/dssm_checks.py (8 x the float32 restatement's own error, floor 1e-6;
dq / dd row by row; parameters and moments after Adam by helpers.assert_adam_weights_close and the 1e-5-of-scale bar).

Sparse layer shapes (rows R, inputs T, outputs N; ld: the padding of every leading dimension):
  a  R 70, T 37, N 5 (one float per lane), 0 to 9 entries a row, values of either sign, a row without entries, a column no row holds
  b  R 1, T 1, N 128: one entry
  c  R 70, T 100, N 300 (wider than 256: two passes of a wave), a row of 65 entries (past one wave), every ld padded by 4
  d  R 300, T 37, N 128: column 5 in EVERY row (300 entries: each of the 8 waves sums 38), column 7 in none
  e  N 128 with ld N + 1: the float-per-lane path on a width the float4 path would take
Every backward runs over a NaN-poisoned dW: an untouched column must come out exactly zero, the padding must keep its poison."""
import ast
import os

import numpy as np
import pytest
import torch

import dssm_checks as K
import dssm_ref as R
from paddlerec_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def padded(a, pad, fill=np.nan):
    """A [rows, n] device view of a buffer whose rows are n + pad floats apart, the padding holding `fill`."""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf, buf[:, :a.shape[1]]


def make_csr(rng, Rr, T, special=None, max_per_row=9):
    """Random multi-hot rows: 0 to max_per_row ascending columns, values of either sign and not 1.0; special(r) -> the columns
    of row r or None."""
    cols, vals, lod = [], [], [0]
    for r in range(Rr):
        c = special(r) if special else None
        if c is None:
            c = np.sort(rng.choice(T, int(rng.integers(0, min(max_per_row, T) + 1)), replace=False))
        cols += list(c)
        vals += list(rng.choice([1.0, 1.0, -0.5, 2.25], len(c)) * rng.uniform(0.5, 1.5, len(c)))
        lod.append(len(cols))
    return np.asarray(cols, np.int64), np.asarray(vals, np.float32), np.asarray(lod, np.int64)


def sparse_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "a":
        Rr, T, N, pad = 70, 37, 5, 0
        sp = lambda r: np.asarray([], np.int64) if r == 3 else None
        csr = make_csr(rng, Rr, T - 1, sp)                                   # column 36: in no row
    elif name == "b":
        Rr, T, N, pad = 1, 1, 128, 0
        csr = np.asarray([0], np.int64), np.asarray([-1.5], np.float32), np.asarray([0, 1], np.int64)
    elif name == "c":
        Rr, T, N, pad = 70, 100, 300, 4
        csr = make_csr(rng, Rr, T, lambda r: np.sort(rng.choice(T, 65, replace=False)) if r == 3 else None)
    elif name == "d":
        Rr, T, N, pad = 300, 37, 128, 0

        def sp(r):
            c = rng.choice([x for x in range(T) if x not in (5, 7)], int(rng.integers(0, 5)), replace=False)
            return np.sort(np.append(c, 5))
        csr = make_csr(rng, Rr, T, sp)
    else:
        Rr, T, N, pad = 70, 37, 128, 1
        csr = make_csr(rng, Rr, T)
    W, b, dY = rng.standard_normal((T, N)), rng.standard_normal(N), rng.standard_normal((Rr, N))
    return Rr, T, N, pad, csr, W.astype(np.float32), b.astype(np.float32), dY.astype(np.float32)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list("abcde"))
def test_sparse_linear_fwd_against_float64(name, relu):
    from paddlerec_amd import ops
    Rr, T, N, pad, (cols, vals, lod), W, b, _ = sparse_case(name)
    ref = {}
    for dt in (np.float64, np.float32):
        y = R.csr_dense(cols, vals, lod, T, dt) @ W.astype(dt) + b.astype(dt)
        ref[dt] = np.maximum(y, 0) if relu else y
    _, Wv = padded(W, pad)
    ybuf, yv = padded(np.zeros((Rr, N)), pad)
    status = ops.new_status(DEV)
    out = ops.dssm_sparse_linear_fwd(dev(cols), dev(vals), dev(lod), Wv, dev(b), relu=relu, status=status, out=yv)
    assert out is yv and int(status.item()) == 0
    K.check_tensor("sparse fwd", "%s relu=%d" % (name, relu), yv.cpu().numpy(), ref[np.float64], ref[np.float32])
    assert pad == 0 or bool(torch.isnan(ybuf[:, N:]).all())                  # the padding is never written
    empty = np.flatnonzero(np.diff(lod) == 0)
    if name == "a":
        assert 3 in empty
    for r in empty:                                                          # a row without entries: act(bias), exactly
        assert np.array_equal(yv[r].cpu().numpy(), np.maximum(b, 0) if relu else b)


@pytest.mark.parametrize("name", list("abcde"))
def test_sparse_linear_bwd_against_float64(name):
    from paddlerec_amd import ops
    Rr, T, N, pad, (cols, vals, lod), _, _, dY = sparse_case(name)
    ref = {dt: R.csr_dense(cols, vals, lod, T, dt).T @ dY.astype(dt) for dt in (np.float64, np.float32)}
    if name == "d":
        assert np.bincount(cols, minlength=T)[5] == 300 and np.bincount(cols, minlength=T)[7] == 0
    if name == "c":
        assert np.diff(lod).max() == 65
    c, v, l = dev(cols), dev(vals), dev(lod)
    row_of = ops.dssm_lod_rows(l, len(cols))
    assert np.array_equal(row_of[:len(cols)].cpu().numpy(), np.repeat(np.arange(Rr), np.diff(lod)))
    groups, status = ops.ids_group(c, T, None, ops.Workspace(DEV))
    from paddlerec_amd.reader import dssm_group
    sp, uq, seg, nu = dssm_group(cols, T)                                    # the reader's grouping IS the device's
    U = int(nu[0])
    assert groups.n_uniq[:2].tolist() == nu[:2].tolist() and np.array_equal(groups.sorted_pos[:len(cols)].cpu().numpy(), sp[:len(cols)])
    assert np.array_equal(groups.uniq_rows[:U].cpu().numpy(), uq[:U]) and np.array_equal(groups.seg_offset[:U + 1].cpu().numpy(), seg[:U + 1])
    _, dyv = padded(dY, pad)
    wbuf, wv = padded(np.full((T, N), np.nan), pad)                          # poisoned: no memset precedes the kernel
    ops.dssm_sparse_linear_bwd(v, row_of, groups, dyv, wv)
    got = wv.cpu().numpy()
    assert int(status.item()) == 0 and np.isfinite(got).all()
    K.check_tensor("sparse bwd", name, got, ref[np.float64], ref[np.float32])
    untouched = np.flatnonzero(np.bincount(cols, minlength=T) == 0)
    assert name not in "ad" or len(untouched) > 0
    assert not got[untouched].any()                                          # exactly zero
    assert pad == 0 or bool(torch.isnan(wbuf[:, N:]).all())
    again, _ = padded(np.full((T, N), np.nan), pad)
    ops.dssm_sparse_linear_bwd(v, row_of, groups, dyv, again[:, :N])
    assert torch.equal(again[:, :N], wv)                                     # a rerun is bit-identical


def test_sparse_linear_bwd_without_any_entry_writes_zeros():
    from paddlerec_amd import ops
    _, wv = padded(np.full((37, 128), np.nan), 0)
    dY = dev(np.ones((4, 128), np.float32))
    ops.dssm_sparse_linear_bwd(torch.empty(0, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV), ops.IdGroups(0, DEV), dY, wv)
    assert not wv.any()


def test_an_out_of_range_column_is_flagged_and_skipped():
    from paddlerec_amd import ops
    rng = np.random.default_rng(9)
    T, N = 37, 128
    cols, vals, lod = make_csr(rng, 70, T, lambda r: np.asarray([2, 11, 30]) if r == 4 else None)
    bad = cols.copy()
    j = int(lod[4]) + 1
    bad[j] = T                                                               # one column past the table
    keep = np.ones(len(cols), bool)
    keep[j] = False
    W, b, dY = (rng.standard_normal(s).astype(np.float32) for s in ((T, N), (N,), (70, N)))
    # the reference: the same rows without that entry
    lod2 = lod.copy()
    lod2[5:] -= 1
    x64 = R.csr_dense(cols[keep], vals[keep], lod2, T)
    x32 = x64.astype(np.float32)
    status = ops.new_status(DEV)
    y = ops.dssm_sparse_linear_fwd(dev(bad), dev(vals), dev(lod), dev(W), dev(b), status=status)
    assert int(status.item()) & _lib.REC_FLAG_INDEX_OOB
    K.check_tensor("oob", "fwd", y.cpu().numpy(), x64 @ W.astype(np.float64) + b, x32 @ W + b)
    groups, gstatus = ops.ids_group(dev(bad), T, None, ops.Workspace(DEV))
    assert int(gstatus.item()) & _lib.REC_FLAG_INDEX_OOB
    _, wv = padded(np.full((T, N), np.nan), 0)
    ops.dssm_sparse_linear_bwd(dev(vals), ops.dssm_lod_rows(dev(lod), len(bad)), groups, dev(dY), wv)
    K.check_tensor("oob", "bwd", wv.cpu().numpy(), x64.T @ dY.astype(np.float64), x32.T @ dY)
    neg = bad.copy()
    neg[j] = -1
    status.zero_()
    y2 = ops.dssm_sparse_linear_fwd(dev(neg), dev(vals), dev(lod), dev(W), dev(b), status=status)
    assert int(status.item()) & _lib.REC_FLAG_INDEX_OOB and torch.equal(y, y2)


def test_lod_rows():
    from paddlerec_amd import ops
    for lod in ([0, 1], [0, 0, 3, 3, 70, 71], list(range(0, 600, 2))):
        lod = np.asarray(lod, np.int64)
        got = ops.dssm_lod_rows(dev(lod), int(lod[-1]))
        assert got.dtype == torch.int32
        assert np.array_equal(got[:lod[-1]].cpu().numpy(), np.repeat(np.arange(len(lod) - 1), np.diff(lod)))


# (B, neg, N, slice_end, relu mask folded, zero rows, padding of every leading dimension)
HEAD = [(1, 0, 5, 1, False, False, 0), (6, 1, 5, 4, True, False, 0), (6, 4, 128, 6, False, True, 0), (6, 4, 128, 4, True, True, 0),
        (70, 1, 128, 100, True, False, 0), (70, 4, 5, 8, False, True, 0), (70, 0, 128, 70, False, False, 0),
        (6, 1, 128, 9, False, False, 3), (70, 4, 128, 69, True, False, 4)]


@pytest.mark.parametrize("B,neg,N,slice_end,relu,zeros,pad", HEAD)
def test_head_step_against_float64(B, neg, N, slice_end, relu, zeros, pad):
    from paddlerec_amd import ops
    rng = np.random.default_rng(B * 1000 + neg * 100 + N + slice_end)
    q, d = rng.standard_normal((B, N)).astype(np.float32), rng.standard_normal(((1 + neg) * B, N)).astype(np.float32)
    if relu:
        q, d = np.maximum(q, 0), np.maximum(d, 0)
    if zeros:                                                                # the clamped branch, in value and in gradient
        q[1 % B] = 0
        d[(neg * B + 2) % len(d)] = 0
    ref = {}
    for dt in (np.float64, np.float32):
        h = R.head(q, d, slice_end, dt)
        if relu:
            h["dq"], h["dd"] = h["dq"] * (q > 0), h["dd"] * (d > 0)
        ref[dt] = h
    r64, r32 = ref[np.float64], ref[np.float32]
    M = min(B, slice_end)
    if zeros and not relu and 1 % B < M:                                     # the other vector / eps: eight orders above its neighbours
        assert np.abs(r64["dq"][1 % B]).max() > 1e5 * np.abs(r64["dq"][0]).max() > 0
    _, qv = padded(q, pad)
    _, dv = padded(d, pad)
    out = None
    if pad:
        f32 = dict(dtype=torch.float32, device=DEV)
        out = dict(cos=torch.empty(B, 1 + neg, **f32), hit_prob=torch.empty(B, **f32), loss_terms=torch.empty(B, **f32),
                   loss=torch.zeros(1, **f32), dq=padded(np.full((B, N), np.nan), pad)[1],
                   dd=padded(np.full(((1 + neg) * B, N), np.nan), pad)[1])
    got = ops.dssm_head_step(qv, dv, slice_end, relu_mask=relu, out=out)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert all(np.isfinite(v).all() for v in g.values())
    what = "head B%d neg%d N%d" % (B, neg, N)
    K.check_tensor(what, "cos", g["cos"], r64["cos"], r32["cos"])
    K.check_tensor(what, "hit_prob", g["hit_prob"], r64["hit_prob"], r32["hit_prob"])
    if neg:
        K.check_tensor(what, "loss_terms", g["loss_terms"], r64["terms"], r32["terms"])
        K.check_tensor(what, "loss", g["loss"], r64["loss"], r32["loss"])
    else:                                                                    # no negatives: the softmax is 1, everything else 0
        assert (g["hit_prob"] == 1).all() and not g["loss_terms"].any() and g["loss"][0] == 0
        assert not g["dq"].any() and not g["dd"].any()
    K.check_rows(what, "dq", g["dq"], r64["dq"], r32["dq"])
    K.check_rows(what, "dd", g["dd"], r64["dd"], r32["dd"])
    assert not g["dq"][M:].any() and not g["dd"].reshape(1 + neg, B, N)[:, M:].any()
    if zeros:
        assert g["cos"][1 % B, 0] == 0
    again = ops.dssm_head_step(qv, dv, slice_end, relu_mask=relu)
    assert all(torch.equal(again[k], got[k]) for k in got)                   # a rerun is bit-identical


@pytest.mark.parametrize("B,N,pad", [(6, 5, 0), (70, 128, 0), (70, 128, 2), (1, 300, 0)])
def test_cos_against_float64(B, N, pad):
    from paddlerec_amd import ops
    rng = np.random.default_rng(B + N)
    q, d = rng.standard_normal((B, N)).astype(np.float32), rng.standard_normal((B, N)).astype(np.float32)
    if B > 2:
        q[1], d[2] = 0, 0
    got = ops.dssm_cos(padded(q, pad)[1], padded(d, pad)[1]).cpu().numpy()
    K.check_tensor("cos", "B%d N%d" % (B, N), got, R.cosine(q.astype(np.float64), d.astype(np.float64))[0], R.cosine(q, d, np.float32)[0])
    if B > 2:
        assert got[1] == 0 and got[2] == 0
    if pad == 0:                                                             # the head's positive column is the same arithmetic
        head = ops.dssm_head_step(dev(q), dev(d), B)
        assert np.array_equal(head["cos"][:, 0].cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ the layer
ROUTES = ("sparse", "general")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", K.GOLDENS)
def test_layer_reproduces_the_golden(name, route):
    G = K.gold(name)
    m = K.layer_of(G, DEV)
    K.check_layer(G, m, route, "%s %s" % (name[:-4], route))
    assert m._last["sparse"] == (route == "sparse") and m._last["docs"] == 3
    K.check_infer(G, m, route, "%s %s" % (name[:-4], route))


def _run(G, route, rows=None):
    m = K.layer_of(G, DEV)
    m.set_dict(G["p"])
    out = []
    for s in range(G["steps"]):
        loss = m.train_step(K.feeds_of(G, "*_%d" % s, route, DEV, rows), lr=G["lr"])
        cos, hit = m.last_outputs()
        out.append(dict(loss=loss.clone(), cos=cos.clone(), hit_prob=hit.clone(), g=m.last_gradients(),
                        n={k: v.clone() for k, v in m.state_dict().items()}))
    return out


@pytest.mark.parametrize("name", K.GOLDENS)
def test_routes_agree_and_reruns_are_bit_identical(name):
    G = K.gold(name)
    runs = {r: (_run(G, r), _run(G, r)) for r in ROUTES}
    for r, (a, b) in runs.items():
        for s in range(G["steps"]):
            assert all(torch.equal(a[s][k], b[s][k]) for k in ("loss", "cos", "hit_prob")), (r, s)
            assert all(torch.equal(a[s][w][k], b[s][w][k]) for w in ("g", "n") for k in a[s][w]), (r, s)
    s = 0                                                                    # step 0 starts from one state on both routes
    a, b = runs["sparse"][0][s], runs["general"][0][s]
    r64, r32 = G["r64"][s], G["r32"][s]
    for k in ("loss", "cos", "hit_prob"):
        assert R.relerr(a[k].cpu().numpy().reshape(r64[k].shape), b[k].cpu().numpy().reshape(r64[k].shape)) <= K.bound_of(r32[k], r64[k]), k
    for k in r64["g"]:
        assert R.relerr(a["g"][k].cpu().numpy(), b["g"][k].cpu().numpy()) <= K.bound_of(r32["g"][k], r64["g"][k]), k


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", K.GOLDENS)
def test_rows_beyond_slice_end_add_nothing_to_the_gradients(name, route):
    """B 6, slice_end 4: the gradients of the whole batch are those of the batch cut to its first four rows."""
    G = K.gold(name)
    g, T = G["g"], G["trigram_d"]
    full, cut = _run(G, route)[0], _run(G, route, rows=G["slice_end"])[0]
    q, d = K.dense_of(g, "q_0", T), K.dense_of(g, "d_0", T).reshape(3, 6, T)[:, :4].reshape(12, T)
    ref = {dt: R.loss_and_grads(G["p"], G["relu"], q[:4].astype(dt), d.astype(dt), 4, dt) for dt in (np.float64, np.float32)}
    assert tuple(cut["cos"].shape) == (4, 3) and tuple(full["cos"].shape) == (6, 3)
    for run, what in ((full, "full batch"), (cut, "cut batch")):
        K.check_tensor(what, "loss", run["loss"].cpu().numpy(), ref[np.float64]["loss"], ref[np.float32]["loss"])
        for k in ref[np.float64]["g"]:
            K.check_tensor(what, "g_" + k, run["g"][k].cpu().numpy(), ref[np.float64]["g"][k], ref[np.float32]["g"][k])


def test_the_environment_switch_sends_csr_feeds_down_the_general_route(monkeypatch):
    G = K.gold("dssm_relu.npz")
    monkeypatch.setenv("REC_DSSM_SPARSE", "0")
    m = K.layer_of(G, DEV)
    K.check_layer(G, m, "sparse", "csr densified")
    assert m._last["sparse"] is False
    K.check_infer(G, m, "sparse", "csr densified")


def test_feeds_are_validated_and_what_the_reader_supplies_is_used():
    """A feed may carry row_of, and the entries grouped by column (reader.dssm_group: the device grouping's own format, made on
    the host): the step then launches neither rec_dssm_lod_rows nor the sort, and its bits do not change."""
    from paddlerec_amd.reader import dssm_csr, dssm_group
    G = K.gold("dssm_lin.npz")
    m = K.layer_of(G, DEV)
    m.set_dict(G["p"])
    q, d = K.feeds_of(G, "*_0", "sparse", DEV)
    with pytest.raises(ValueError, match="multiple"):
        m.train_step([q, (d[0], d[1], d[2][:-1])])
    with pytest.raises(ValueError, match="int64"):
        m.train_step([(q[0].int(), q[1], q[2]), d])
    with pytest.raises(ValueError, match="query and the positive"):
        m.train_step([q])
    a = m.train_step([q, d], lr=G["lr"]).clone()
    ga = m.last_gradients()
    m2 = K.layer_of(G, DEV)
    m2.set_dict(G["p"])
    T = G["trigram_d"]
    with_rows = [tuple(dev(x) for x in dssm_csr(list(K.dense_of(G["g"], p, T, np.float32)))) for p in ("q_0", "d_0")]
    assert all(len(x) == 4 and x[3].dtype == torch.int32 for x in with_rows)
    b = m2.train_step(with_rows, lr=G["lr"])
    assert torch.equal(a, b) and all(torch.equal(ga[k], v) for k, v in m2.last_gradients().items())
    m3 = K.layer_of(G, DEV)
    m3.set_dict(G["p"])
    grouped = [x + tuple(dev(t) for t in dssm_group(x[0].cpu().numpy(), T)) for x in with_rows]
    calls = []
    m3._grouped = lambda *a, **k: calls.append(a)                            # the device sort must not be asked for
    c = m3.train_step(grouped, lr=G["lr"])
    assert not calls and torch.equal(a, c) and all(torch.equal(ga[k], v) for k, v in m3.last_gradients().items())
    assert all(torch.equal(v, m3.state_dict()[k]) for k, v in m.state_dict().items())
    with pytest.raises(_lib.RecError, match="seg_offset"):
        m3.train_step([grouped[0][:6] + (grouped[0][6][:2], grouped[0][7]), grouped[1]], lr=G["lr"])


def test_trainer_trains_saves_and_infers_on_the_sample(tmp_path, capsys):
    """--model by the directory name `dssm`: one epoch (two batches of five) on the first ten lines of the reference's train
    sample at the shipped sizes, a checkpoint, then --infer prints query_doc_sim — the mean the reference restatement gets from
    the saved parameters."""
    from conftest import GOLDEN
    from paddlerec_amd import checkpoint, trainer
    from paddlerec_amd.dssm import DSSMLayer
    from paddlerec_amd.reader import dssm_parse
    root = tmp_path / "dssm"
    for d, src in (("train", "dssm_sample_train.txt"), ("test", "dssm_sample_test.txt")):
        (root / "data" / d).mkdir(parents=True)
        with open(os.path.join(GOLDEN, src)) as f:
            (root / "data" / d / "sample.txt").write_text(f.read())
    (root / "config.yaml").write_text(
        "runner:\n  train_data_dir: data/train\n  test_data_dir: data/test\n  train_batch_size: 5\n  infer_batch_size: 3\n"
        "  epochs: 1\n  print_interval: 1\n  model_save_path: %s\n  infer_load_path: %s\n  infer_start_epoch: 0\n"
        "  infer_end_epoch: 1\nhyper_parameters:\n  optimizer:\n    class: adam\n    learning_rate: 0.001\n  trigram_d: 2900\n"
        "  neg_num: 1\n  slice_end: 8\n  fc_sizes: [300, 300, 128]\n  fc_acts: ['relu', 'relu', 'relu']\n"
        % (tmp_path / "out", tmp_path / "out"))
    trainer.main(["-m", str(root / "config.yaml"), "--device", DEV])
    (train,) = [ast.literal_eval(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert train["batches"] == 2 and train["samples"] == 10 and np.isfinite(train["loss"]) and 0 < train["loss"] < 2
    trainer.main(["-m", str(root / "config.yaml"), "--infer", "--device", DEV])
    (res,) = [ast.literal_eval(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert res["batches"] == 2 and res["samples"] == 4
    m = DSSMLayer(2900, 1, 8, [300, 300, 128], ["relu"] * 3, device=DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    checkpoint.load_model(os.path.join(str(tmp_path / "out"), "0"), m, load_optimizer=False)
    assert all(not torch.equal(before[k], v) for k, v in m.state_dict().items())
    lines = dssm_parse([str(root / "data" / "test" / "sample.txt")], 2)
    p = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    want = R.forward_infer(p, [True] * 3, np.stack([l[0] for l in lines]), np.stack([l[1] for l in lines]))
    assert -1 <= res["query_doc_sim"] <= 1 and abs(res["query_doc_sim"] - float(want.mean())) < 1e-5
