"""ENSFM on the GPU (csrc/ensfm_ops.hip, paddlerec_amd/ensfm.py) against tests/ensfm_ref.py in float64.

Tolerance, the project's rule (tests/ensfm_checks.py), for every tensor, the Adagrad accumulators included:
max|got - ref64| / max|ref64| <= 8 x the same error of ensfm_ref.py in float32 on the same inputs, floor 1e-6; parameters after
Adagrad: at least 0.98 of the elements within 1e-5 of the tensor's scale and none further than steps * lr away.

Capped grids: rec_ensfm_tower_bwd gives a block a slice of the rows once n > 4 * REC_ENSFM_MAX_PARTIALS, rec_ensfm_gram a
run of tiles once n > 64 * REC_ENSFM_GRAM_MAX_BLOCKS; both are driven past that here.  Every other kernel's grid grows
with its shape."""
import os

import numpy as np
import pytest
import torch

import ensfm_checks as K
import ensfm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _both(fn):
    """fn(dtype) evaluated in float64 and float32."""
    return fn(np.float64), fn(np.float32)


def _tower_ref(ids, table, bias_table, Hs, bias, item, dtype):
    ok, okb = (ids >= 0) & (ids < len(table)), (ids >= 0) & (ids < len(bias_table))
    e = np.asarray(table, dtype)[np.where(ok, ids, 0)] * ok[:, :, None]
    b = (np.asarray(bias_table, dtype).reshape(-1)[np.where(okb, ids, 0)] * okb).sum(1, keepdims=True)
    s = e.sum(1)
    cross = dtype(0.5) * (s ** 2 - (e ** 2).sum(1))
    score = cross @ np.asarray(Hs, dtype).reshape(-1, 1) + b + (dtype(bias) if bias is not None else dtype(0))
    one = np.ones((len(ids), 1), dtype)
    return (np.concatenate([s, one, score], 1) if item else np.concatenate([s, score, one], 1)), e, s, cross, ok


def _tower_bwd_ref(ids, table, bias_table, Hs, d_out, item, dtype):
    D = table.shape[1]
    _, e, s, cross, ok = _tower_ref(ids, table, bias_table, Hs, None, item, dtype)
    d_out = np.asarray(d_out, dtype)
    ds, dsc = d_out[:, :D], d_out[:, D + 1:D + 2] if item else d_out[:, D:D + 1]
    rows = (ds[:, None, :] + (dsc * np.asarray(Hs, dtype).reshape(1, -1))[:, None, :] * (s[:, None, :] - e)) * ok[:, :, None]
    return rows.reshape(-1, D), dsc.reshape(-1), (cross * dsc).sum(0), dsc.sum().reshape(1)


@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("D", [1, 8, 64, 65])
def test_towers_forward_and_backward(F, D):
    from paddlerec_amd import ops
    rng = np.random.default_rng(100 * F + D)
    n, rows, brows = 5, 9, 8
    # positive table entries and score gradients: dH_s and d bias are then sums of one sign, so the scalar cases (D 1) are
    # held to a bound relative to a sum that cannot cancel
    table, bias_table = 0.1 + 0.3 * np.abs(rng.standard_normal((rows, D))), 0.3 * rng.standard_normal((brows, 1))
    Hs, bias = 0.3 * rng.standard_normal((D, 1)), 0.3 * rng.standard_normal(1)
    ids = rng.integers(0, brows, (n, F))
    if F > 1:
        ids[1, 1] = ids[1, 0]                                 # the same id twice in a row: a non-zero cross term for the pair
    d_out = rng.standard_normal((n, D + 2))
    d_out[:, D:] = 0.5 + np.abs(d_out[:, D:])
    f32 = lambda a: _t(np.asarray(a, np.float32))
    tb, bt, hs, bs = f32(table), f32(bias_table), f32(Hs), f32(bias)
    f = lambda a: np.asarray(a, np.float32)                   # the references start from the float32 inputs
    for item in (False, True):
        st = ops.new_status(DEV)
        out = ops.ensfm_tower_fwd(_t(ids), tb, bt, hs, None if item else bs, item_layout=item, status=st)
        r64, r32 = _both(lambda dt: _tower_ref(ids, f(table), f(bias_table), f(Hs), None if item else f(bias)[0], item, dt)[0])
        K.check_tensor("tower", "fwd F %d D %d item %d" % (F, D, item), out.cpu().numpy(), r64, r32)
        assert int(st.item()) == 0
        const = out[:, D] if item else out[:, D + 1]
        assert (const == 1).all()
        dHs, db = torch.full((D,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
        rows_g, dsc = ops.ensfm_tower_bwd(_t(ids), tb, hs, f32(d_out), dHs, db, item_layout=item)
        b64, b32 = _both(lambda dt: _tower_bwd_ref(ids, f(table), f(bias_table), f(Hs), f(d_out), item, dt))
        for name, got, i in (("rows", rows_g, 0), ("dscore", dsc[:n], 1), ("dH_s", dHs, 2), ("dbias", db, 3)):
            K.check_tensor("tower", "bwd %s F %d D %d item %d" % (name, F, D, item), got.cpu().numpy(), b64[i], b32[i])
        # accumulate adds to what dH_s / dbias hold, in place
        ops.ensfm_tower_bwd(_t(ids), tb, hs, f32(d_out), dHs, None, item_layout=item, accumulate=True)
        K.check_tensor("tower", "bwd accumulate", dHs.cpu().numpy(), 2 * b64[2], 2 * b32[2])
    # an id outside the table: the status bit is set, it contributes zero, nothing else changes
    bad = ids.copy()
    bad[2, F - 1] = rows + 3
    bad[3, 0] = brows                                          # inside the table, outside the (one row shorter) bias table
    st = ops.new_status(DEV)
    out = ops.ensfm_tower_fwd(_t(bad), tb, bt, hs, bs, status=st)
    from paddlerec_amd import _lib
    assert int(st.item()) & _lib.REC_FLAG_INDEX_OOB
    r64, r32 = _both(lambda dt: _tower_ref(bad, f(table), f(bias_table), f(Hs), f(bias)[0], False, dt)[0])
    K.check_tensor("tower", "fwd with a bad id", out.cpu().numpy(), r64, r32)
    good = ops.ensfm_tower_fwd(_t(ids), tb, bt, hs, bs)
    keep = [r for r in range(n) if r not in (2, 3)]
    assert torch.equal(out[keep], good[keep])
    rows_g, _ = ops.ensfm_tower_bwd(_t(bad), tb, hs, f32(d_out), torch.empty(D, device=DEV))
    b64, b32 = _both(lambda dt: _tower_bwd_ref(bad, f(table), f(bias_table), f(Hs), f(d_out), False, dt))
    K.check_tensor("tower", "bwd rows with a bad id", rows_g.cpu().numpy(), b64[0], b32[0])
    assert (rows_g[2 * F + F - 1] == 0).all()


def test_tower_backward_past_its_grid_cap():
    """n > 4 * REC_ENSFM_MAX_PARTIALS: a block owns 8 rows, the last block a short slice."""
    from paddlerec_amd import _lib, ops
    n, F, D = 4 * _lib.REC_ENSFM_MAX_PARTIALS + 5, 2, 3
    rng = np.random.default_rng(5)
    f = lambda a: np.asarray(a, np.float32)
    table, Hs, ids, d_out = f(0.1 + 0.3 * np.abs(rng.standard_normal((7, D)))), f(0.3 * rng.standard_normal((D, 1))), \
        rng.integers(0, 7, (n, F)), f(0.5 + np.abs(rng.standard_normal((n, D + 2))))
    dHs, db = torch.empty(D, device=DEV), torch.empty(1, device=DEV)
    rows_g, dsc = ops.ensfm_tower_bwd(_t(ids), _t(table), _t(Hs), _t(d_out), dHs, db)
    b64, b32 = _both(lambda dt: _tower_bwd_ref(ids, table, np.zeros((7, 1), np.float32), Hs, d_out, False, dt))
    for name, got, i in (("rows", rows_g, 0), ("dscore", dsc[:n], 1), ("dH_s", dHs, 2), ("dbias", db, 3)):
        K.check_tensor("tower cap", name, got.cpu().numpy(), b64[i], b32[i])


@pytest.mark.parametrize("C", [3, 10, 66])
def test_gram(C):
    from paddlerec_amd import _lib, ops
    rng = np.random.default_rng(C)
    sizes = [1, 63, 64, 65, 1000] + ([64 * _lib.REC_ENSFM_GRAM_MAX_BLOCKS + 65] if C == 3 else [])      # the last: past the grid cap
    for n in sizes:
        X = np.asarray(rng.standard_normal((n, C + 1)), np.float32)
        view = _t(X)[:, :C]                                   # a row stride above the width
        G = ops.ensfm_gram(view)
        r64, r32 = _both(lambda dt: np.asarray(X[:, :C], dt).T @ np.asarray(X[:, :C], dt))
        K.check_tensor("gram", "n %d C %d" % (n, C), G.cpu().numpy(), r64, r32)
        assert torch.equal(G, ops.ensfm_gram(view))           # bit-identical rerun


def _positives_ref(ur, p, q, Hi, w, dtype):
    """g, pos_r, dP, dQ, loss, dH_i of the positives and the whole-data term, in the materialising formulation."""
    I = len(q) - 1
    p, q, w = np.asarray(p, dtype), np.asarray(q, dtype), dtype(w)
    h = np.concatenate([np.asarray(Hi, dtype).reshape(-1, 1), np.ones((2, 1), dtype)])
    c = dict(p_emb=p, q_emb=q, h=h)
    mask = ((ur >= 0) & (ur < I)).astype(dtype)
    c["pos_item"] = q[np.where(mask > 0, ur, 0)] * mask[:, :, None]
    c["pos3"] = p[:, None, :] * c["pos_item"]
    c["pos_r"] = (c["pos3"] @ h)[:, :, 0]
    loss = R.loss_of(c, w, dtype)
    g = (dtype(2) * (dtype(1) - w) * c["pos_r"] - dtype(2)) * mask
    d_pos3 = g[:, :, None] * h[None, None, :, 0]
    dP = (d_pos3 * c["pos_item"]).sum(1) + p @ (dtype(2) * w * c["qq"] * c["hh"])
    dQ = q @ (dtype(2) * w * c["pp"] * c["hh"])
    np.add.at(dQ, np.where(mask > 0, ur, 0).reshape(-1), (d_pos3 * p[:, None, :]).reshape(-1, q.shape[1]))
    dh = (g[:, :, None] * c["pos3"]).sum((0, 1))[:, None] + dtype(2) * w * (c["qq"] * c["pp"]) @ h
    return dict(g=g, pos_r=c["pos_r"], dP=dP, dQ=dQ, loss=np.asarray(loss).reshape(1), dH_i=dh[:len(h) - 2, 0])


def _run_positives(ur, p, q, Hi, w, st=None):
    from paddlerec_amd import ops
    I = len(q) - 1
    tp, tq, th, tur = _t(p), _t(q), _t(Hi), _t(ur)
    Gp, Gq = ops.ensfm_gram(tp), ops.ensfm_gram(tq)
    g, dP, lp, dhp, pos_r = ops.ensfm_pos_user(tur, tp, tq, th, Gq, w, status=st, want_pos_r=True)
    groups, gst = ops.ids_group(tur.view(-1), I + 1, I, ops.Workspace(DEV))
    dQ = ops.ensfm_pos_item(groups, g, tp, tq, th, Gp, w)
    loss, dH = ops.ensfm_loss(Gp, Gq, th, lp, dhp, w, len(p))
    return dict(g=g, pos_r=pos_r, dP=dP, dQ=dQ, loss=loss, dH_i=dH), groups


def test_positives_corner_users():
    """B 3, P 7, I 6: an all-padding list, a full list with one item twice, item 0 in a list."""
    rng = np.random.default_rng(8)
    B, P, I, D, w = 3, 7, 6, 5, 0.3
    ur = np.full((B, P), I, np.int64)
    ur[1] = (3, 1, 4, 1, 5, 2, 0)
    ur[2, :3] = (0, 5, 3)
    f = lambda a: np.asarray(a, np.float32)
    p, q, Hi = (f(0.1 + 0.5 * np.abs(rng.standard_normal(sh))) for sh in ((B, D + 2), (I + 1, D + 2), (D,)))   # one sign: the loss cannot cancel
    got, _ = _run_positives(ur, p, q, Hi, w)
    r64, r32 = _both(lambda dt: _positives_ref(ur, p, q, Hi, w, dt))
    for k in r64:
        K.check_tensor("positives", k, got[k].cpu().numpy(), r64[k], r32[k])
    assert (got["g"][0] == 0).all() and (got["pos_r"][0] == 0).all()                 # padded pairs contribute nothing
    # the padding row and a row without positives get exactly the Gram term
    from paddlerec_amd import ops
    only_gram = ops.ensfm_pos_item(ops.ids_group(_t(np.full((B, P), I, np.int64)).view(-1), I + 1, I, ops.Workspace(DEV))[0],
                                   torch.zeros(B, P, device=DEV), _t(p), _t(q), _t(Hi), ops.ensfm_gram(_t(p)), w)
    assert torch.equal(got["dQ"][I], only_gram[I])
    # an id outside [0, I]: flagged, counted as padding
    bad = ur.copy()
    bad[1, 2] = I + 4
    st = ops.new_status(DEV)
    got_bad, _ = _run_positives(bad, p, q, Hi, w, st)
    from paddlerec_amd import _lib
    assert int(st.item()) & _lib.REC_FLAG_INDEX_OOB
    r64, r32 = _both(lambda dt: _positives_ref(bad, p, q, Hi, w, dt))
    for k in ("g", "pos_r", "dP", "loss"):
        K.check_tensor("positives", k + " with a bad id", got_bad[k].cpu().numpy(), r64[k], r32[k])


def test_positives_one_item_in_every_list():
    """B 300, P 3, I 4: item 2 is in every list, a segment of 300 >= REC_SEG_LONG for the item-owned pass."""
    from paddlerec_amd import _lib
    rng = np.random.default_rng(9)
    B, P, I, D, w = 300, 3, 4, 6, 0.5
    ur = np.full((B, P), I, np.int64)
    ur[:, 1] = 2
    ur[::3, 0] = rng.integers(0, 2, len(ur[::3]))
    ur[1::5, 2] = 3
    f = lambda a: np.asarray(a, np.float32)
    p, q, Hi = (f(0.1 + 0.5 * np.abs(rng.standard_normal(sh))) for sh in ((B, D + 2), (I + 1, D + 2), (D,)))   # one sign: the loss cannot cancel
    got, groups = _run_positives(ur, p, q, Hi, w)
    _, uniq, seg = groups.host()
    assert int(np.diff(seg)[list(uniq).index(2)]) == B >= _lib.REC_SEG_LONG and int(groups.n_uniq[2].item()) == 1
    r64, r32 = _both(lambda dt: _positives_ref(ur, p, q, Hi, w, dt))
    for k in r64:
        K.check_tensor("hot item", k, got[k].cpu().numpy(), r64[k], r32[k])
    again, _ = _run_positives(ur, p, q, Hi, w)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_score():
    from paddlerec_amd import ops
    rng = np.random.default_rng(10)
    f = lambda a: np.asarray(a, np.float32)
    for B, rows, D in ((1, 1, 1), (17, 65, 8), (35, 130, 65)):
        p, q, Hi = f(rng.standard_normal((B, D + 2))), f(rng.standard_normal((rows, D + 2))), f(rng.standard_normal(D))
        pre = ops.ensfm_score(_t(p), _t(q), _t(Hi))
        ref = lambda dt: (np.asarray(p, dt) * np.concatenate([np.asarray(Hi, dt), np.ones(2, dt)])) @ np.asarray(q, dt).T
        r64, r32 = _both(ref)
        K.check_tensor("score", "B %d rows %d D %d" % (B, rows, D), pre.cpu().numpy(), r64, r32)


def test_layer_against_the_golden_both_steps_and_infer():
    G = K.gold()
    m = K.layer_of(G, DEV)
    K.check_layer(G, m, "gpu")
    K.check_infer(G, m, "gpu")


def _random_layer_and_batch(seed=3):
    from paddlerec_amd.ensfm import ENSFMLayer
    g = torch.Generator().manual_seed(seed)
    B, Fu, Fi, D, I, P = 37, 4, 2, 16, 50, 9
    m = ENSFMLayer(40, 30, D, device=DEV)
    for t in list(m.tables.values()) + [m.params["H_i"], m.params["H_s"], m.params["bias"]]:
        t.copy_((0.3 * torch.randn(t.shape, generator=g)).to(DEV))
    u = torch.randint(0, 20, (B, Fu), generator=g)            # rows 20..39 of the user tables stay untouched
    attr = torch.randint(0, 15, (I + 1, Fi), generator=g)     # rows 15.. of the item tables stay untouched
    attr[I] = attr[0]
    ur = torch.randint(0, I, (B, P), generator=g)
    ur[torch.rand(B, P, generator=g) < 0.4] = I
    return m, u.to(DEV), attr.to(DEV), ur.to(DEV)


def test_train_step_is_deterministic_and_leaves_untouched_rows_alone():
    runs = []
    for _ in range(2):
        m, u, attr, ur = _random_layer_and_batch()
        before = {k: v.clone() for k, v in m.state_dict().items()}
        acc0 = {k: v.clone() for k, v in m.acc.items()}
        loss = m.train_step(u, attr, ur, lr=0.05, negative_weight=0.5)
        grads = {k: v.clone() for k, v in m.last_gradients().items()}
        grads.update({"raw " + k: m._last[k].clone() for k in ("rows_u", "dsc_u", "rows_v", "dsc_v", "dP", "dQ", "g")})
        state = {k: v.clone() for k, v in m.state_dict().items()}
        state.update({"acc " + k: v.clone() for k, v in m._shown("m").items()})
        runs.append((loss.clone(), grads, state))
        assert int(m.status.item()) == 0 and torch.isfinite(loss).all()
        for name, ids in (("user_feature_emb.weight", u), ("user_bias.weight", u), ("all_item_feature_emb.weight", attr),
                          ("item_bias.weight", attr)):
            touched = torch.zeros(m.tables[name].shape[0], dtype=torch.bool, device=DEV)
            touched[ids.reshape(-1)] = True
            assert (~touched).any() and touched.any()
            assert torch.equal(m.tables[name][~touched], before[name][~touched]), name         # bit-unchanged
            assert torch.equal(m.acc[name][~touched], acc0[name][~touched]), name
            assert not torch.equal(m.tables[name][touched], before[name][touched]), name
    (l0, g0, p0), (l1, g1, p1) = runs
    assert torch.equal(l0, l1)
    assert [k for k in g0 if not torch.equal(g0[k], g1[k])] == [] and [k for k in p0 if not torch.equal(p0[k], p1[k])] == []


def test_trainer_trains_and_infers_on_the_sample(tmp_path):
    """--model ensfm end to end on the reference's 100-line sample: two epochs, checkpoints, then infer.py's HR@k."""
    from conftest import GOLDEN
    from paddlerec_amd import trainer
    d = tmp_path / "data"
    d.mkdir()
    for name in ("train", "test"):
        with open(os.path.join(GOLDEN, "ensfm_%s_sample.csv" % name)) as f:
            (d / (name + ".csv")).write_text(f.read())
    cfg = {"config_abs_dir": str(tmp_path), "runner.train_data_dir": str(d), "runner.test_data_dir": str(d),
           "runner.train_batch_size": 2, "runner.infer_batch_size": 32, "runner.epochs": 2, "runner.print_interval": 1,
           "runner.model_save_path": str(tmp_path / "out"), "runner.infer_load_path": str(tmp_path / "out"),
           "runner.infer_start_epoch": 1, "runner.infer_end_epoch": 2, "hyper_parameters.optimizer.class": "adagrad",
           "hyper_parameters.optimizer.learning_rate": 0.05, "hyper_parameters.num_users": 6069, "hyper_parameters.num_items": 3953,
           "hyper_parameters.mf_dim": 64, "hyper_parameters.negative_weight": 0.5}
    summaries, model = trainer.train(dict(cfg), "ensfm", DEV)
    assert [s["batches"] for s in summaries] == [1, 1] and all(np.isfinite(s["loss"]) for s in summaries)
    assert summaries[1]["loss"] != summaries[0]["loss"] and int(model.status.item()) == 0      # the step moved the parameters
    (res,) = trainer.infer(dict(cfg), "ensfm", DEV)
    assert res["batches"] == 3 and res["samples"] == 96                    # 100 test lines, drop_last
    assert all(0.0 <= res[k] <= 1.0 for k in ("HR@5", "HR@10", "HR@20"))


def test_trainer_path_groups_the_item_attributes_once(tmp_path):
    """EnsfmReader hands every batch a fresh VIEW of the one device-resident attribute tensor and create_feeds takes [0] of it:
    a new Python object per step over the same storage.  The item-side groupings must be made on the first train_forward only."""
    from conftest import GOLDEN
    from paddlerec_amd.ensfm import DygraphModel
    from paddlerec_amd.reader import EnsfmReader
    for name in ("train", "test"):
        with open(os.path.join(GOLDEN, "ensfm_%s_sample.csv" % name)) as f:
            (tmp_path / (name + ".csv")).write_text(f.read())
    rd = EnsfmReader(sorted(str(p) for p in tmp_path.iterdir()), 1, DEV, "train")
    cfg = {"hyper_parameters.num_users": 6069, "hyper_parameters.num_items": 3953, "hyper_parameters.mf_dim": 8}
    dm = DygraphModel()
    m = dm.create_model(cfg, DEV)
    batches = list(rd) + list(rd)                              # two users, two epochs: four steps
    assert len(batches) == 4 and batches[0][1] is not batches[1][1]
    feeds = [dm.create_feeds(b, DEV) for b in batches]
    assert feeds[0][1] is not feeds[1][1] and feeds[0][1].data_ptr() == feeds[1][1].data_ptr() == rd.item_attribute.data_ptr()
    assert feeds[0][0] is batches[0][0] and feeds[0][3].device.type == "cpu"       # passed through; item_bind_M stays on the host
    calls = []

    class Counting:
        def __getattr__(self, n):
            f = getattr(m_k, n)
            if n != "ids_group":
                return f
            return lambda ids, *a, **kw: (calls.append(ids.numel()), f(ids, *a, **kw))[1]
    m_k = m.k
    m.k = Counting()
    for b in batches:
        loss, _, _ = dm.train_forward(m, [], b, cfg)
    m.k = m_k
    assert torch.isfinite(loss).all() and int(m.status.item()) == 0
    n_attr = rd.item_attribute.numel()
    assert m.item_groupings_made == 1 and calls.count(n_attr) == 2, (m.item_groupings_made, calls)      # feature table + item_bias, once
    assert len(calls) == 2 + 2 * len(batches)                  # per step: the lists and the user ids only
    # a changed attribute tensor is grouped again
    rd.item_attribute[0, 0] = rd.item_attribute[1, 0]
    dm.train_forward(m, [], batches[0], cfg)
    assert m.item_groupings_made == 2
