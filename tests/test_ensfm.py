"""ENSFM without a GPU: the numpy restatement (tests/ensfm_ref.py, the reference's materialising formulation) against the
golden recorded from the reference's own net.py / dygraph_model.py (tools/make_golden_ensfm.py), the reader against what the
reference's movielens_reader.py yields, and infer.py's HR@k on a hand-made score matrix."""
import os

import numpy as np
import torch

import ensfm_checks as K
import ensfm_ref as R
from conftest import GOLDEN


def test_ref_float64_matches_the_golden_on_every_recorded_tensor():
    G = K.gold()
    assert G["steps"] == 2
    K.check_golden(G)
    # and the float32 restatement ALONE passes the post-step bound (what the tool chose the seed by)
    for s in range(G["steps"]):
        for k in R.PARAMS:
            K.assert_adagrad_weights_close(G["r32"][s]["n"][k], G["r64"][s]["n"][k], G["lr"], 1, err_msg=k)


def test_golden_holds_the_corner_cases():
    g = K.gold()["g"]
    I = g["attr"].shape[0] - 1
    ur, u, attr = g["ur_0"], g["u_0"], g["attr"]
    assert (g["u_0"].shape, attr.shape, ur.shape, g["p_H_i"].shape) == ((4, 3), (7, 2), (4, 5), (5, 1))
    assert (ur[0] == I).all() and (ur[1] != I).all()                              # all padding; a full list
    assert sorted(ur[2][ur[2] != I].tolist()) != sorted(set(ur[2][ur[2] != I].tolist()))      # one item twice in a list
    assert 0 in ur[3] and (attr[I] == attr[0]).all()                              # item 0; the padding row copies it
    assert any(len(set(r.tolist())) < len(r) for r in u) and any(len(set(r.tolist())) < len(r) for r in attr[:I])
    assert [g["p_" + k].shape[0] for k in R.TABLES] == [10, 12, 10, 11]
    # padded pairs contribute nothing and the padding column of pre is item 0's
    assert (g["pos_r_0"][ur == I] == 0).all() and np.array_equal(g["pre_0"][:, I], g["pre_0"][:, 0])


def test_reader_matches_the_reference_reader(tmp_path):
    from paddlerec_amd.reader import EnsfmDataset, EnsfmReader
    for name in ("train", "test"):
        with open(os.path.join(GOLDEN, "ensfm_%s_sample.csv" % name)) as f:
            (tmp_path / (name + ".csv")).write_text(f.read())
    want = np.load(os.path.join(GOLDEN, "ensfm_reader.npz"))
    files = sorted(str(p) for p in tmp_path.iterdir())
    tr, te = EnsfmDataset(files, "train"), EnsfmDataset(files, "test")
    assert [tr.user_field_M, tr.item_field_M, tr.user_bind_M, tr.item_bind_M, tr.max_positive_len] == want["sizes"].tolist()
    assert len(tr) == len(want["user_train"]) and len(te) == len(want["user_test"])
    rows = [tr[i] for i in range(len(tr))]
    assert np.array_equal(np.stack([r[0] for r in rows]), want["user_train"])
    assert np.array_equal(np.stack([r[2] for r in rows]), want["item_train"])
    assert all(np.array_equal(r[1], want["item_map_list"]) and int(r[3]) == int(want["item_bind_M"]) for r in rows)
    assert np.array_equal(np.stack([te[i][0] for i in range(len(te))]), want["user_test"])
    assert np.array_equal(te[0][1], want["item_map_list_test"])
    assert np.array_equal(tr.item_map_list[-1], tr.item_map_list[0])             # the duplicated last row
    key = lambda a: sorted(map(tuple, a.tolist()))
    assert key(tr.train_pairs) == key(want["train_pairs"]) and key(tr.test_pairs) == key(want["test_pairs"])
    # the loader: batches of stacked rows, the last partial one dropped, ONE attribute tensor behind a leading axis
    rd = EnsfmReader(files, 32, "cpu", "test")
    batches = list(rd)
    assert len(batches) == len(te) // 32 and all(b[0].shape == (32, want["user_test"].shape[1]) for b in batches)
    assert all(b[1].data_ptr() == rd.item_attribute.data_ptr() and b[1].shape[0] == 1 for b in batches)
    tm, sm = te.user_masks(batches[0][0], "cpu")
    uid = te.user_ids(batches[0][0].numpy())
    assert tm.shape == (32, tr.item_bind_M) and int(tm[0].sum()) == int((want["train_pairs"][:, 0] == uid[0]).sum())
    assert int(sm[5].sum()) == int((want["test_pairs"][:, 0] == uid[5]).sum())
    import paddlerec_amd.reader as reader_module
    assert "import scipy" not in open(reader_module.__file__).read()          # the reader works where scipy is absent


def test_hit_ratio_on_a_hand_made_score_matrix():
    from paddlerec_amd.ensfm import hit_ratios
    I = 24
    pre = torch.zeros(3, I + 1)
    pre[:, I] = 100.0                                        # the padding column: dropped, never a candidate
    # user 0: scores descend with the id; train positives 0 and 1 are masked, so the top 5 are 2..6
    pre[0, :I] = torch.arange(I, 0, -1, dtype=torch.float32)
    # user 1: a tie — items 3, 7, 9, 11, 13, 15 all score 5, nothing else is above 0; the lower ids win the five places
    pre[1, [3, 7, 9, 11, 13, 15]] = 5.0
    # user 2: distinct scores ascending with the id: the top k are the last k ids
    pre[2, :I] = torch.arange(I, dtype=torch.float32)
    train = torch.zeros(3, I, dtype=torch.bool)
    train[0, [0, 1]] = True
    test = torch.zeros(3, I, dtype=torch.bool)
    test[0, [2, 3, 20]] = True                               # 2 of 3 in the top 5, still 2 at 10, all 3 at 20
    test[1, [13, 15]] = True                                 # 13 is the 5th of the tied ids: in; 15 the 6th: out at k = 5
    test[2, [23, 0, 1, 2, 3, 4, 5]] = True                   # 7 test positives: the divisor is min(k, 7)
    hr = hit_ratios(pre, train, test)
    assert hr.shape == (3, 3)
    want = [[2 / 3, 1 / 2, 1 / 5], [2 / 3, 2 / 2, 1 / 7], [3 / 3, 2 / 2, 3 / 7]]            # [k][user]
    assert torch.allclose(hr, torch.tensor(want)), hr
    # infer.py:183-209 in numpy (argpartition leaves ties open; the untied users must agree with it exactly)
    p = pre[:, :-1].numpy().copy()
    p[train.numpy()] = -np.inf
    for ki, kk in enumerate((5, 10, 20)):
        top = np.argpartition(-p, kk, 1)[:, :kk]
        for b in (0, 2):
            hits = test.numpy()[b, top[b]].sum()
            assert abs(hits / min(kk, int(test[b].sum())) - float(hr[ki, b])) < 1e-6


def test_dygraph_model_mirrors_the_reference_methods():
    from paddlerec_amd.ensfm import DygraphModel, QUIRKS
    for name in ("create_model", "create_feeds", "create_loss", "create_optimizer", "create_metrics", "train_forward", "infer_forward"):
        assert callable(getattr(DygraphModel, name))
    assert "item 0" in QUIRKS and "Adagrad" in QUIRKS
    # create_loss is dygraph_model.py:40-51: on the golden's tensors it gives the golden's loss
    g = K.gold()["g"]
    t = lambda k: torch.as_tensor(g[k])
    h = torch.cat([t("p_H_i"), torch.ones(2, 1)])
    loss = DygraphModel().create_loss((t("pre_0"), t("pos_r_0"), t("q_emb_0"), t("p_emb_0"), h),
                                      {"hyper_parameters.negative_weight": float(g["w"][0])})
    assert abs(float(loss) - float(g["loss_0"][0])) <= 1e-5 * abs(float(g["loss_0"][0]))
    from paddlerec_amd import trainer
    assert "ensfm" in trainer.MODELS and trainer.guess_model("/x/models/recall/ensfm/config.yaml") == "ensfm"


def test_create_feeds_passes_device_tensors_through_and_keeps_item_bind_on_the_host(tmp_path):
    from paddlerec_amd.ensfm import DygraphModel
    from paddlerec_amd.reader import EnsfmReader
    for name in ("train", "test"):
        with open(os.path.join(GOLDEN, "ensfm_%s_sample.csv" % name)) as f:
            (tmp_path / (name + ".csv")).write_text(f.read())
    files = sorted(str(p) for p in tmp_path.iterdir())
    rd = EnsfmReader(files, 1, "cpu", "train")
    b0, b1 = list(rd)
    dm = DygraphModel()
    f0, f1 = dm.create_feeds(b0, "cpu"), dm.create_feeds(b1, "cpu")
    # a fresh view per batch over ONE storage: what the layer's grouping cache is keyed on
    assert f0[1] is not f1[1] and f0[1].data_ptr() == f1[1].data_ptr() == rd.item_attribute.data_ptr()
    assert (tuple(f0[1].shape), f0[1].stride(), f0[1]._version) == (tuple(f1[1].shape), f1[1].stride(), f1[1]._version)
    assert f0[0] is b0[0] and f0[2] is b0[2]                                      # already int64 on the device: no copy
    assert f0[3].device.type == "cpu" and int(f0[3]) == rd.dataset.item_bind_M
    # numpy feeds, as the reference's loader would hand them over, are converted
    g = dm.create_feeds([b0[0].numpy().astype(np.int32), b0[1].numpy(), b0[2].numpy(), np.asarray([rd.dataset.item_bind_M])], "cpu")
    assert all(t.dtype == torch.int64 for t in g) and torch.equal(g[0], b0[0]) and torch.equal(g[1], rd.item_attribute)
    # test mode: the bound user id of every row travels with the batch and selects the same masks as the host lookup
    te = EnsfmReader(files, 32, "cpu", "test")
    u, attr, uid = next(iter(te))
    assert uid.tolist() == te.dataset.user_ids(u.numpy())
    a, b = te.dataset.user_masks(u, "cpu", uid), te.dataset.user_masks(u, "cpu")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
