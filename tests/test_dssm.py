"""DSSM without a GPU: the numpy restatement (tests/dssm_ref.py) against the goldens recorded from the reference's own net.py /
dygraph_model.py (tools/make_golden_dssm.py), the parser against what the reference's two readers yield in CSR and dense form,
the constructions the reference fails on, the state_dict's names, the initialisation and the trainer's model table."""
import math
import os

import numpy as np
import pytest
import torch

import dssm_checks as K
import dssm_ref as R
from conftest import GOLDEN

SHIPPED = dict(trigram_d=2900, neg_num=1, slice_end=8, hidden_layers=[300, 300, 128], hidden_acts=["relu"] * 3)


@pytest.mark.parametrize("name", K.GOLDENS)
def test_ref_float64_matches_the_golden_on_every_recorded_tensor(name):
    G = K.gold(name)
    assert G["steps"] == 2 and G["lr"] == 0.001
    K.check_golden(G)
    # and the float32 restatement ALONE passes the same bounds (what the tool chose the seed by)
    for s in range(G["steps"]):
        K.check_step(G["r64"][s], G["r32"][s], G["lr"], s, G["r32"][s], "float32")


@pytest.mark.parametrize("name", K.GOLDENS)
def test_golden_holds_the_corner_cases(name):
    G = K.gold(name)
    g = G["g"]
    assert (G["trigram_d"], G["fc_sizes"], G["B"], G["neg"], G["slice_end"]) == (37, [12, 7, 5], 6, 2, 4)
    assert G["relu"] == [name == "dssm_relu.npz"] * 3
    for s in range(2):
        ql, dl = g["q_%d_lod" % s], g["d_%d_lod" % s]
        assert len(ql) == 7 and len(dl) == 19                       # two negatives, field-major
        per_row = np.concatenate([np.diff(ql), np.diff(dl)])
        assert per_row.min() == 0 and per_row.max() == 9
        vals = np.concatenate([g["q_%d_vals" % s], g["d_%d_vals" % s]])
        assert (vals != 1.0).sum() == 1 and not (vals == 0).any()
        for pre in ("q_%d" % s, "d_%d" % s):                        # ascending within a row
            c, lod = g[pre + "_cols"], g[pre + "_lod"]
            assert all((np.diff(c[lod[r]:lod[r + 1]]) > 0).all() for r in range(len(lod) - 1))
        assert g["cos_%d" % s].shape == (6, 3) and g["hit_%d" % s].shape == (4, 1)
    # slice_end 4 of B 6: the loss is the mean over four rows
    r = G["r64"][0]
    assert abs(float(r["loss"][0]) + float(np.log(r["hit_prob"]).mean())) < 1e-12 and len(r["hit_prob"]) == 4
    # Adam is not lazy: a weight row no sample touched in step 1 (zero gradient) still moves in step 1, on its first moment
    k = "query_linear_0.weight"
    idle = [c for c in range(37) if not g["g_1_" + k][c].any() and g["g_0_" + k][c].any()]
    assert idle and all((g["n_1_" + k][c] != g["n_0_" + k][c]).any() for c in idle)


def test_rows_beyond_slice_end_get_a_zero_gradient_and_no_negatives_give_zero():
    rng = np.random.default_rng(3)
    q, d = rng.standard_normal((6, 5)), rng.standard_normal((18, 5))
    h = R.head(q, d, 4)
    assert not h["dq"][4:].any() and not h["dd"].reshape(3, 6, 5)[:, 4:].any() and h["dq"][:4].all()
    cut = R.head(q[:4], d.reshape(3, 6, 5)[:, :4].reshape(12, 5), 4)
    assert np.allclose(cut["dq"], h["dq"][:4], rtol=1e-14, atol=0) and abs(cut["loss"] - h["loss"]) < 1e-15
    over = R.head(q, d, 9)                                            # slice_end above B: the mean is over B rows
    assert abs(over["loss"] - over["terms"].mean()) < 1e-15
    none = R.head(q, d[:6], 4)
    assert none["loss"] == 0 and not none["dq"].any() and not none["dd"].any() and (none["hit_prob"] == 1).all()


def test_the_clamped_cosine_branch_of_the_reference():
    q, d = np.asarray([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]), np.asarray([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0]])
    cs, aux = R.cosine(q, d)
    assert (cs == 0).all() and not aux[3].any()
    dx, dy = R.cosine_bwd(q, d, cs, aux, np.ones(2))
    assert np.array_equal(dx, d / 1e-8) and np.array_equal(dy, q / 1e-8)


def _csr_dense(z, kind, f, width=2900):
    return R.csr_dense(z["%s_%d_cols" % (kind, f)], z["%s_%d_vals" % (kind, f)], z["%s_%d_lod" % (kind, f)], width, np.float32)


def test_parser_matches_the_reference_readers():
    from paddlerec_amd.reader import DssmReader, dssm_csr, dssm_parse
    want = np.load(os.path.join(GOLDEN, "dssm_reader.npz"))
    train, test = os.path.join(GOLDEN, "dssm_sample_train.txt"), os.path.join(GOLDEN, "dssm_sample_test.txt")
    assert int(want["train_fields"][0]) == 3 and int(want["test_fields"][0]) == 2
    for kind, path, fields, n in (("train", train, None, 10), ("test", test, 2, 4)):
        lines = dssm_parse([path], fields)
        assert len(lines) == n
        for f in range(int(want[kind + "_fields"][0])):
            rows = [l[f] for l in lines]
            assert all(r.dtype == np.float32 and r.shape == (2900,) for r in rows)
            cols, vals, lod, row_of = dssm_csr(rows)
            for got, k in ((cols, "cols"), (vals, "vals"), (lod, "lod")):
                assert got.dtype == want["%s_%d_%s" % (kind, f, k)].dtype and np.array_equal(got, want["%s_%d_%s" % (kind, f, k)])
            assert np.array_equal(row_of, np.repeat(np.arange(n), np.diff(lod))) and row_of.dtype == np.int32
            assert np.array_equal(np.stack(rows), _csr_dense(want, kind, f))         # dense form, value for value
            # what the sparse route rests on: a row sets under 1 % of its 2 900 entries (2 to 17 in these lines), all to 1.0
            assert 2 <= np.diff(lod).min() and np.diff(lod).max() <= 17 and (vals == 1.0).all()
    # the infer reader takes the first two fields of a line that has three
    assert [len(l) for l in dssm_parse([train], 2)] == [2] * 10
    # batches: CSR by default (docs field-major: the batch's positives, then its negatives), the last batch short
    batches = list(DssmReader([train], 4, "cpu"))
    assert [int(b[0][2].numel()) - 1 for b in batches] == [4, 4, 2] and [int(b[1][2].numel()) - 1 for b in batches] == [8, 8, 4]
    dense = list(DssmReader([train], 4, "cpu", dense=True))
    assert [tuple(t.shape) for t in dense[2]] == [(2, 2900)] * 3 and all(t.dtype == torch.float32 for b in dense for t in b)
    for b, db in zip(batches, dense):
        q, d = (R.csr_dense(*(t.numpy() for t in x[:3]), 2900, np.float32) for x in b)
        assert np.array_equal(q, db[0].numpy()) and np.array_equal(d, torch.cat(db[1:]).numpy())
        want_dt = [torch.int64, torch.float32, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32]
        assert all([t.dtype for t in x] == want_dt for x in b)           # the CSR, row_of and the entries grouped by column
    for f in range(3):
        assert np.array_equal(torch.cat([db[f] for db in dense]).numpy(), _csr_dense(want, "train", f))
    infer = list(DssmReader([test], 1, "cpu", mode="infer"))
    assert len(infer) == 4 and all(int(b[1][2].numel()) == 2 for b in infer)


def test_csr_drops_exact_zeros_only():
    from paddlerec_amd.reader import dssm_csr
    rows = [np.asarray([0, 0.5, -0.0, 1, 1e-30, -2], np.float32), np.zeros(6, np.float32)]
    cols, vals, lod, row_of = dssm_csr(rows)
    assert cols.tolist() == [1, 3, 4, 5] and vals.tolist() == [0.5, 1.0, np.float32(1e-30), -2.0]
    assert lod.tolist() == [0, 4, 4] and row_of.tolist() == [0, 0, 0, 0]


def test_host_grouping_is_the_device_grouping_s_format():
    """reader.dssm_group against the definition in include/recengine.h (rec_ids_group): positions stably sorted by column,
    the distinct columns ascending, their segments, the counts; a column outside the table is dropped."""
    from paddlerec_amd.reader import dssm_group
    cols = np.asarray([5, 2, 9, 2, 5, 5, 0, 12, -1, 2], np.int64)
    sp, uq, seg, nu = dssm_group(cols, 10)
    assert (sp.dtype, uq.dtype, seg.dtype, nu.dtype) == (np.int32, np.int64, np.int32, np.int32)
    assert (len(sp), len(uq), len(seg), nu.tolist()) == (10, 10, 11, [4, 8, 0, 0])
    assert sp[:8].tolist() == [6, 1, 3, 9, 0, 4, 5, 2] and uq[:4].tolist() == [0, 2, 5, 9] and seg[:5].tolist() == [0, 1, 4, 7, 8]
    sp, uq, seg, nu = dssm_group(np.zeros(0, np.int64), 10)
    assert (len(sp), len(uq), len(seg), nu.tolist()) == (1, 1, 1, [0, 0, 0, 0])
    rng = np.random.default_rng(0)
    cols = rng.integers(0, 37, 500)
    sp, uq, seg, nu = dssm_group(cols, 37)
    for u in range(nu[0]):
        mine = sp[seg[u]:seg[u + 1]]
        assert (cols[mine] == uq[u]).all() and (np.diff(mine) > 0).all()
    assert seg[nu[0]] == 500 and (np.diff(uq[:nu[0]]) > 0).all()


def test_constructions_the_reference_fails_on():
    from paddlerec_amd.dssm import DSSMLayer, layer_kinds
    assert layer_kinds([3, 2], ["relu", "relu"]) == ["linear", "relu", "linear", "relu"]
    assert layer_kinds([3, 2, 2], ["", "", ""]) == ["linear"] * 3
    assert layer_kinds([3], ["relu"]) == ["linear", "relu"]
    assert layer_kinds([3, 2], ["tanh", "relu", "relu"]) == ["linear", "linear", "relu"]     # only "relu" adds a sublayer
    for sizes, acts, word in (([3, 2], ["relu", "tanh"], "a ReLU"), ([3, 2], ["relu", ""], "a ReLU"), ([3], [""], "no entry"),
                              ([3, 2], ["relu"], "shorter"), ([3], [], "shorter"), ([], [], "empty")):
        with pytest.raises(ValueError, match=word):
            layer_kinds(sizes, acts)
        with pytest.raises(ValueError, match=word):
            DSSMLayer(7, 1, 4, sizes, acts, device="cpu")
    with pytest.raises(ValueError, match=r"_query_layers\[-2\]\.bias"):
        layer_kinds([3, 2], ["relu", "sigmoid"])


def test_state_dict_names_shapes_and_initialisation():
    from paddlerec_amd.dssm import QUIRKS, DSSMLayer
    torch.manual_seed(5)
    m = DSSMLayer(device="cpu", **SHIPPED)
    sd = m.state_dict()
    h = [2900, 300, 300, 128]
    want = {"%s_linear_%d.%s" % (t, i, k): ((h[i], h[i + 1]) if k == "weight" else (h[i + 1],))
            for t in ("query", "pos") for i in range(3) for k in ("weight", "bias")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want            # the ReLU sublayers hold no parameters
    mm, vv = m.moments()
    assert sorted(mm) == sorted(vv) == sorted(want) and not any(t.any() for t in mm.values())
    assert sorted(m._optimizer_views()) == sorted("dssm.%s.%s" % (s, k) for s in "mv" for k in want)
    for name, t in sd.items():
        i = int(name.split("_")[2][0])
        std = math.sqrt(2.0 / (h[i] + h[i + 1]))                          # XavierNormal — the bias too
        n = t.numel()
        assert abs(float(t.std()) / std - 1) < 4 / math.sqrt(2 * n) + 1e-3, (name, float(t.std()), std)
        assert abs(float(t.mean())) < 4 * std / math.sqrt(n), name
    assert float(sd["query_linear_0.weight"].flatten()[:100].sub(sd["pos_linear_0.weight"].flatten()[:100]).abs().max()) > 0
    assert all(t.data_ptr() % 16 == 0 for t in sd.values())               # float4 rows
    assert "neg_num" in QUIRKS and "slice_end" in QUIRKS and "[-2]" in QUIRKS
    m.set_dict({"pos_linear_2.bias": np.arange(128, dtype=np.float32)})
    assert float(m.state_dict()["pos_linear_2.bias"][5]) == 5.0


def test_dygraph_model_restates_the_loss_and_has_no_optimizer():
    from paddlerec_amd.dssm import DygraphModel
    dm = DygraphModel()
    hit = torch.tensor([[0.5], [0.25]])
    assert abs(float(dm.create_loss(hit)) - 1.5 * math.log(2)) < 1e-6
    assert dm.create_optimizer(None, {}) is None and dm.create_metrics("cpu") == ([], [])
    feeds = dm.create_feeds_train([np.ones((2, 7)), np.zeros((2, 7)), np.ones((2, 7))], 7, "cpu")
    assert len(feeds) == 3 and all(f.dtype == torch.float32 and tuple(f.shape) == (2, 7) for f in feeds)
    assert len(dm.create_feeds_infer([np.ones((2, 7)), np.zeros((2, 7)), np.ones((2, 7))], 7, "cpu")) == 2


def test_trainer_knows_the_model():
    from paddlerec_amd import trainer
    assert "dssm" in trainer.MODELS and trainer.MODELS[-1] == "dssm"
    assert trainer.guess_model("/somewhere/models/match/dssm/config.yaml") == "dssm"
    assert type(trainer._dygraph_model("dssm")).__module__ == "paddlerec_amd.dssm"
    assert "|dssm]" in trainer.__doc__
    assert trainer._batch_size([(None, None, torch.zeros(5, dtype=torch.int64), None)]) == 4
