"""NCF without a GPU: the numpy restatement (tests/ncf_ref.py) against the goldens recorded from the reference's own net.py /
dygraph_model.py (tools/make_golden_ncf.py), the parser against what the reference's movielens_reader.py yields, evaluate.py's
metric on crafted cases, the `prediction` width rule, the state_dict's names, the initialisation and the host query of the
fused kernels' eligibility."""
import math
import os

import numpy as np
import pytest
import torch

import ncf_checks as K
import ncf_ref as R
from conftest import GOLDEN

SHIPPED = dict(num_users=6040, num_items=3706, mf_dim=8, layers=[64, 32, 16, 8])


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
    assert (int(g["num_users"][0]), int(g["num_items"][0]), G["layers"]) == (7, 9, [8, 6, 5, 2])
    assert G["mf_dim"] == (3 if G["mode"] == "NCF_NeuMF" else 2)
    for s in range(2):
        u, i, y = (g["%s_%d" % (k, s)] for k in ("users", "items", "labels"))
        assert len(u) == 6 and np.bincount(u).max() >= 3 and np.bincount(i).max() >= 2 and set(y.tolist()) == {0, 1}
    # Adam is not lazy: a row that step 0 touched and step 1 did not still moves in step 1, on its first moment
    late = 0
    for k in G["p"]:
        if "Embedding" in k:
            ids = "users_%d" if "User" in k else "items_%d"
            rows = sorted(set(g[ids % 0].tolist()) - set(g[ids % 1].tolist()))
            assert (g["n_0_" + k] != g["p_" + k]).any(1).sum() == len(set(g[ids % 0].tolist()))
            assert all((g["n_1_" + k][r] != g["n_0_" + k][r]).all() for r in rows)
            late += len(rows)
    assert late > 0


def test_parser_matches_the_reference_reader():
    from paddlerec_amd.reader import NcfReader, ncf_parse
    want = np.load(os.path.join(GOLDEN, "ncf_reader.npz"))
    path = os.path.join(GOLDEN, "ncf_sample.txt")
    got = ncf_parse([path])
    for k, a in zip(("users", "items", "labels"), got):
        assert a.dtype == np.int64 and np.array_equal(a, want[k])
    batches = list(NcfReader([path, path], 32, "cpu"))
    assert [b[0].shape for b in batches] == [(32, 1)] * 6 + [(8, 1)]                # the last batch is short
    assert all(t.dtype == torch.int64 for b in batches for t in b)
    for c, k in enumerate(("users", "items", "labels")):
        assert np.array_equal(torch.cat([b[c] for b in batches]).view(-1).numpy(), np.tile(want[k], 2))


def evaluate_py(pair):
    """evaluate.py:44-68, its loop as it stands (without result[:-1]) over [user, prediction, label] lines."""
    def takeSecond(x):
        return x[1]
    hits, ndcg = [], []
    pair = [pair[i:i + 100] for i in range(0, len(pair), 100)]
    for user in pair:
        user.sort(key=takeSecond, reverse=True)
        each_user_top10_line = user[:10]
        each_user_top10_line_label = [i[2] for i in each_user_top10_line]
        if 1 in each_user_top10_line_label:
            i = each_user_top10_line_label.index(1)
            ndcg.append(math.log(2) / math.log(i + 2))
            hits.append(1)
        else:
            hits.append(0)
            ndcg.append(0)
    return len(hits), np.array(hits).mean(), np.array(ndcg).mean()


def _metric_cases():
    rng = np.random.default_rng(5)
    base = lambda: (rng.permutation(100) / 100.0 + 1.0, np.zeros(100, np.int64))
    # ties at the 10th place: nine scores above, then five lines tied; only the FIRST tied line in file order is in the top 10
    p, y = base()
    p[:] = 0.0
    p[20:29] = 0.9
    p[[40, 50, 60, 70, 80]] = 0.5
    ya, yb = y.copy(), y.copy()
    ya[40], yb[50] = 1, 1
    yield "tie at the 10th place, the first tied line", p, ya
    yield "tie at the 10th place, the second tied line", p.copy(), yb
    # two positives in one chunk: the better-ranked one counts
    p, y = base()
    order = np.argsort(-p)
    y[order[3]] = y[order[7]] = 1
    yield "two positives", p, y
    p, y = base()
    y[np.argsort(-p)[10]] = 1                               # rank 11: a miss
    yield "a positive at rank 11", p, y
    yield "no positive", *base()
    # three chunks, the last of 7 lines with its positive ranked 2nd of 7
    p = np.concatenate([base()[0], base()[0], rng.permutation(7) / 7.0])
    y = np.zeros(207, np.int64)
    y[np.argsort(-p[:100])[0]] = 1
    y[200 + np.argsort(-p[200:])[1]] = 1
    yield "a short last chunk", p, y


@pytest.mark.parametrize("case", list(_metric_cases()), ids=lambda c: c[0])
def test_metric_equals_evaluate_py(case):
    from paddlerec_amd.ncf import hr_ndcg
    _, p, y = case
    p = p.astype(np.float32)
    want = evaluate_py([[0, float(a), int(b)] for a, b in zip(p, y)])
    got = hr_ndcg(torch.from_numpy(p), torch.from_numpy(y))
    ref = R.hr_ndcg(p, y)
    for g in (got, ref):
        assert g[0] == want[0] and abs(g[1] - want[1]) < 1e-12 and abs(g[2] - want[2]) < 1e-12, (g, want)
    assert hr_ndcg(torch.from_numpy(p), torch.from_numpy(y), chunk=100, top=10) == got


def test_metric_cases_are_what_they_say():
    c = {name: evaluate_py([[0, float(a), int(b)] for a, b in zip(p.astype(np.float32), y)]) for name, p, y in _metric_cases()}
    assert c["tie at the 10th place, the first tied line"][1:] == (1.0, math.log(2) / math.log(11))
    assert c["tie at the 10th place, the second tied line"][1:] == (0.0, 0.0)
    assert c["two positives"][1:] == (1.0, math.log(2) / math.log(5))
    assert c["a positive at rank 11"][1:] == (0.0, 0.0) and c["no positive"][1:] == (0.0, 0.0)
    assert c["a short last chunk"][0] == 3 and abs(c["a short last chunk"][1] - 2 / 3) < 1e-12
    assert abs(c["a short last chunk"][2] - (1.0 + 0.0 + math.log(2) / math.log(3)) / 3) < 1e-12


def test_prediction_width_rule():
    from paddlerec_amd.ncf import NCFLayer, prediction_width
    with pytest.raises(ValueError, match=r"fc_layers\[2\] = 4 .* 5 wide"):
        prediction_width("NCF_NeuMF", 3, [8, 6, 4, 2])
    with pytest.raises(ValueError, match=r"fc_layers\[3\] = 2 .* 3 wide"):
        prediction_width("NCF_GMF", 3, [8, 6, 5, 2])
    for mode in ("NCF_GMF", "NCF_MLP"):
        with pytest.raises(ValueError, match=r"fc_layers\[3\], which \[8, 6, 5\] does not have .* width is (5|3)"):
            prediction_width(mode, 3, [8, 6, 5])
    with pytest.raises(ValueError):
        prediction_width("NCF_NeuMF", 3, [8, 6, 5])          # 3 + 5 != fc_layers[2]
    with pytest.raises(ValueError):
        NCFLayer(7, 9, 3, [8, 6, 4, 2], "NCF_NeuMF", device="cpu")
    with pytest.raises(ValueError):
        prediction_width("NCF_Other", 8, SHIPPED["layers"])
    assert [prediction_width(m, 8, SHIPPED["layers"]) for m in ("NCF_NeuMF", "NCF_GMF", "NCF_MLP")] == [16, 8, 8]
    assert prediction_width("NCF_NeuMF", 3, [8, 6, 5, 2]) == 5


@pytest.mark.parametrize("name", K.GOLDENS)
def test_state_dict_names_and_shapes_equal_the_goldens(name):
    G = K.gold(name)
    m = K.layer_of(G, "cpu")
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in G["p"].items()}
    # the views write through to the packed buffers and the flat dense buffer, and read back
    m.load_state_dict(G["p"])
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), G["p"][k]), k
    if m.mf and m.half:
        assert np.array_equal(m.packed["p"]["user"].numpy(),
                              np.concatenate([G["p"]["MF_Embedding_User.weight"], G["p"]["MLP_Embedding_User.weight"]], 1))
    from paddlerec_amd import ops
    assert m.P == ops.ncf_dense_numel(m.desc) == m.flat["p"].numel()
    assert float(m.flat["p"].abs().sum()) == pytest.approx(sum(float(np.abs(v).sum()) for k, v in G["p"].items() if "Embedding" not in k),
                                                            rel=1e-5)      # the padding floats are zero
    mm, vv = m.moments()
    assert sorted(mm) == sorted(vv) == sorted(sd)
    keys = m.extra_optimizer_state()
    assert sorted(keys) == sorted("ncf.%s.%s" % (s, k) for s in "mv" for k in sd)


@pytest.mark.parametrize("mode", ["NCF_NeuMF", "NCF_GMF", "NCF_MLP"])
def test_init_statistics_follow_the_reference(mode):
    from paddlerec_amd.ncf import NCFLayer
    torch.manual_seed(3)
    m = NCFLayer(device="cpu", mode=mode, **SHIPPED)
    for k, v in m.state_dict().items():
        if "Embedding" in k:
            assert abs(float(v.std()) / 0.01 - 1) < 0.05 and abs(float(v.mean())) < 1e-3, k
        elif k.startswith("layer_") and k.endswith(".weight"):
            std = 1 / math.sqrt(v.shape[0])
            assert float(v.abs().max()) <= 2 * std and float(v.std()) > 0.5 * std, k
        elif k.endswith(".bias"):
            assert float(v.abs().max()) == 0
    w = m.state_dict()["prediction.weight"]
    fan_in = {"NCF_NeuMF": 32, "NCF_GMF": 8, "NCF_MLP": 16}[mode]     # 2 layers[2]; the weight's own rows; 2 layers[3]
    assert m.kaiming_limit() == math.sqrt(6 / fan_in)
    assert 0 < float(w.abs().max()) <= m.kaiming_limit() and tuple(w.shape) == ({"NCF_NeuMF": 16}.get(mode, 8), 1)


def test_fused_eligibility_is_a_host_query():
    from paddlerec_amd import _lib, ops
    d = lambda mf, widths: ops.ncf_desc(6040, 3706, mf, widths)
    assert ops.ncf_fused_eligible(d(8, [64, 32, 16, 8])) and ops.ncf_fused_eligible(d(8, [])) and ops.ncf_fused_eligible(d(0, [64, 32, 16, 8]))
    assert not ops.ncf_fused_eligible(d(8, [512, 256, 128, 64]))
    assert not ops.ncf_fused_eligible(d(8, [128, 128, 64]))                   # within the widths, beyond the LDS
    assert not ops.ncf_fused_eligible(d(8, [16, 8, 8, 8, 8, 8]))              # more Linears than REC_NCF_MAX_FC
    # the budget of include/recengine.h, restated: weights + accumulators + one tile of REC_NCF_TILE samples
    for mf, widths in ((8, [64, 32, 16, 8]), (8, []), (0, [64, 32, 16, 8]), (8, [128, 64, 32]), (8, [128, 96, 32]), (8, [128, 128, 64])):
        P = ops.ncf_dense_layout(mf, widths)[1]
        S = sum(w | 1 for w in widths) + sum(w | 1 for w in widths[1:]) + 2 * ((mf | 1) if mf else 0) + 2 + 4
        fits = 4 * (2 * P + _lib.REC_NCF_TILE * S) <= _lib.REC_NCF_LDS_BYTES
        assert ops.ncf_fused_eligible(d(mf, widths)) == fits, (mf, widths, P, S)
    assert ops.ncf_dense_layout(8, [64, 32, 16, 8])[1] == 2764 == ops.ncf_dense_numel(d(8, [64, 32, 16, 8]))   # 2 761 floats, padded
    assert _lib.REC_NCF_LDS_BYTES == 64 * 1024


def test_dygraph_model_mirrors_the_reference_methods():
    from paddlerec_amd import trainer
    from paddlerec_amd.ncf import DygraphModel, QUIRKS
    for name in ("create_model", "create_feeds", "create_loss", "create_optimizer", "create_metrics", "train_forward", "infer_forward"):
        assert callable(getattr(DygraphModel, name))
    assert "layers[2]" in QUIRKS and "result[:-1]" in QUIRKS
    g = K.gold("ncf_neumf.npz")["g"]
    loss = DygraphModel().create_loss(torch.as_tensor(g["pred_0"]).view(-1, 1), torch.as_tensor(g["labels_0"]).view(-1, 1))
    assert abs(float(loss) - float(g["loss_0"][0])) <= 1e-6
    feeds = DygraphModel().create_feeds([g["users_0"].astype(np.int32), g["items_0"], torch.as_tensor(g["labels_0"])], "cpu")
    assert all(t.dtype == torch.int64 and tuple(t.shape) == (6, 1) for t in feeds)
    assert "ncf" in trainer.MODELS and trainer.guess_model("/x/models/recall/ncf/config.yaml") == "ncf"
