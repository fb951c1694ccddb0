"""MatchPyramid without a GPU: the numpy restatement (tests/match_pyramid_ref.py) against the goldens recorded from the
reference's own net.py / dygraph_model.py (tools/make_golden_match_pyramid.py), its rules on hand-made cases, the parser against
what the reference's reader yields, the constructions the reference fails on and the trainer's model table."""
import os

import numpy as np
import pytest
import torch

import match_pyramid_checks as K
import match_pyramid_ref as R
from conftest import GOLDEN

SMALL = dict(emb_path="", vocab_size=193368, emb_size=2, kernel_num=8, conv_filter=[2, 4], conv_act="relu", hidden_size=5,
             out_size=1, pool_size=[2, 2], pool_stride=[2, 2], pool_padding="VALID", pool_type="max", hidden_act="relu",
             sentence_left_size=7, sentence_right_size=21)


@pytest.mark.parametrize("name", K.GOLDENS)
def test_ref_float64_matches_the_golden_on_every_recorded_tensor(name):
    G = K.gold(name)
    assert G["steps"] == 2 and G["lr"] == 0.001
    K.check_golden(G)
    # and the float32 restatement ALONE passes the same bounds (what the tool chose the seed by)
    for s in range(G["steps"]):
        assert np.array_equal(G["r32"][s]["argmax"], G["r64"][s]["argmax"])
        K.check_step(G["r64"][s], G["r32"][s], G["lr"], s, G["r32"][s], "float32")


@pytest.mark.parametrize("name", K.GOLDENS)
def test_golden_holds_the_corner_cases(name):
    G = K.gold(name)
    g = G["g"]
    assert (G["B"], G["Ll"], G["Lr"], G["E"], G["K"], G["vocab"]) == (128, 7, 21, 6, 8, 193368)
    assert G["cfg"] == dict(pad=len(G["rows"]) - 1, filter=(2, 4), pool=(2, 2), stride=(2, 2), relu=name == "match_pyramid_relu.npz",
                            pairs=64)
    assert R.pooled_shape(7, 21, G["cfg"]) == (3, 10)                       # 240 features; row 6 and column 20 are dropped
    assert G["rows"][-1] == K.PAD and (np.diff(G["rows"]) > 0).all() and G["rows"][-2] < 40
    assert os.path.getsize(os.path.join(GOLDEN, name)) < os.path.getsize(os.path.join(GOLDEN, "dmr_E4.npz"))
    for s in range(2):
        left, right = g["left_%d" % s], g["right_%d" % s]
        assert left.dtype == right.dtype == np.int64 and left.shape == (128, 7) and right.shape == (128, 21)
        assert (left[0] == K.PAD).all() and (right[1, 12:] == K.PAD).all() and (right[1, :12] != K.PAD).any()
        assert (right[2] == K.PAD).all()
        r = G["r64"][s]
        assert not (r["hinge"] == 0).any()                                  # no hinge term pinned at 0
        assert (r["hinge"] > 0).any()
        assert not g["g_%d_emb.weight" % s][-1].any()                       # the padding row takes no gradient ...
        assert np.array_equal(g["n_%d_emb.weight" % s][-1], np.zeros(6, np.float32))        # ... and stays zero
        assert not r["dL"][0].any() and not r["dR"][2].any() and not r["dR"][1, 12:].any()
        assert not (g["p_conv.bias"] > 0).any()
    # argmax never names the unpooled row 6 or column 20
    am = G["r64"][0]["argmax"]
    assert (am // 21).max() == 5 and (am % 21).max() == 19


# The three test_yardstick_* cases pin tests/match_pyramid_ref.py itself — the rules every other comparison rests on — on inputs
# worked out by hand.  They run no code of the package and pass without it: they are not coverage of the feature.
def test_yardstick_same_padding_puts_the_smaller_half_in_front():
    assert [R.same_pad(k) for k in (1, 2, 3, 4, 10)] == [(0, 0), (0, 1), (1, 1), (1, 2), (4, 5)]
    # one left word, an identity embedding: cross is the indicator of right word 1; a [1, 4] filter of distinct weights
    table = np.asarray([[0.0], [1.0]])
    cfg = dict(pad=-1, filter=(1, 4), pool=(1, 1), stride=(1, 1), relu=False, pairs=1)
    f = R.interaction_fwd(table, [[1]], [[0, 0, 1, 0, 0, 0]], np.asarray([1.0, 2.0, 3.0, 4.0]).reshape(1, 1, 1, 4), [0.0], cfg)
    # out[j] = sum_b w[b] cross[j + b - 1] (one zero in front, two behind): the indicator at column 2 shows w[3] at j = 0
    assert f["pooled"].reshape(-1).tolist() == [4.0, 3.0, 2.0, 1.0, 0.0, 0.0]


def test_yardstick_pool_is_valid_takes_the_first_maximum_and_a_cell_may_win_twice():
    # E 1, left and right embeddings chosen so that cross = outer(l, r); a [1, 1] filter of weight 1 keeps the image
    table = np.asarray([[0.0], [1.0], [2.0], [3.0]])
    w, b = np.ones((1, 1, 1, 1)), [0.0]
    cfg = dict(pad=0, filter=(1, 1), pool=(2, 3), stride=(1, 2), relu=True, pairs=1)
    left, right = [[1, 2, 1]], [[1, 1, 3, 1, 0, 2]]                        # the last column is beyond the last window
    f = R.interaction_fwd(table, left, right, w, b, cfg)
    assert R.pooled_shape(3, 6, cfg) == (2, 2)
    # image rows: [1 1 3 1 0 2], [2 2 6 2 0 4], [1 1 3 1 0 2]; windows of 2 x 3 at rows 0 / 1 and columns 0 / 2
    assert f["pooled"].tolist() == [[6.0, 6.0, 6.0, 6.0]] and f["argmax"].tolist() == [[8, 8, 8, 8]]      # cell (1, 2) wins all
    bw = R.interaction_bwd(f, np.asarray([[1.0, 10.0, 100.0, 1000.0]]), cfg)
    assert bw["d_cross"][0, 1, 2] == 1111.0 and np.count_nonzero(bw["d_cross"]) == 1
    assert bw["dL"][0].reshape(-1).tolist() == [0.0, 3333.0, 0.0] and bw["dR"][0].reshape(-1).tolist() == [0, 0, 2222.0, 0, 0, 0]
    # a tie: the first in row-major order
    f = R.interaction_fwd(table, [[1, 1]], [[2, 1, 2]], w, b, dict(cfg, pool=(2, 3), stride=(1, 1)))
    assert f["argmax"].tolist() == [[0]]
    # a window that is all <= 0 before ReLU: pooled 0, nothing passes
    f = R.interaction_fwd(table, [[1, 1]], [[2, 1, 2]], -w, b, dict(cfg, pool=(2, 3), stride=(1, 1)))
    bw = R.interaction_bwd(f, np.asarray([[5.0]]), dict(cfg, pool=(2, 3), stride=(1, 1)))
    assert f["pooled"].tolist() == [[0.0]] and not bw["d_cross"].any() and not bw["d_w"].any() and not bw["d_b"].any()


def test_yardstick_hinge_rows_beyond_the_pairs_and_the_gradient_at_zero():
    pred = np.asarray([2.0, 0.5, 1.0, 0.25, 0.0, 9.0, 7.0])               # pairs 3: rows 6 on are ignored
    loss, d, x = R.hinge(pred, 3)
    assert x.tolist() == [1 - 2.0 + 0.25, 1 - 0.5 + 0.0, 1 - 1.0 + 9.0]
    assert abs(loss - (0.5 + 9.0) / 3) < 1e-15 and d.tolist() == [0, -1 / 3, -1 / 3, 0, 1 / 3, 1 / 3, 0]
    loss, d, x = R.hinge(np.asarray([1.5, 0.5]), 1)                         # pinned at exactly 0: the gradient flows
    assert x[0] == 0 and loss == 0 and d.tolist() == [-1.0, 1.0]


def test_parser_matches_the_reference_reader(tmp_path):
    from paddlerec_amd.reader import LetorReader, letor_parse
    want = np.load(os.path.join(GOLDEN, "match_pyramid_reader.npz"))
    path = K.sample_train(tmp_path)                                        # the reference's whole 128-line sample
    left, right = letor_parse([path])
    assert left.dtype == right.dtype == np.int64 and left.shape == (128, 20) and right.shape == (128, 500)
    assert np.array_equal(left, want["left"]) and np.array_equal(right, want["right"])
    assert (right == K.PAD).any() and max(left.max(), right.max()) == K.PAD and min(left.min(), right.min()) >= 0
    batches = list(LetorReader([path], 50, "cpu"))
    assert [tuple(b[0].shape) for b in batches] == [(50, 20), (50, 20), (28, 20)] and len(LetorReader([path], 50, "cpu")) == 3
    assert all(b[0].dtype == b[1].dtype == torch.int64 and b[1].shape[1] == 500 for b in batches)
    assert np.array_equal(torch.cat([b[1] for b in batches]).numpy(), right)
    ragged = tmp_path / "ragged.txt"
    ragged.write_text("1,2\t3,4,5\n1\t3,4,5\n")
    with pytest.raises(ValueError, match="same sentence lengths"):
        letor_parse([str(ragged)])


def test_constructions_the_reference_fails_on():
    from paddlerec_amd.match_pyramid import QUIRKS, MatchPyramidLayer
    m = MatchPyramidLayer(device="cpu", **SMALL)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"emb.weight": (193368, 2), "conv.weight": (8, 1, 2, 4), "conv.bias": (8,),
                                                          "fc1.weight": (240, 5), "fc1.bias": (5,), "fc2.weight": (5, 1),
                                                          "fc2.bias": (1,)}
    assert not sd["emb.weight"][K.PAD].any() and sd["emb.weight"][:100].any()           # the padding row is zeroed at init
    assert not sd["conv.bias"].any() and not sd["fc1.bias"].any() and sd["fc1.weight"].any() and sd["conv.weight"].any()
    assert sorted(m._optimizer_views()) == sorted("match_pyramid.%s.%s" % (s, k) for s in "mv" for k in sd)
    for change, word in ((dict(vocab_size=193367), "padding_idx"), (dict(vocab_size=100), "padding_idx"),
                         (dict(kernel_num=4), "240"), (dict(pool_size=[2, 4]), "240"), (dict(sentence_right_size=23), "240"),
                         (dict(pool_type="avg"), "pool_type"), (dict(hidden_act=""), "hidden_act"),
                         (dict(hidden_act="tanh"), "hidden_act"), (dict(sentence_left_size=40, pool_size=[12, 2],
                                                                        pool_stride=[12, 2]), "above the kernels"),
                         (dict(conv_filter=[8, 4]), "fit"), (dict(emb_size=129), "above the kernels")):
        with pytest.raises(ValueError, match=word):
            MatchPyramidLayer(device="cpu", **dict(SMALL, **change))
    assert MatchPyramidLayer(device="cpu", **dict(SMALL, conv_act="tanh")).shape.relu == 0      # anything but "relu": no activation
    assert MatchPyramidLayer(device="cpu", **dict(SMALL, conv_act="relu")).shape.relu == 1
    ids = [torch.zeros(127, 7, dtype=torch.int64), torch.zeros(127, 21, dtype=torch.int64)]
    with pytest.raises(ValueError, match=r"\[0:64\] and \[64:128\]"):       # training needs B >= 128
        m.train_step(ids)
    for word in ("193367", "240", "pool_type", "hidden_act", "conv_act", "[64:128]", "channels", "create_metrics"):
        assert word in QUIRKS, word


def test_emb_path_is_loaded_when_the_file_exists(tmp_path):
    from paddlerec_amd.match_pyramid import MatchPyramidLayer
    table = np.arange(193368 * 2, dtype=np.float32).reshape(193368, 2)
    np.save(tmp_path / "embedding.npy", table)
    m = MatchPyramidLayer(device="cpu", **dict(SMALL, emb_path=str(tmp_path / "embedding.npy")))
    got = m.state_dict()["emb.weight"].numpy()
    assert np.array_equal(got[:K.PAD], table[:K.PAD]) and not got[K.PAD].any()


def test_dygraph_model_restates_the_loss_and_has_no_optimizer():
    from paddlerec_amd.match_pyramid import DygraphModel
    dm = DygraphModel()
    assert sorted(n for n in dir(dm) if not n.startswith("_")) == ["create_feeds", "create_loss", "create_metrics", "create_model",
                                                                  "create_optimizer", "infer_forward", "train_forward"]
    rng = np.random.default_rng(0)
    pred = rng.standard_normal((130, 1))
    assert abs(float(dm.create_loss(torch.as_tensor(pred))) - float(R.hinge(pred, 64)[0])) < 1e-12
    assert dm.create_optimizer(None, {}) is None and dm.create_metrics("cpu") == ([], [])
    feeds = dm.create_feeds([np.ones((2, 7)), np.zeros((2 * 21,))], 7, 21, "cpu")
    assert [tuple(f.shape) for f in feeds] == [(2, 7), (2, 21)] and all(f.dtype == torch.int64 for f in feeds)


def test_trainer_knows_the_model():
    from paddlerec_amd import trainer
    assert "match-pyramid" in trainer.MODELS and trainer.MODELS[-1] == "dssm"
    assert trainer.guess_model("/somewhere/models/match/match-pyramid/config.yaml") == "match-pyramid"
    assert type(trainer._dygraph_model("match-pyramid")).__module__ == "paddlerec_amd.match_pyramid"
    assert "|match-pyramid|dssm]" in trainer.__doc__
