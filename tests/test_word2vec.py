"""word2vec (paddlerec_amd/word2vec.py) on the CPU, through tests/word2vec_cpu_kernels.py: the golden against the NumPy
restatement, the layer's two steps, the loss's quirks, the readers and the trainer.  The device kernels are held to the same
reference in tests/test_word2vec_gpu.py."""
import os

import numpy as np
import pytest
import torch

import word2vec_checks as K
import word2vec_cpu_kernels
import word2vec_ref as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return K.gold()


def test_golden_matches_the_restatement_in_float64(gold):
    K.check_golden(gold)
    g = gold["g"]
    for s in range(gold["steps"]):
        i, t = g["in_%d" % s], g["target_%d" % s]
        assert t[0, 0] in t[0, 1:] and i[1] == t[1, 0] and i[2] == 0 and t[5, 0] == 0 and i[3] == i[4]      # the fixture's cases
        assert (t[:, -1] == t[0, -1]).all() and np.abs(g["p_embedding_w.weight"]).max() > 0
    # the analogy batch: ids exactly, no tie rule involved
    W = g["n_%d_embedding.weight" % (gold["steps"] - 1)]
    s64 = R.scores(W, g["a_ids"], g["b_ids"], g["c_ids"])
    assert R.separated(s64, 6)
    v, ids = R.topk(s64, 4)
    assert np.array_equal(ids, g["topk_ids"])
    K.check_close(g["topk_values"], R.topk(R.scores(W, g["a_ids"], g["b_ids"], g["c_ids"], np.float32), 4)[0], v, "golden top-k values")


def test_layer_two_steps_cpu(gold):
    m = K.layer_of(gold, "cpu", word2vec_cpu_kernels)
    assert list(m.state_dict()) == ["embedding.weight", "embedding_w.weight", "embedding_b.weight"]
    assert tuple(m.emb_b.shape) == (50, 1) and not m.emb_w.any() and not m.emb_b.any()        # net.py:48, :56
    assert float(m.emb.abs().max()) <= 0.5 / 12                                                # net.py:32
    K.check_layer(gold, m, "cpu layer")
    from paddlerec_amd.word2vec import Word2VecInferLayer
    g = gold["g"]
    inf = Word2VecInferLayer(50, 12, device="cpu", kernels=word2vec_cpu_kernels, table=torch.as_tensor(g["n_1_embedding.weight"]))
    _, inf_ids = inf.forward(*(torch.as_tensor(g[n]).reshape(-1, 1) for n in ("a_ids", "b_ids", "c_ids")))
    assert np.array_equal(inf_ids.numpy(), gold["g"]["topk_ids"])


def test_loss_is_a_mean_of_means(gold):
    """BCE(true) is averaged over B and BCE(neg) over B neg (dygraph_model.py:60-66): a mean over B (1 + neg) differs."""
    from paddlerec_amd.word2vec import QUIRKS
    g, p = gold["g"], gold["p"]
    c = R.sgns(p["embedding.weight"], p["embedding_w.weight"], p["embedding_b.weight"], g["in_0"], g["target_0"])
    z = np.concatenate([c["true_logits"][:, None], c["neg_logits"]], 1)
    sp = lambda x: np.log1p(np.exp(x))
    terms = np.concatenate([sp(-z[:, :1]), sp(z[:, 1:])], 1)
    want = terms[:, 0].mean() + terms[:, 1:].mean()
    flat = terms.mean()
    assert abs(want - flat) > 0.1 * want                       # the two definitions are far apart on this batch
    assert abs(float(g["loss_0"][0]) - want) < 1e-6 * want and abs(float(c["loss"][0]) - want) < 1e-12 * want
    m = K.layer_of(gold, "cpu", word2vec_cpu_kernels)
    m.set_dict(p)
    loss, _, _ = m.train_step(torch.as_tensor(g["in_0"]), torch.as_tensor(g["target_0"]), gold["lr"])
    assert abs(float(loss) - want) < 1e-5 * want and abs(float(loss) - flat) > 0.1 * want
    assert "mean of means" in QUIRKS and "random.seed(12345)" in QUIRKS and "np.random.randint(1, window_size + 1)" in QUIRKS


def test_saturated_sigmoid_gives_100_and_a_zero_gradient():
    """A true logit <= -110 and a negative logit >= 20: the float32 sigmoid is exactly 0 / 1, each loss term is the clamp's 100,
    the gradient exactly 0 (two stages, not BCE-with-logits) and nothing is non-finite."""
    from paddlerec_amd.word2vec import Word2VecLayer
    m = Word2VecLayer(6, 4, 1, device="cpu", kernels=word2vec_cpu_kernels)
    m.record_gradients = True
    m.emb.zero_()
    m.emb_w.zero_()
    m.emb[1] = torch.tensor([1.0, 2.0, 0.0, -1.0])
    m.emb_w[2] = torch.tensor([-30.0, -20.0, 7.0, 41.0])       # <emb[1], emb_w[2]> = -111
    m.emb_w[3] = torch.tensor([5.0, 10.0, 3.0, 2.0])            # <emb[1], emb_w[3]> = 23
    m.emb_b[2], m.emb_b[3] = 0.5, -1.0                          # logits -110.5 and 22
    before = K.layer_state(m)
    with np.errstate(over="ignore"):
        loss, t, n = m.train_step(torch.tensor([1]), torch.tensor([[2, 3]]), 1.0)
    assert float(t[0]) == -110.5 and float(n[0, 0]) == 22.0
    assert float(loss) == 200.0                                 # 100 / 1 + 100 / (1 * 1)
    assert not m._last["g"].any() and torch.isfinite(m._last["g"]).all() and torch.isfinite(m._last["d_in"]).all()
    for k, v in m.last_gradients().items():
        assert not v.any() and torch.isfinite(v).all(), k
    for k, v in K.layer_state(m).items():
        assert np.array_equal(v, before[k]), k
    z = torch.tensor([-110.5, 22.0])                            # BCE-with-logits would give 110.5 + 22 and gradients -1, 1
    assert float(torch.nn.functional.binary_cross_entropy_with_logits(z, torch.tensor([1.0, 0.0]), reduction="sum")) == 132.5


def test_out_of_range_id_raises_through_status_and_updates_nothing(gold):
    from paddlerec_amd._lib import RecError
    g = gold["g"]
    for where in ("in", "target"):
        m = K.layer_of(gold, "cpu", word2vec_cpu_kernels)
        m.set_dict(gold["p"])
        in_ids, target_ids = torch.as_tensor(g["in_0"]).clone(), torch.as_tensor(g["target_0"]).clone()
        if where == "in":
            in_ids[3] = 50
        else:
            target_ids[2, 1] = -1
        before = K.layer_state(m)
        with pytest.raises(RecError, match="out of range"):
            m.train_step(in_ids, target_ids, gold["lr"], check_ids=True)
        assert int(m.status.item()) & 1 and m.step_count == 0
        for k, v in K.layer_state(m).items():
            assert np.array_equal(v, before[k]), (where, k)
        # without the host check the flagged pairs contribute nothing and the status word stays set for the trainer
        m.train_step(in_ids, target_ids, gold["lr"])
        gg = m._last["g"].numpy()
        assert (gg[3] == 0).all() if where == "in" else (gg[2, 1] == 0 and gg[2, 0] != 0)
        assert int(m.status.item()) & 1 and all(np.isfinite(v).all() for v in K.layer_state(m).values())


def test_readers_match_the_reference_readers(tmp_path):
    from paddlerec_amd.reader import Word2vecInferReader, Word2vecReader
    want = np.load(os.path.join(GOLDEN, "word2vec_reader.npz"))
    for n in ("word_count_dict", "word_id_dict"):               # the dict files the recording was made with
        assert open(os.path.join(GOLDEN, "word2vec_%s.txt" % n), "rb").read() == want[n].tobytes()
    bs, neg = 100, int(want["neg_num"][0])
    rd = Word2vecReader([os.path.join(GOLDEN, "word2vec_train_sample.txt")], bs, "cpu",
                        os.path.join(GOLDEN, "word2vec_word_count_dict.txt"), int(want["window_size"][0]), neg)
    assert rd.window == int(want["window"][0]) == 3             # ONE draw, np.random.seed(12345), for window_size 5
    assert (want["train_neg"] == want["train_neg"][0]).all()    # the identical negatives of every sample
    assert np.array_equal(rd.negatives(), want["train_neg"][0])
    for _ in range(2):                                          # a second pass yields the same samples
        batches = list(rd)
        assert len(batches) == len(want["train_input"]) // bs == 7            # drop_last
        for i, (in_ids, target_ids) in enumerate(batches):
            assert in_ids.dtype == target_ids.dtype == torch.int64 and tuple(in_ids.shape) == (bs,)
            assert tuple(target_ids.shape) == (bs, 1 + neg) and target_ids.is_contiguous()
            sl = slice(bs * i, bs * i + bs)
            assert np.array_equal(in_ids.numpy(), want["train_input"][sl, 0])
            assert np.array_equal(target_ids.numpy()[:, 0], want["train_true"][sl, 0])
            assert np.array_equal(target_ids.numpy()[:, 1:], want["train_neg"][sl])
    ids = os.path.join(GOLDEN, "word2vec_word_id_dict.txt")
    inf = list(Word2vecInferReader([os.path.join(GOLDEN, "word2vec_test_sample.txt")], 4, "cpu", ids))
    assert len(inf) == len(want["infer_a"]) // 4 == 3
    for i, batch in enumerate(inf):
        for got, name in zip(batch, ("a", "b", "c", "label", "inputs_word")):
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want["infer_" + name][4 * i:4 * i + 4]), (i, name)
    stop = tmp_path / "t.txt"                                   # reading stops at the first line that holds a ':'
    lines = open(os.path.join(GOLDEN, "word2vec_test_sample.txt")).readlines()
    stop.write_text("".join(lines[:3]) + ": capital-world\n" + "".join(lines[3:]))
    assert len(list(Word2vecInferReader([str(stop)], 1, "cpu", ids))) == 3


def test_trainer_knows_the_model_trains_and_infers(tmp_path):
    from paddlerec_amd import checkpoint, trainer
    from paddlerec_amd.word2vec import DygraphModel
    assert "word2vec" in trainer.MODELS and "word2vec" in trainer.__doc__
    assert trainer.guess_model("/x/models/recall/word2vec/config.yaml") == "word2vec"
    assert type(trainer._dygraph_model("word2vec")).__module__ == "paddlerec_amd.word2vec"
    assert DygraphModel().create_metrics("cpu") == ([], [])                              # dygraph_model.py:80-83
    cfg = K.w2v_config(tmp_path)
    out, m = trainer.train(cfg, "word2vec", device="cpu", kernels=word2vec_cpu_kernels)
    assert len(out) == 2 and out[1]["batches"] == 7 and np.isfinite(out[1]["loss"]) and m.step_count == 14
    assert out[1]["loss"] < out[0]["loss"] and m.emb_w.any() and m.emb_b.any() and int(m.status.item()) == 0
    m2 = trainer._dygraph_model("word2vec").create_model(cfg, "cpu", kernels=word2vec_cpu_kernels)
    checkpoint.load_model(out[1]["model_dir"], m2)
    assert m2.step_count == 14
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    res = trainer.infer(cfg, "word2vec", device="cpu", kernels=word2vec_cpu_kernels)
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 12 and res[1]["batches"] == 6
    # the acc the recorded analogy lines imply for the saved table: float64 scores, infer.py:138-146 on the host
    want = np.load(os.path.join(GOLDEN, "word2vec_reader.npz"))
    a, b, c, label = (want["infer_" + n].reshape(-1) for n in ("a", "b", "c", "label"))
    _, top4 = R.topk(R.scores(m.emb.numpy(), a, b, c), 4)
    hits = 0
    for ii in range(len(label)):
        for idx in top4[ii]:
            if int(idx) in want["infer_inputs_word"][ii]:
                continue
            hits += int(idx) == int(label[ii])
            break
    assert res[1]["acc"] == hits / len(label) and 0.0 <= res[0]["acc"] <= 1.0
