"""MIND (models/recall/mind) without a GPU: tests/mind_ref.py (float64) against the golden recorded from the reference's
net.py / dygraph_model.py, the layer on the CPU operator backend against it, state-dict names and the never-stepped tensors,
the log_q table, the negative sampler, the readers, the retrieval metrics and the trainer.  Tolerances: mind_checks.py."""
import math
import os

import numpy as np
import pytest
import torch

import mind_checks as K
import mind_cpu_kernels
import mind_ref as R
from conftest import GOLDEN

KEYS = ["item_emb.weight", "embedding_bias", "capsual_layer.routing_logits", "capsual_layer.bilinear_mapping_matrix",
        "capsual_layer.relu_layer.weight", "capsual_layer.relu_layer.bias"]


@pytest.fixture(scope="module")
def gold():
    return K.gold()


def test_golden_holds_the_cases_it_is_meant_to(gold):
    g, p = gold["g"], gold["p"]
    assert gold["steps"] == 2 and sorted(p) == sorted(KEYS) and gold["pow_p"] == 1.0 and gold["iters"] == 3
    assert p["item_emb.weight"].shape == (50, 12) and p["capsual_layer.bilinear_mapping_matrix"].shape == (12, 12)
    assert p["capsual_layer.routing_logits"].shape == (1, 3, 6) and p["embedding_bias"].shape == (50,)
    assert p["item_emb.weight"][0].any() and p["embedding_bias"].any()                 # overwritten, the padding row too
    assert g["log_q"].shape == (50,) and g["log_q"][0] == -np.inf and np.isfinite(g["log_q"][1:]).all()
    for s in range(2):
        hist, seq, label, neg = (g["%s_%d" % (n, s)] for n in ("hist", "seq_len", "label", "neg"))
        assert hist.shape == (7, 6) and {1, 5, 6} <= set(seq.tolist()) and neg.shape == (6,)
        assert seq[1] == 5 and hist[1, 5] == 17                                      # a non-zero id at a padded position
        assert seq[2] == 6 and hist[2, 1] == 0 and hist[3, 0] == hist[3, 1] != 0       # id 0 in the prefix; a duplicate
        assert label[4] == hist[0, 0] and neg[0] == label[2]                           # a shared row; an accidental hit
        assert (label != 0).all() and (neg != 0).all() and len(set(neg.tolist())) == 6
        W = g["W_%d" % s]
        assert W.shape == (7, 3, 6) and np.array_equal(W[1, :, 5], np.full(3, np.float32(1) / np.float32(3)))      # exactly 1/K
        assert g["g_%d_item_emb.weight" % s].shape == (50, 12) and not g["g_%d_item_emb.weight" % s][0].any()
        assert "g_%d_embedding_bias" % s not in g and "g_%d_capsual_layer.routing_logits" % s not in g
        for k in R.FROZEN:
            assert np.array_equal(g["n_%d_%s" % (s, k)], p[k])


def test_float64_reference_matches_every_array_of_the_golden(gold):
    K.check_golden(gold)


def test_the_capsules_carry_a_gradient_and_a_transposed_mapping_matrix_does_not_pass(gold):
    g, p = gold["g"], gold["p"]
    assert np.abs(g["g_0_capsual_layer.bilinear_mapping_matrix"]).max() > 1e-3
    q = dict(p, **{"capsual_layer.bilinear_mapping_matrix": p["capsual_layer.bilinear_mapping_matrix"].T.copy()})
    c = R.forward(q, g["hist_0"], g["seq_len_0"], g["label_0"], g["neg_0"], g["log_q"], gold["pow_p"], gold["iters"])
    assert R.relerr(c["caps2"], g["user_cap_0"]) > 1e-2


def test_layer_on_cpu_kernels_matches_the_reference(gold):
    m = K.layer_of(gold, "cpu", mind_cpu_kernels)
    assert sorted(m.state_dict()) == sorted(KEYS)
    K.check_layer(gold, m, "cpu mirror")
    assert m.step_count == 2
    ex = m.extra_optimizer_state()
    assert sorted(ex) == sorted("mtl.%s.%s" % (s, k) for s in "mv" for k in m.STEPPED)      # no moments for the frozen two
    m.eval()
    user_cap, W = m.forward(*K.feeds(gold, 0, "cpu")[:2])
    assert tuple(user_cap.shape) == (7, 3, 12) and tuple(W.shape) == (7, 3, 6)


def test_one_grouping_one_row_adam_one_dense_adam_per_step(gold):
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(mind_cpu_kernels, name)
            if name not in ("ids_group", "adam_rows_all", "adam_dense", "mind_routing_fwd", "mind_ssm_head", "emb_gather"):
                return fn
            return lambda *a, **kw: (calls.append((name, a)), fn(*a, **kw))[1]

    m = K.layer_of(gold, "cpu", Counting())
    m.set_dict(gold["p"])
    m.train_step(*K.feeds(gold, 0, "cpu")[:3], gold["lr"], neg=K.feeds(gold, 0, "cpu")[3])
    names = [n for n, _ in calls]
    assert [names.count(n) for n in ("ids_group", "adam_rows_all", "adam_dense", "mind_routing_fwd", "mind_ssm_head")] == [1] * 5
    rows = [a for n, a in calls if n == "ids_group"][0][0]
    g = gold["g"]
    B, T, n = 7, 6, 6
    assert rows.numel() == B * T + 2 * B + n                                             # the four sources, grouped once
    hist = torch.as_tensor(g["hist_0"]).reshape(-1)
    assert torch.equal(rows[:B * T], torch.where(hist == 0, torch.full_like(hist, -1), hist))       # padding id: dropped
    assert torch.equal(rows[B * T + B:B * T + 2 * B], torch.as_tensor(g["label_0"]))                # gather: id 0 would count
    pads = [a[2] for n, a in calls if n == "emb_gather"]
    assert pads == [0, 0, None, None, None]                          # history and query through the padding Embedding


def test_quirks_config_defaults_and_refusals():
    from paddlerec_amd.mind import QUIRKS, DygraphModel, Mind_Capsual_Layer, MindLayer
    import inspect
    sig = inspect.signature(MindLayer.__init__).parameters
    assert [sig[k].default for k in ("neg_samples", "maxlen", "pow_p", "capsual_iters", "capsual_max_k", "capsual_init_std")] == \
        [100, 30, 1.0, 3, 3, 1.0]
    sig = inspect.signature(Mind_Capsual_Layer.__init__).parameters
    assert [sig[k].default for k in ("iters", "maxlen", "k_max", "init_std")] == [3, 32, 3, 1.0]
    dm = DygraphModel()
    m = dm.create_model({"hyper_parameters.item_count": 40, "hyper_parameters.embedding_dim": 8, "hyper_parameters.hidden_size": 8,
                         "hyper_parameters.neg_samples": 5}, device="cpu", kernels=mind_cpu_kernels)
    assert m.capsual_layer.k_max == 4 and m.maxlen == 30 and m.capsual_layer.iters == 3      # dygraph_model.py's max_k is 4
    sd = m.state_dict()
    assert not sd["item_emb.weight"][0].any() and not sd["embedding_bias"].any() and not sd["capsual_layer.relu_layer.bias"].any()
    assert float(sd["item_emb.weight"].abs().max()) <= math.sqrt(6.0 / 48)
    assert dm.create_metrics("cpu") == ([], [])
    for word in ("axis=1", "1/k_max", "stop_gradient", "trainable=False", "embedding_dim must equal hidden_size", "padding_idx=0",
                 "paddle.gather", "-1e30", "BEFORE", "log_q[0] = -inf", "non-finite", "cannot be reproduced", "non-lazy",
                 "random.seed(12345)", "total = 1"):
        assert word in QUIRKS, word
    with pytest.raises(ValueError, match=r"net\.py:287-290"):
        MindLayer(40, 8, 12, 5, device="cpu", kernels=mind_cpu_kernels)
    with pytest.raises(ValueError, match="neg_samples"):
        MindLayer(40, 8, 8, 40, device="cpu", kernels=mind_cpu_kernels)
    for kw in (dict(maxlen=65), dict(k_max=9), dict(iters=0), dict(iters=9)):
        with pytest.raises(ValueError, match="must be in 1"):
            Mind_Capsual_Layer(8, 8, device="cpu", kernels=mind_cpu_kernels, **kw)
    with pytest.raises(ValueError, match=r"hist_item int64 \[B, 30\]"):
        m.forward(torch.zeros(2, 7, dtype=torch.int64), torch.ones(2, dtype=torch.int64))


def test_log_q_table_is_the_recorded_one_bit_for_bit(gold):
    from paddlerec_amd.mind import log_uniform_table
    prob, log_q = log_uniform_table(50, 6)
    assert log_q.dtype == torch.float32 and np.array_equal(log_q.numpy().view(np.uint32), gold["g"]["log_q"].view(np.uint32))
    assert prob[0] == 0 and log_q[0] == -np.inf and abs(float(prob.sum()) - 1.0) > 1e-3          # not normalised
    big = log_uniform_table(367983, 128)[1].numpy()                                      # the config's size: finite past row 0
    assert np.isfinite(big[1:]).all() and (np.diff(big[1:2000]) <= 0).all()


def test_a_label_of_zero_gives_a_non_finite_loss_as_in_the_reference(gold):
    m = K.layer_of(gold, "cpu", mind_cpu_kernels)
    m.set_dict(gold["p"])
    hist, seq, label, neg = K.feeds(gold, 0, "cpu")
    label = label.clone()
    label[5] = 0
    loss, _, _ = m.train_step(hist, seq, label, gold["lr"], neg=neg)
    assert not np.isfinite(loss.item())


def test_sampler_is_distinct_never_zero_and_rebuilt_from_seed_and_step(gold):
    m = K.layer_of(gold, "cpu", mind_cpu_kernels)
    a, b, c = m.sample_negatives(1), m.sample_negatives(1), m.sample_negatives(2)
    assert torch.equal(a, b) and not torch.equal(a, c) and a.dtype == torch.int64 and tuple(a.shape) == (6,)
    for step in range(1, 40):
        d = m.sample_negatives(step).tolist()
        assert len(set(d)) == 6 and 0 not in d and max(d) < 50
    from paddlerec_amd.mind import MindLayer
    other = MindLayer(50, 12, 12, 6, 6, device="cpu", kernels=mind_cpu_kernels, seed=7)
    assert not torch.equal(other.sample_negatives(1), a)
    m.set_dict(gold["p"])
    hist, seq, label, _ = K.feeds(gold, 0, "cpu")
    m.train_step(hist, seq, label, gold["lr"])                                         # no negatives given: the step's draw
    assert torch.equal(m._last["neg"], m.sample_negatives(1))


def test_readers_match_the_reference_readers():
    from paddlerec_amd.reader import MindInferReader, MindReader
    want = np.load(os.path.join(GOLDEN, "mind_reader.npz"))
    bs, maxlen, per_epoch = (int(want[k][0]) for k in ("batch_size", "maxlen", "batches_per_epoch"))
    rd = MindReader([os.path.join(GOLDEN, "mind_sample.txt")], bs, "cpu", maxlen, per_epoch)
    for epoch in range(2):
        batches = list(rd)
        n = len(want["train_hist_%d" % epoch])
        assert len(batches) == n // bs and n >= 2 * bs                                   # drop_last
        for i, (hist, target, seq) in enumerate(batches):
            assert hist.dtype == torch.int64 and tuple(hist.shape) == (bs, maxlen) and tuple(target.shape) == (bs, 1)
            for got, name in ((hist, "hist"), (target, "target"), (seq, "seq_len")):
                assert np.array_equal(got.numpy(), want["train_%s_%d" % (name, epoch)][bs * i:bs * i + bs]), (epoch, i, name)
    assert (want["train_seq_len_0"] >= 4).all() and (want["train_target_0"] != 0).all()
    inf = list(MindInferReader([os.path.join(GOLDEN, "mind_valid_sample.txt")], bs, "cpu", maxlen))
    assert len(inf) == len(want["infer_hist"]) // bs == 3
    for i, (hist, seq, ev) in enumerate(inf):
        assert tuple(hist.shape) == (bs, maxlen) and tuple(seq.shape) == (bs, 1) and tuple(ev.shape) == (bs, 1, maxlen)
        for got, name in ((hist, "hist"), (seq, "seq_len"), (ev, "eval")):
            assert np.array_equal(got.numpy(), want["infer_%s" % name][bs * i:bs * i + bs]), (i, name)


def _infer_py_metrics(user_embs, table, target_items, top_n):
    """infer.py:103-194 restated over a brute-force inner product (np.argsort in the place of faiss.IndexFlatIP)."""
    total, total_recall, total_ndcg, total_hitrate = 1, 0.0, 0.0, 0
    ni = user_embs.shape[1]
    flat = np.reshape(user_embs, [-1, user_embs.shape[-1]])
    scores = flat.astype(np.float64) @ table.astype(np.float64).T
    I = np.argsort(-scores, axis=1, kind="stable")[:, :top_n]
    D = np.take_along_axis(scores, I, 1)
    for i, iid_list in enumerate(target_items):
        recall, dcg = 0, 0.0
        item_list_set, item_cor_list = set(), []
        item_list = list(zip(np.reshape(I[i * ni:(i + 1) * ni], -1), np.reshape(D[i * ni:(i + 1) * ni], -1)))
        item_list.sort(key=lambda x: x[1], reverse=True)
        for j in range(len(item_list)):
            if item_list[j][0] not in item_list_set and item_list[j][0] != 0:
                item_list_set.add(item_list[j][0])
                item_cor_list.append(item_list[j][0])
                if len(item_list_set) >= top_n:
                    break
        iid_list = list(filter(lambda x: x != 0, list(iid_list)))
        true_item_set = set(iid_list)
        for no, iid in enumerate(item_cor_list):
            if iid == 0:
                break
            if iid in true_item_set:
                recall += 1
                dcg += 1.0 / math.log(no + 2, 2)
        idcg = 0.0
        for no in range(recall):
            idcg += 1.0 / math.log(no + 2, 2)
        total_recall += recall * 1.0 / len(iid_list)
        if recall > 0:
            total_ndcg += dcg / idcg
            total_hitrate += 1
    total += target_items.shape[0]
    return total_recall / total, total_ndcg / total, total_hitrate * 1.0 / total


def test_retrieval_metrics_match_infer_py_on_a_brute_force_search():
    from paddlerec_amd.mind import RetrievalMetrics, search_inner_product
    rng = np.random.default_rng(3)
    N, E, B, Kc, top_n = 300, 8, 9, 3, 20
    table = rng.standard_normal((N, E)).astype(np.float32)
    user = rng.standard_normal((B, Kc, E)).astype(np.float32)
    user[0, 1] = user[0, 0]                                                     # two capsules with the same hits: dedup
    table[0] = 10 * user[1, 0]                                                  # id 0 scores highest for sample 1: dropped
    target = np.zeros((B, 6), np.int64)
    scores = user.reshape(-1, E) @ table.T
    for b in range(B):
        best = np.argsort(-scores[b * Kc])
        target[b, :3] = [best[1], best[25], best[2]] if b % 2 == 0 else [best[40], best[50], best[60]]
    D, I = search_inner_product(mind_cpu_kernels, mind_cpu_kernels.Workspace("cpu"), torch.as_tensor(user.reshape(-1, E)),
                                torch.as_tensor(table), top_n, chunk=70)         # five chunks, the last one ragged
    want_I = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")[:, :top_n]
    assert np.array_equal(I.numpy(), want_I)
    rm = RetrievalMetrics(top_n)
    rm.update(D.numpy(), I.numpy(), target, Kc)
    want = _infer_py_metrics(user, table, target, top_n)
    got = rm.values()
    assert list(got) == ["recall@20", "ndcg@20", "hitrate@20"]
    assert np.allclose(list(got.values()), want, rtol=0, atol=1e-12) and 0 < want[0] < 1 and 0 < want[2] < 1
    assert rm.total == B + 1                                                    # the reference's total = 1 start


def test_trainer_knows_the_model_trains_and_infers(tmp_path):
    from paddlerec_amd import checkpoint, trainer
    assert "mind" in trainer.MODELS and "mind" in trainer.__doc__
    assert trainer.guess_model("/x/models/recall/mind/config.yaml") == "mind"
    assert type(trainer._dygraph_model("mind")).__module__ == "paddlerec_amd.mind"
    cfg = K.mind_config(tmp_path)
    out, m = trainer.train(cfg, "mind", device="cpu", kernels=mind_cpu_kernels)
    assert len(out) == 2 and out[1]["batches"] == 3 and np.isfinite(out[1]["loss"]) and m.step_count == 6
    assert not m.embedding_bias.any()                                                   # never stepped
    res = trainer.infer(cfg, "mind", device="cpu", kernels=mind_cpu_kernels)
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 12
    for r in res:
        assert all(0.0 <= r[k] <= 1.0 for k in ("recall@20", "ndcg@20", "hitrate@20"))
    m2 = trainer._dygraph_model("mind").create_model(cfg, "cpu", kernels=mind_cpu_kernels)
    checkpoint.load_model(out[1]["model_dir"], m2)
    assert m2.step_count == 6
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
