#!/usr/bin/env python3
"""Generate the word2vec fixtures under tests/golden/ by executing the reference's UNMODIFIED models/recall/word2vec/net.py,
dygraph_model.py, word2vec_reader.py and word2vec_infer_reader.py over the paddle shim (oracle/paddle_shim), the way
tools/make_golden_mind.py pins MIND.  Runs only where the reference tree is; the tests use the committed fixtures.

    python tools/make_golden_word2vec.py     # rewrites the fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: everything tools/make_golden_aitm.py sets
(F.binary_cross_entropy = torch's: the log clamped at -100, the backward's denominator at 1e-12, Paddle's semantics [EXT]),
and paddle.full, paddle.shape (a list of ints), paddle.squeeze with a list of axes, paddle.topk, F.normalize(axis=),
paddle.optimizer.SGD = torch's plain SGD, Embedding(sparse=True) (the shim's dense gradient holds the same numbers).

word2vec_rand.npz: V 50, D 12, neg 3, B 7, lr 0.25, built through DygraphModel.create_model from a flat config, EVERY
state_dict tensor overwritten with seeded normal draws (embedding_w / embedding_b are not zero).  The ids of each step: sample
0's true id is also one of its negatives; sample 1's input id equals its true id; sample 2's input id is 0; samples 3 and 4
share the input word; the LAST negative is the same for every sample; id 0 also appears as a true id.  TWO consecutive SGD
steps (create_feeds -> forward -> create_loss -> backward -> step).  Also one analogy batch, Q 5, k 4, through
Word2VecInferLayer over step 2's embedding: the tool asserts that the six best float64 scores of every query are pairwise
more than 1e-4 of the largest apart, so no tie rule enters.
The file: lr, steps, seed, p_<key> (the initial state_dict) and per step s: in_s [B], target_s [B, 1 + neg], true_logits_s
[B], neg_logits_s [B, neg], loss_s [1], g_s_<key> (dense), n_s_<key>; a_ids, b_ids, c_ids [Q], topk_values, topk_ids [Q, 4].
word2vec_train_sample.txt / word2vec_test_sample.txt: the first TRAIN_LINES / TEST_LINES lines of data/train/convert_sample.txt
and data/test/sample.txt; word2vec_word_count_dict.txt / word2vec_word_id_dict.txt: the two dict files; word2vec_reader.npz:
what the two reference readers yield for them, the window draw and the dict files' text."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from make_golden_aitm import _patch_shim as _patch_aitm      # noqa: E402
from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

SEED, STEPS, TRAIN_LINES, TEST_LINES = 20, 2, 40, 12
RAND = dict(V=50, D=12, neg=3, B=7, lr=0.25, Q=5, k=4)
BASE = "models/recall/word2vec"


def _patch_shim():
    paddle = _patch_aitm()
    import paddle.nn.functional as F
    ints = lambda r: [int(v) for v in r]
    paddle.full = lambda shape, fill_value, dtype="float32": torch.full(ints(shape), float(fill_value), dtype=paddle._dtype(dtype))
    paddle.shape = lambda x: list(x.shape)

    def squeeze(x, axis=None):
        for a in sorted(ints(axis if isinstance(axis, (list, tuple)) else [axis]), reverse=True) if axis is not None else ():
            x = x.squeeze(a)
        return x if axis is not None else x.squeeze()

    paddle.squeeze = squeeze
    paddle.topk = lambda x, k, axis=-1: torch.topk(x, k, dim=axis)
    F.normalize = lambda x, p=2, axis=1, epsilon=1e-12: torch.nn.functional.normalize(x, p=p, dim=axis, eps=epsilon)
    paddle.optimizer.SGD = lambda learning_rate=0.001, parameters=None, **kw: torch.optim.SGD(list(parameters), lr=learning_rate)
    return paddle


def _load():
    _patch_shim()
    net = load_ref_module(BASE + "/net.py", "ref_w2v_net")
    sys.modules["net"] = net                         # dygraph_model.py: `import net`
    dm = load_ref_module(BASE + "/dygraph_model.py", "ref_w2v_dygraph").DygraphModel()
    return net, dm


class _Np:
    """What the reference's create_feeds calls .numpy() on."""

    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


def _batch(rng):
    r = RAND
    B, V, neg = r["B"], r["V"], r["neg"]
    in_ids = rng.integers(1, V, B).astype(np.int64)
    true = rng.integers(1, V, B).astype(np.int64)
    negs = rng.integers(1, V, (B, neg)).astype(np.int64)
    negs[:, neg - 1] = negs[0, neg - 1]              # one negative shared by all samples
    negs[0, 0] = true[0]                             # a true id that is also one of its sample's negatives
    true[1] = in_ids[1]                              # an input id equal to its true id
    in_ids[2] = 0                                    # id 0 is an ordinary word ...
    true[5] = 0                                      # ... on the target side too
    in_ids[4] = in_ids[3]                            # two samples with the same input word
    return in_ids, true, negs


def golden_rand(seed):
    net, dm = _load()
    r = RAND
    rng = np.random.default_rng(seed)
    cfg = {"hyper_parameters.sparse_feature_number": r["V"], "hyper_parameters.sparse_feature_dim": r["D"],
           "hyper_parameters.neg_num": r["neg"], "hyper_parameters.optimizer.learning_rate": r["lr"]}
    m = dm.create_model(cfg)
    assert sorted(m.state_dict()) == ["embedding.weight", "embedding_b.weight", "embedding_w.weight"]
    assert tuple(m.state_dict()["embedding_b.weight"].shape) == (r["V"], 1)
    assert float(m.embedding_w.weight.abs().max()) == 0.0 and float(m.embedding.weight.abs().max()) <= 0.5 / r["D"]
    with torch.no_grad():
        for _, q in sorted(m.named_parameters()):
            q.copy_(torch.as_tensor(0.5 * rng.standard_normal(tuple(q.shape)), dtype=torch.float32))
    opt = dm.create_optimizer(m, cfg)
    rec = dict(lr=np.asarray([r["lr"]], np.float64), steps=np.asarray([STEPS], np.int64), seed=np.asarray([seed], np.int64))
    for k, v in m.state_dict().items():
        rec["p_" + k] = npy(v)
    for s in range(STEPS):
        in_ids, true, negs = _batch(rng)
        input_word, true_word, neg_word = dm.create_feeds([_Np(in_ids), _Np(true), _Np(negs)], cfg)
        true_logits, neg_logits = m.forward([input_word, true_word, neg_word])
        loss = dm.create_loss(true_logits, neg_logits, cfg)
        loss.backward()
        rec["in_%d" % s], rec["target_%d" % s] = in_ids, np.concatenate([true[:, None], negs], 1)
        rec["true_logits_%d" % s], rec["neg_logits_%d" % s] = npy(true_logits).reshape(-1), npy(neg_logits)
        rec["loss_%d" % s] = npy(loss).reshape(1)
        for k, q in m.named_parameters():
            rec["g_%d_%s" % (s, k)] = npy(q.grad)
        opt.step()
        opt.zero_grad(set_to_none=True)
        for k, q in m.state_dict().items():
            rec["n_%d_%s" % (s, k)] = npy(q)
    # the analogy batch over the trained embedding (infer.py:62-69: the whole vocabulary is all_label)
    import word2vec_ref as R
    W = rec["n_%d_embedding.weight" % (STEPS - 1)]
    Q, k = r["Q"], r["k"]
    for _ in range(1000):
        a, b, c = (rng.integers(0, r["V"], Q).astype(np.int64) for _ in range(3))
        if R.separated(R.scores(W, a, b, c), 6):
            break
    else:
        raise SystemExit("no separated analogy batch")
    s64 = np.sort(R.scores(W, a, b, c), 1)[:, ::-1][:, :6]
    assert (-(np.diff(s64, axis=1)) > 1e-4 * np.abs(s64[:, :1])).all()              # the docstring's assertion
    inf = net.Word2VecInferLayer(r["V"], r["D"], "emb")
    with torch.no_grad():
        inf.embedding.weight.copy_(torch.from_numpy(W))
        t = lambda x: torch.from_numpy(x.reshape(-1, 1))
        values, pred_idx = inf.forward(t(a), t(b), t(c), torch.arange(r["V"]))
    rec.update(a_ids=a, b_ids=b, c_ids=c, topk_values=npy(values).reshape(Q, k), topk_ids=npy(pred_idx).reshape(Q, k).astype(np.int64))
    return rec


def check_against_ref(rec):
    import word2vec_ref as R
    p = {k[2:]: rec[k] for k in rec if k.startswith("p_")}
    worst = {}
    for dtype in (np.float64, np.float32):
        cur, w = p, 0.0
        for s in range(STEPS):
            c, g, new = R.train_step(cur, rec["in_%d" % s], rec["target_%d" % s], RAND["lr"], dtype)
            pairs = [(c[n], rec["%s_%d" % (n, s)]) for n in ("true_logits", "neg_logits", "loss")]
            pairs += [(g[k], rec["g_%d_%s" % (s, k)]) for k in g] + [(new[k], rec["n_%d_%s" % (s, k)]) for k in new]
            w = max([w] + [R.relerr(x, y) for x, y in pairs])
            cur = {k: rec["n_%d_%s" % (s, k)] for k in p}
        worst[dtype] = w
    v, i = R.topk(R.scores(rec["n_%d_embedding.weight" % (STEPS - 1)], rec["a_ids"], rec["b_ids"], rec["c_ids"]), RAND["k"])
    assert np.array_equal(i, rec["topk_ids"]), (i, rec["topk_ids"])
    return worst[np.float64], worst[np.float32], R.relerr(v, rec["topk_values"])


def golden_reader():
    _patch_shim()
    base = os.path.join(REF, BASE)
    paths = {}
    for name, src, lines in (("word2vec_train_sample.txt", "data/train/convert_sample.txt", TRAIN_LINES),
                             ("word2vec_test_sample.txt", "data/test/sample.txt", TEST_LINES),
                             ("word2vec_word_count_dict.txt", "data/dict/word_count_dict.txt", None),
                             ("word2vec_word_id_dict.txt", "data/dict/word_id_dict.txt", None)):
        with open(os.path.join(base, src)) as f:
            head = f.readlines()[:lines]
        paths[name] = os.path.join(OUT, name)
        with open(paths[name], "w") as o:
            o.writelines(head)
    cfg = {"config_abs_dir": OUT, "runner.word_count_dict_path": "word2vec_word_count_dict.txt",
           "runner.word_id_dict_path": "word2vec_word_id_dict.txt", "hyper_parameters.window_size": 5,
           "hyper_parameters.neg_num": 5, "hyper_parameters.with_shuffle_batch": False, "runner.batch_size": 4}
    tr = load_ref_module(BASE + "/word2vec_reader.py", "ref_w2v_reader").RecDataset([paths["word2vec_train_sample.txt"]], cfg)
    out = dict(window=np.asarray([tr.random_generator], np.int64), window_size=np.asarray([5], np.int64),
               neg_num=np.asarray([5], np.int64))
    assert int(tr.random_generator) == 3                                  # the ONE window draw for window_size 5
    rows = list(tr)
    for i, n in enumerate(("input", "true", "neg")):
        out["train_" + n] = np.stack([r[i] for r in rows])
    assert (out["train_neg"] == out["train_neg"][0]).all()                # every sample: the same negatives
    inf = load_ref_module(BASE + "/word2vec_infer_reader.py", "ref_w2v_infer_reader").RecDataset(
        [paths["word2vec_test_sample.txt"]], cfg)
    rows = list(inf)
    for i, n in enumerate(("a", "b", "c", "label", "inputs_word")):
        out["infer_" + n] = np.stack([r[i] for r in rows])
    for n in ("word2vec_word_count_dict.txt", "word2vec_word_id_dict.txt"):
        out[n[9:-4]] = np.frombuffer(open(paths[n], "rb").read(), np.uint8)
    path = os.path.join(OUT, "word2vec_reader.npz")
    np.savez_compressed(path, **out)
    print("word2vec readers: %d train samples, %d infer lines, negatives %s -> %s (%d bytes)" % (
        len(out["train_input"]), len(rows), out["train_neg"][0].tolist(), path, os.path.getsize(path)))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_reader()
    rec = golden_rand(SEED)
    e64, e32, ev = check_against_ref(rec)
    print("word2vec_rand seed %d: word2vec_ref float64 err %.3g, float32 err %.3g, top-k values err %.3g" % (SEED, e64, e32, ev))
    assert e64 < 1e-5
    path = os.path.join(OUT, "word2vec_rand.npz")
    np.savez_compressed(path, **rec)
    print("word2vec_rand loss=%s keys=%d -> %s (%d bytes)" % ([float(rec["loss_%d" % s][0]) for s in range(STEPS)], len(rec), path,
                                                             os.path.getsize(path)))
