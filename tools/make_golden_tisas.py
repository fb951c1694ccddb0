#!/usr/bin/env python3
"""Generate the TiSASRec fixtures under tests/golden/ by executing the reference's UNMODIFIED models/recall/tisas/net.py,
dygraph_model.py and movielens_reader.py over the paddle shim (oracle/paddle_shim), the way tools/make_golden_word2vec.py pins
word2vec.  Runs only where the reference tree is; the tests use the committed fixtures.

    python tools/make_golden_tisas.py     # rewrites the fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: everything tools/make_golden_mind.py sets,
and nn.Conv1D (torch's conv1d, weight [C_out, C_in, k]), nn.LayerNorm (weight, bias, epsilon), nn.BCEWithLogitsLoss,
paddle.split (equal parts), paddle.ones, paddle.bool, paddle.get_default_dtype, Tensor.astype for Python types,
Tensor.transpose with a permutation, Embedding._embedding_dim, paddle.optimizer.Adam with its betas (torch's Adam: the same
update algebraically), tqdm / scipy stand-ins when missing.  nn.Dropout is the IDENTITY: the reference hard-codes 0.2 and its
masks cannot be reproduced; tests/tisas_ref.py takes explicit masks and the device tests rebuild theirs.

tisas_h1.npz / tisas_h2.npz: B 4, L 6, D 8, time_span 4, 11 items, 2 blocks, H 1 / H 2, built through
DygraphModel.create_model from a flat config, every state_dict tensor overwritten with seeded draws (layer-norm weights
around 1; item_emb row 0 stays zero, as Paddle keeps a padding row).  Sample 0 starts with padding, sample 1 is full,
sample 2 has one event, sample 3 is ALL padding (uniform attention rows, nothing selected for the loss); the time gaps
include 0 and values past the clip.  TWO consecutive Adam steps (train_forward -> backward -> step) and one infer call.
The file: lr, steps, heads, p_<key> and per step s: seq_s [B, L], tm_s [B, L, L], pos_s, neg_s [B, L], loss_s [1],
log_feats_s [B, L, D], g_s_<key> (dense), n_s_<key>; inf_seq, inf_tm, inf_items [B, 7], inf_logits [B, 7].
tisas_sample.txt: the reference's data/sample_data/sample_data.txt.  tisas_synth.txt: a ratings file from a fixed seed (see
synth()).  tisas_reader.npz: what the reference's RecDataset yields for both files in train and test mode."""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from make_golden_mind import _patch_shim as _patch_mind      # noqa: E402
from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

SEED, STEPS, LR = 7, 2, 0.001
SHAPE = dict(B=4, L=6, D=8, span=4, items=11, blocks=2, cand=7)
BASE = "models/recall/tisas"
READER_CASES = (("sample", "tisas_sample.txt", 50, 256, 4), ("synth", "tisas_synth.txt", 8, 6, 6))   # name, file, maxlen, span, draws


def _patch_shim():
    paddle = _patch_mind()
    import paddle.nn as nn
    paddle.bool = torch.bool
    paddle.get_default_dtype = lambda: "float32"
    paddle.ones = lambda shape, dtype="float32": torch.ones([int(v) for v in shape], dtype=paddle._dtype(dtype))
    paddle.split = lambda x, num_or_sections, axis=0: list(torch.chunk(x, int(num_or_sections), dim=axis))
    paddle.zeros_like = torch.zeros_like
    py = {int: torch.int64, float: torch.float32, bool: torch.bool}
    torch.Tensor.astype = lambda self, d: self.to(py[d] if d in py else paddle._dtype(d))
    if not getattr(torch.Tensor.transpose, "_takes_perm", False):
        plain = torch.Tensor.transpose

        def transpose(self, *a):
            return self.permute(*a[0]) if len(a) == 1 and isinstance(a[0], (list, tuple)) else plain(self, *a)

        transpose._takes_perm = True
        torch.Tensor.transpose = transpose

    class Identity(nn.Layer):
        def __init__(self, p=0.5):
            super().__init__()
            self.p = p

        def forward(self, x):
            return x

    class Conv1D(nn.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, weight_attr=None, bias_attr=None):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels, kernel_size))
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
            with torch.no_grad():
                weight_attr.initializer(self.weight)

        def forward(self, x):
            return torch.nn.functional.conv1d(x, self.weight, self.bias)

    class LayerNorm(nn.Layer):
        def __init__(self, normalized_shape, epsilon=1e-5):
            super().__init__()
            self.n, self.epsilon = int(normalized_shape), epsilon
            self.weight, self.bias = torch.nn.Parameter(torch.ones(self.n)), torch.nn.Parameter(torch.zeros(self.n))

        def forward(self, x):
            return torch.nn.functional.layer_norm(x, (self.n,), self.weight, self.bias, self.epsilon)

    if not hasattr(nn.Embedding, "_embedding_dim"):
        base = nn.Embedding

        class Embedding(base):
            def __init__(self, num_embeddings, embedding_dim, *a, **kw):
                super().__init__(num_embeddings, embedding_dim, *a, **kw)
                self._embedding_dim = embedding_dim

        nn.Embedding = Embedding
    nn.Dropout, nn.Conv1D, nn.LayerNorm, nn.BCEWithLogitsLoss = Identity, Conv1D, LayerNorm, torch.nn.BCEWithLogitsLoss
    paddle.optimizer.Adam = lambda learning_rate=0.001, parameters=None, beta1=0.9, beta2=0.999, epsilon=1e-8, **kw: \
        torch.optim.Adam(list(parameters), lr=learning_rate, betas=(beta1, beta2), eps=epsilon)
    for name, make in (("tqdm", lambda m: setattr(m, "tqdm", lambda it, **kw: it)), ("scipy", lambda m: None),
                       ("scipy.sparse", lambda m: None)):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            make(mod)
            sys.modules[name] = mod
    if "scipy" in sys.modules and "scipy.sparse" in sys.modules and not hasattr(sys.modules["scipy"], "sparse"):
        sys.modules["scipy"].sparse = sys.modules["scipy.sparse"]
    return paddle


def _load():
    _patch_shim()
    net = load_ref_module(BASE + "/net.py", "ref_tisas_net")
    sys.modules["net"] = net                         # dygraph_model.py: `import net`
    dm = load_ref_module(BASE + "/dygraph_model.py", "ref_tisas_dygraph").DygraphModel()
    return net, dm


def _batch(rng, step):
    s = SHAPE
    B, L, N, span = s["B"], s["L"], s["items"], s["span"]
    seq, pos, neg, ts = (np.zeros((B, L), np.int64) for _ in range(4))
    lens = [3, L, 1, 0] if step == 0 else [L, 2, 0, 4]
    for b, n in enumerate(lens):
        if n == 0:
            continue
        items = rng.integers(1, N + 1, n + 1)
        seq[b, L - n:], pos[b, L - n:] = items[:-1], items[1:]
        neg[b, L - n:] = rng.integers(1, N + 1, n)
        gaps = rng.integers(0, 4, n)
        gaps[0] = 1
        if n > 2:
            gaps[1], gaps[2] = 0, span + 3            # a gap of 0 and one past the clip
        ts[b, L - n:] = np.cumsum(gaps)
    tm = np.minimum(np.abs(ts[:, :, None] - ts[:, None, :]), span).astype(np.int64)
    assert tm.min() == 0 and tm.max() == span
    return seq, tm, pos, neg


def golden_model(heads, seed):
    net, dm = _load()
    s = SHAPE
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    cfg = {"hyper_parameters.num_users": 5, "hyper_parameters.num_items": s["items"], "hyper_parameters.hidden_units": s["D"],
           "hyper_parameters.maxlen": s["L"], "hyper_parameters.time_span": s["span"], "hyper_parameters.num_blocks": s["blocks"],
           "hyper_parameters.num_heads": heads, "hyper_parameters.optimizer.learning_rate": LR}
    m = dm.create_model(cfg)
    with torch.no_grad():
        for k, q in sorted(m.named_parameters()):
            draw = torch.as_tensor(0.4 * rng.standard_normal(tuple(q.shape)), dtype=torch.float32)
            q.copy_(1.0 + draw if "layernorm" in k and k.endswith("weight") else draw)
        m.item_emb.weight[0].zero_()
    opt = dm.create_optimizer(m, cfg)
    rec = dict(lr=np.asarray([LR], np.float64), steps=np.asarray([STEPS], np.int64), heads=np.asarray([heads], np.int64),
               seed=np.asarray([seed], np.int64))
    for k, v in m.state_dict().items():
        rec["p_" + k] = npy(v)
    assert tuple(rec["p_forward_layers.0.conv1.weight"].shape) == (s["D"], s["D"], 1)
    m.train()
    for st in range(STEPS):
        seq, tm, pos, neg = _batch(rng, st)
        batch = [torch.from_numpy(a) for a in (seq, tm, pos, neg)]
        loss, _, _ = dm.train_forward(m, [], batch, cfg)
        log_feats = m.seq2feats(batch[0], batch[1])
        loss.backward()
        rec.update({"seq_%d" % st: seq, "tm_%d" % st: tm, "pos_%d" % st: pos, "neg_%d" % st: neg,
                    "loss_%d" % st: npy(loss).reshape(1), "log_feats_%d" % st: npy(log_feats)})
        for k, q in m.named_parameters():
            rec["g_%d_%s" % (st, k)] = npy(q.grad) if q.grad is not None else np.zeros(tuple(q.shape), np.float32)
        opt.step()
        opt.zero_grad(set_to_none=True)
        for k, q in m.state_dict().items():
            rec["n_%d_%s" % (st, k)] = npy(q)
    m.eval()
    seq, tm, _, _ = _batch(rng, 0)
    items = rng.integers(1, s["items"] + 1, (s["B"], s["cand"])).astype(np.int64)
    with torch.no_grad():
        _, out = dm.infer_forward(m, [], [torch.from_numpy(a) for a in (seq, tm, items)], cfg)
    rec.update(inf_seq=seq, inf_tm=tm, inf_items=items, inf_logits=npy(out["prediction"]))
    return rec


def check_against_ref(rec):
    import tisas_ref as R
    p = {k[2:]: rec[k] for k in rec if k.startswith("p_")}
    H, worst = int(rec["heads"][0]), {}
    for dtype in (np.float64, np.float32):
        cur, st, w = p, None, 0.0
        for s in range(STEPS):
            c, g, new, _ = R.train_step(cur, rec["seq_%d" % s], rec["tm_%d" % s], rec["pos_%d" % s], rec["neg_%d" % s], H, LR, st,
                                        None, dtype)
            assert sorted(g) == sorted(p)
            pairs = [(c["loss"], rec["loss_%d" % s]), (c["log_feats"], rec["log_feats_%d" % s])]
            live = [k for k in g if not R.structural_zero(k)]
            pairs += [(g[k], rec["g_%d_%s" % (s, k)]) for k in live]
            errs = {k: R.relerr(g[k], rec["g_%d_%s" % (s, k)]) for k in live}
            for k in set(g) - set(live):                 # zero in exact arithmetic: noise on both sides
                assert np.abs(rec["g_%d_%s" % (s, k)]).max() <= 32 * 2.0 ** -24 * c["kbias_scale"][k], k
            w = max([w] + [R.relerr(x, y) for x, y in pairs])
            if dtype is np.float64 and max(errs.values()) > 1e-4:
                print("  step %d worst gradients: %s" % (s, sorted(errs.items(), key=lambda kv: -kv[1])[:4]))
            grads = {k: rec["g_%d_%s" % (s, k)] for k in p}
            _, st = R.adam_step(cur, grads, LR, st, dtype)
            cur = {k: rec["n_%d_%s" % (s, k)] for k in p}
        worst[dtype] = w
    e_inf = R.relerr(R.infer(cur, rec["inf_seq"], rec["inf_tm"], rec["inf_items"], H), rec["inf_logits"])
    return worst[np.float64], worst[np.float32], e_inf


def synth(path, seed=11):
    """A ratings file in the reference's format: 12 users over 16 items with 5 .. 14 events each (sequence lengths below
    and above the reader case's maxlen 8), times in a per-user unit of 1 .. 5 x 60 seconds (the per-user time_scale) with
    repeated times and gaps far past time_span 6; every third user writes 3-column lines; user 13 has 5 lines of which 3
    name items nobody else has (dropped by the item filter: fewer than 3 events left); user 14 has 4 lines (dropped by the
    user filter)."""
    rng = np.random.default_rng(seed)
    lines = []
    for u in range(1, 13):
        n = int(rng.integers(5, 15))
        items = rng.permutation(16)[:n] + 1
        unit = 60 * int(rng.integers(1, 6))
        gaps = rng.integers(0, 4, n) * unit
        gaps[rng.integers(0, n)] = 40 * unit
        times = 978300000 + int(rng.integers(0, 5000)) + np.cumsum(gaps)
        order = rng.permutation(n)                    # the file is not sorted by time
        for j in order:
            cols = [u, int(items[j]), int(times[j])] if u % 3 == 0 else [u, int(items[j]), int(rng.integers(1, 6)), int(times[j])]
            lines.append("\t".join(str(c) for c in cols))
    for j, it in enumerate((1, 2, 101, 102, 103)):
        lines.append("13\t%d\t3\t%d" % (it, 978400000 + 100 * j))
    for j, it in enumerate((3, 4, 5, 6)):
        lines.append("14\t%d\t4\t%d" % (it, 978500000 + 77 * j))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


def golden_reader():
    _patch_shim()
    mod = load_ref_module(BASE + "/movielens_reader.py", "ref_tisas_reader")
    with open(os.path.join(REF, BASE, "data/sample_data/sample_data.txt")) as f:
        text = f.read()
    with open(os.path.join(OUT, "tisas_sample.txt"), "w") as f:
        f.write(text)
    n = synth(os.path.join(OUT, "tisas_synth.txt"))
    out = {}
    for name, fname, maxlen, span, draws in READER_CASES:
        path = os.path.join(OUT, fname)
        for mode in ("train", "test"):
            cfg = {"hyper_parameters.maxlen": maxlen, "hyper_parameters.time_span": span, "runner.mode": mode}
            ds = mod.RecDataset([path], cfg)
            key = "%s_%s_" % (name, mode)
            out[key + "shape"] = np.asarray([maxlen, span, ds.usernum, ds.itemnum, len(ds)], np.int64)
            rows, failed = [], []
            for i in range(draws if mode == "train" else len(ds)):
                try:
                    rows.append(ds[i])
                except IndexError:                    # a test user without a valid item: the reference fails there
                    failed.append(i)
            out[key + "failed"] = np.asarray(failed, np.int64)
            for c, col in enumerate(("seq", "tm", "pos", "neg") if mode == "train" else ("seq", "tm", "items")):
                out[key + col] = np.stack([np.asarray(r[c]) for r in rows]).astype(np.int64)
            print("tisas reader %s/%s: %d users, %d items, len %d, %d samples recorded, failed %s" % (
                name, mode, ds.usernum, ds.itemnum, len(ds), len(rows), failed))
    path = os.path.join(OUT, "tisas_reader.npz")
    np.savez_compressed(path, **out)
    print("tisas_synth.txt: %d lines; -> %s (%d bytes)" % (n, path, os.path.getsize(path)))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_reader()
    for heads in (1, 2):
        rec = golden_model(heads, SEED + heads)
        e64, e32, ei = check_against_ref(rec)
        print("tisas_h%d: tisas_ref float64 err %.3g, float32 err %.3g, infer err %.3g" % (heads, e64, e32, ei))
        assert e64 < 1e-5 and ei < 1e-5
        path = os.path.join(OUT, "tisas_h%d.npz" % heads)
        np.savez_compressed(path, **rec)
        print("tisas_h%d loss=%s keys=%d -> %s (%d bytes)" % (heads, [float(rec["loss_%d" % s][0]) for s in range(STEPS)], len(rec),
                                                              path, os.path.getsize(path)))
