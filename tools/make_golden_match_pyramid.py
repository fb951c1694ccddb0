#!/usr/bin/env python3
"""Generate tests/golden/match_pyramid_relu.npz, match_pyramid_lin.npz, match_pyramid_sample_train.txt.gz and
match_pyramid_reader.npz by executing the reference's UNMODIFIED models/match/match-pyramid/net.py, dygraph_model.py and
letor_reader.py over the paddle shim (oracle/paddle_shim), the way tools/make_golden_dssm.py pins match/dssm.  Runs only where
the reference tree is (PADDLEREC_REF); the tests use the committed fixtures.

    python tools/make_golden_match_pyramid.py     # rewrites the four fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: nn.Conv2D with stride and padding="SAME",
F.relu, F.max_pool2d (padding "VALID"), paddle.full, paddle.subtract, paddle.maximum, paddle.slice, paddle.io.IterableDataset
and optimizer.Adam (torch's Adam with epsilon 1e-8, which is Paddle's rule written differently).  THREE Paddle rules rest on
memory of its documentation and source and not on a Paddle run — the tool runs on torch:
  * "SAME" pads k - 1 per axis, floor((k - 1) / 2) in front and the rest behind (an even filter pads more behind);
  * a pool window's FIRST maximum in row-major order takes the gradient (torch's CPU max_pool2d does the same; the tool asserts
    that no window of a recording ties at a positive value, so the recording does not depend on it);
  * maximum(0, x) passes the gradient at x == 0 (torch splits it in halves; the tool asserts that no hinge term of a recording
    is exactly 0, so the recording does not depend on it).

match_pyramid_*.npz: the layer built through DygraphModel.create_model with vocab_size 193368, emb_size 6, kernel_num 8,
conv_filter [2, 4], pool_size = pool_stride [2, 2], hidden_size 20, sentence sizes 7 and 21 (PH 3, PW 10: 240 features; image
row 6 and column 20 are never pooled), conv_act "relu" (match_pyramid_relu) or "" (match_pyramid_lin).  Two consecutive Adam
steps (lr 0.001) on two batches of B 128 with ids from {0 .. 39, 193367}; sample 0's left sentence is all padding, sample 1's
right sentence ends in 9 paddings, sample 2's right sentence is all padding.  Every parameter is overwritten with seeded draws;
the conv biases are made NEGATIVE: a cell whose tap footprint is all padding convolves to exactly its channel's bias, so with a
positive bias every window inside a padded stretch would tie at a positive value (harmless — such a cell's gradient reaches only
zero rows — but it would make the no-tie assertion below unsatisfiable with the padded sentences above).
Recorded: `rows` (the table rows the feeds name and the padding row, ascending), the feeds (`left_s`, `right_s`), the starting
state_dict (`p_*`), per step `loss_s`, `pred_s`, every gradient (`g_s_*`), the parameters (`n_s_*`) and both moments (`m_s_*`,
`v_s_*`) after the step, and one infer call on the final parameters (`inf_left`, `inf_right`, `inf_pred`); of the embedding table
only the rows `rows` — asserted here: every other row has a zero gradient and does not move.  The seed is the first from SEED0
on at which tests/match_pyramid_ref.py in float32 ALONE passes the bounds of tests/match_pyramid_checks.py against its float64
self and against the recording, at which the recording itself meets them against the float64 restatement, and at which the two
tie conditions above hold.
match_pyramid_sample_train.txt.gz: the reference's whole 128-line data/train/train.txt (data), gzip-compressed byte for byte
(365 KB of text as 85 KB; tests/match_pyramid_checks.py sample_train() unpacks it).  match_pyramid_reader.npz: what the
reference's reader yields for it.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

V, PAD, E, K, FILTER, POOL, HID, LL, LR, B, SEED0, LR_RATE, STEPS = 193368, 193367, 6, 8, [2, 4], [2, 2], 20, 7, 21, 128, 1, 0.001, 2
NETS = (("match_pyramid_relu.npz", "relu"), ("match_pyramid_lin.npz", ""))
MODEL = "models/match/match-pyramid"


def _patch_shim():
    import paddle  # the shim
    import paddle.nn as nn
    import paddle.nn.functional as F
    tf = torch.nn.functional

    class Conv2D(nn.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
            super().__init__()
            assert stride == 1 and padding == "SAME"
            self.k = tuple(kernel_size)
            self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels, *self.k))
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))

        def forward(self, x):
            (kh, kw) = self.k
            pt, pl = (kh - 1) // 2, (kw - 1) // 2
            return tf.conv2d(tf.pad(x, (pl, kw - 1 - pl, pt, kh - 1 - pt)), self.weight, self.bias)

    def max_pool2d(x, kernel_size, stride, padding):
        assert padding == "VALID"
        return tf.max_pool2d(x, tuple(kernel_size), tuple(stride), 0)

    def slice_(x, axes, starts, ends):
        idx = [slice(None)] * x.dim()
        for a, s, e in zip(axes, starts, ends):
            idx[a] = slice(s, min(e, x.shape[a]))
        return x[tuple(idx)]
    nn.Conv2D, F.relu, F.max_pool2d, paddle.slice = Conv2D, torch.relu, max_pool2d, slice_
    paddle.full = lambda shape, fill_value, dtype=None: torch.full(tuple(shape), float(fill_value), dtype=torch.float32)
    paddle.subtract, paddle.maximum = torch.subtract, torch.maximum
    opt = types.ModuleType("paddle.optimizer")
    opt.Adam = lambda learning_rate, parameters: torch.optim.Adam(list(parameters), lr=learning_rate, betas=(0.9, 0.999), eps=1e-8)
    paddle.optimizer = opt
    io = types.ModuleType("paddle.io")
    io.IterableDataset = type("IterableDataset", (), {"__init__": lambda self: None})
    sys.modules["paddle.io"] = paddle.io = io
    return paddle


def _config(act):
    h = "hyper_parameters."
    return {h + "emb_path": "/nonexistent/embedding.npy", h + "vocab_size": V, h + "emb_size": E, h + "kernel_num": K,
            h + "conv_filter": FILTER, h + "conv_act": act, h + "hidden_size": HID, h + "out_size": 1, h + "pool_size": POOL,
            h + "pool_stride": POOL, h + "pool_padding": "VALID", h + "pool_type": "max", h + "hidden_act": "relu",
            h + "sentence_left_size": LL, h + "sentence_right_size": LR, h + "optimizer.learning_rate": LR_RATE}


def _feeds(rng):
    def batch():
        left, right = rng.integers(0, 40, (B, LL)), rng.integers(0, 40, (B, LR))
        left[rng.random((B, LL)) < 0.1] = PAD
        right[rng.random((B, LR)) < 0.1] = PAD
        left[0] = PAD                                          # a fully padded left sentence ...
        right[1, LR - 9:] = PAD                                # ... a fully padded right tail ...
        right[2] = PAD                                         # ... and a right sentence that is all padding
        return left.astype(np.int64), right.astype(np.int64)
    return [batch() for _ in range(STEPS + 1)]


def golden(act, seed):
    _patch_shim()
    torch.set_num_threads(1)
    net = load_ref_module(MODEL + "/net.py", "ref_mpyr_net")
    sys.modules["net"] = net                                 # dygraph_model.py: `import net`
    dm = load_ref_module(MODEL + "/dygraph_model.py", "ref_mpyr_dygraph").DygraphModel()
    cfg = _config(act)
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = dm.create_model(cfg)
    assert sorted(model.state_dict()) == ["conv.bias", "conv.weight", "emb.weight", "fc1.bias", "fc1.weight", "fc2.bias",
                                          "fc2.weight"]
    feeds = _feeds(rng)
    rows = np.unique(np.concatenate([a.reshape(-1) for f in feeds for a in f] + [np.asarray([PAD])]))
    assert rows[-1] == PAD
    others = np.setdiff1d(np.arange(V), rows)
    with torch.no_grad():
        for name, v in model.state_dict().items():
            scale = 0.5 if name == "emb.weight" else 0.3
            v.copy_(torch.as_tensor(scale * rng.standard_normal(tuple(v.shape)), dtype=torch.float32))
        model.emb.weight[PAD].zero_()
        model.conv.bias.copy_(-model.conv.bias.abs())          # see the docstring: a padded footprint convolves to the bias
    start = npy(model.emb.weight)
    cut = lambda name, a: a[rows] if name == "emb.weight" else a
    rec = dict(seed=np.asarray([seed], np.int64), lr=np.asarray([LR_RATE], np.float64), steps=np.asarray([STEPS], np.int64),
               vocab=np.asarray([V], np.int64), rows=rows, filter=np.asarray(FILTER, np.int64), pool=np.asarray(POOL, np.int64),
               stride=np.asarray(POOL, np.int64), relu=np.asarray([act == "relu"], np.int64), pairs=np.asarray([64], np.int64),
               B=np.asarray([B], np.int64))
    for k, v in model.state_dict().items():
        rec["p_" + k] = cut(k, npy(v))
    opt = dm.create_optimizer(model, cfg)
    t = torch.from_numpy
    ties_ok = True
    for s in range(STEPS):
        left, right = feeds[s]
        rec["left_%d" % s], rec["right_%d" % s] = left, right
        opt.zero_grad()
        loss, _, printed = dm.train_forward(model, [], [t(left), t(right)], cfg)
        with torch.no_grad():
            pred = model.forward(dm.create_feeds([t(left), t(right)], LL, LR))
            assert float(dm.create_loss(pred)) == float(loss)
            terms = 1.0 - pred[:64] + pred[64:128]
            ties_ok &= not bool((terms == 0).any())
            conv = model.conv(model.emb(t(left)).matmul(model.emb(t(right)).transpose(1, 2)).unsqueeze(1))
            conv = torch.relu(conv) if act == "relu" else conv
            win = torch.nn.functional.unfold(conv.reshape(-1, 1, LL, LR), tuple(POOL), stride=tuple(POOL))   # [B K, cells, windows]
            top = win.max(1, keepdim=True).values
            ties_ok &= not bool((((win == top).sum(1, keepdim=True) > 1) & (top > 0)).any())
        loss.backward()
        rec["loss_%d" % s], rec["pred_%d" % s] = npy(loss).reshape(1), npy(pred)
        for k, v in model.named_parameters():
            if k == "emb.weight":
                assert not v.grad[others].any()
            rec["g_%d_%s" % (s, k)] = cut(k, npy(v.grad))
        opt.step()
        assert np.array_equal(npy(model.emb.weight)[others], start[others])
        for k, v in model.named_parameters():
            rec["n_%d_%s" % (s, k)] = cut(k, npy(v))
            rec["m_%d_%s" % (s, k)], rec["v_%d_%s" % (s, k)] = cut(k, npy(opt.state[v]["exp_avg"])), cut(k, npy(opt.state[v]["exp_avg_sq"]))
    rec["inf_left"], rec["inf_right"] = feeds[STEPS]
    with torch.no_grad():
        _, out = dm.infer_forward(model, [], [t(a) for a in feeds[STEPS]], cfg)
    rec["inf_pred"] = npy(out["prediction"])
    return rec, ties_ok


def check_against_ref(name):
    """Whether the float32 restatement alone, and the recording, pass tests/match_pyramid_checks.py's bounds."""
    import match_pyramid_checks as C
    C.gold.cache_clear()
    G = C.gold(name)
    try:
        C.check_golden(G)                                    # the recording against the float64 restatement
        for s in range(G["steps"]):                          # the float32 restatement ALONE against its float64 self ...
            assert np.array_equal(G["r32"][s]["argmax"], G["r64"][s]["argmax"])
            C.check_step(G["r64"][s], G["r32"][s], G["lr"], s, G["r32"][s], "float32")
            rec = C.recorded_step(G, s)                      # ... and against the recording
            for k in G["p"]:
                C.assert_adam_weights_close(G["r32"][s]["n"][k], rec["n"][k], G["lr"], 1, err_msg=k)
                C.assert_close_scaled(G["r32"][s]["m"][k], rec["m"][k], 1e-5, err_msg="m " + k)
                C.assert_close_scaled(G["r32"][s]["v"][k], rec["v"][k], 1e-5, err_msg="v " + k)
    except AssertionError as e:
        print("  seed rejected:", str(e)[:200])
        return False
    return True


def golden_reader():
    import gzip
    import tempfile
    _patch_shim()
    with open(os.path.join(REF, MODEL, "data/train/train.txt"), "rb") as f:
        data = f.read()
    path = os.path.join(OUT, "match_pyramid_sample_train.txt.gz")
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as z:
        z.write(data)
    assert os.path.getsize(path) < (1 << 20) and data.count(b"\n") == 128
    rd = load_ref_module(MODEL + "/letor_reader.py", "ref_mpyr_reader")
    with tempfile.TemporaryDirectory() as tmp:
        plain = os.path.join(tmp, "train.txt")
        with open(plain, "wb") as f:
            f.write(gzip.open(path).read())
        rows = list(rd.RecDataset([plain], None))
    assert len(rows) == 128 and all(len(r) == 2 and r[0].dtype == np.int64 and r[1].dtype == np.int64 for r in rows)
    assert len({len(r[0]) for r in rows}) == 1 and len({len(r[1]) for r in rows}) == 1
    out = os.path.join(OUT, "match_pyramid_reader.npz")
    np.savez_compressed(out, left=np.stack([r[0] for r in rows]), right=np.stack([r[1] for r in rows]))
    print("match-pyramid reader: %d lines -> %s (%d bytes)" % (len(rows), out, os.path.getsize(out)))


if __name__ == "__main__":
    for fname, act in NETS:
        path = os.path.join(OUT, fname)
        for seed in range(SEED0, SEED0 + 400):
            rec, ties_ok = golden(act, seed)
            np.savez_compressed(path, **rec)
            ok = ties_ok and check_against_ref(fname)
            print("%s seed %d: %s%s" % (fname, seed, "ok" if ok else "rejected", "" if ties_ok else " (a tie)"))
            if ok:
                break
        else:
            raise SystemExit("no seed passed")
        print("%s loss0=%.6f loss1=%.6f keys=%d -> %s (%d bytes)" % (fname, float(rec["loss_0"][0]), float(rec["loss_1"][0]),
                                                                     len(rec), path, os.path.getsize(path)))
    golden_reader()
