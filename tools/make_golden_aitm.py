#!/usr/bin/env python3
"""Generate the AITM fixtures under tests/golden/ by executing the reference's UNMODIFIED models/multitask/aitm/net.py,
dygraph_model.py and aitm_reader.py over the paddle shim (oracle/paddle_shim), the way tools/make_golden_esm.py pins esmm and
escm2.  Runs only where the reference tree is; the tests use the committed fixtures.

    python tools/make_golden_aitm.py     # rewrites the three fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: everything tools/make_golden_esm.py sets, and
  * nn.Sequential (torch's: its children are named "0", "1", ..., as Paddle's are), nn.Softmax(axis);
  * paddle.flatten, paddle.squeeze, paddle.zeros_like, paddle.no_grad; paddle.io.Dataset;
  * F.binary_cross_entropy as torch's, which clamps the log at -100 and floors p (1 - p) at 1e-12 in the gradient, as Paddle's
    bce_loss kernel does [EXT];
  * nn.Linear honouring bias_attr=False: the shim creates a bias regardless, and with it the fixture would be another model's
    (Attention's three Linears have none: net.py:48-50);
  * paddle.optimizer.Adam passing weight_decay (a float) through as torch's coupled L2, g + weight_decay * w on every
    parameter [EXT: Paddle's Adam(weight_decay=float) is L2Decay]; the patch tools/make_golden_mtl.py installs drops it.

aitm_rand.npz: 5 tables of [7, 3, 14, 3, 4] rows under the names "9", "1", "5", "3", "7" (config order is NOT sorted order),
D 5, dims [12, 7, 32], drop_prob [0, 0, 0], B 7, built through DygraphModel.create_model from a flat config, every parameter
overwritten with seeded normal draws; ids that include 0 and vocab - 1 in every column, a duplicate within a column and a
whole duplicated sample; labels click 0, click 1 / buy 0 and both 1; at least one sample on each side of the hinge in each
step and none within 1e-3 of a tie (asserted); TWO consecutive Adam steps (create_feeds -> forward -> create_loss -> backward
-> step, train_forward's lines).  The seed is the first from SEED0 on at which tests/aitm_ref.py in float32 ALONE passes
helpers.assert_adam_weights_close against the recorded parameters of both steps.
The file: lr, steps, seed, names (the vocabulary's names), p_<key> (the initial state_dict) and per step s: ids_s [B, F],
click_s, buy_s [B], pred_s [B, 2] (pCTR | pCVR), loss_s, g_s_<key> = grad + 1e-6 * w (what the optimizer applies; every
table's dense gradient included), n_s_<key>.
aitm_sample.txt: the first 1 + LINES lines (the header and LINES samples) of aitm/data/sample_data/train/train.csv;
aitm_reader.npz: what the reference reader yields for them."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from make_golden_esm import _patch_shim as _patch_esm        # noqa: E402
from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

SEED0, LINES, STEPS = 51, 12, 2
RAND = dict(vocab=[["9", 7], ["1", 3], ["5", 14], ["3", 3], ["7", 4]], D=5, dims=[12, 7, 32], drop=[0.0, 0.0, 0.0], B=7,
            lr=0.001, l2=1e-6)


def _patch_shim():
    paddle = _patch_esm()
    import paddle.nn as nn
    import paddle.nn.functional as F
    nn.Sequential = torch.nn.Sequential
    nn.Softmax = lambda axis=-1: torch.nn.Softmax(dim=axis)
    paddle.flatten = lambda x, start_axis=0, stop_axis=-1: torch.flatten(x, start_axis, stop_axis)
    paddle.squeeze = lambda x, axis=None: x.squeeze() if axis is None else x.squeeze(axis)
    paddle.zeros_like = torch.zeros_like
    paddle.no_grad = torch.no_grad
    F.binary_cross_entropy = torch.nn.functional.binary_cross_entropy
    sys.modules["paddle.io"].Dataset = object
    paddle.optimizer.Adam = lambda learning_rate=0.001, parameters=None, weight_decay=None, **kw: torch.optim.Adam(
        list(parameters), lr=learning_rate, weight_decay=float(weight_decay or 0.0))
    if not getattr(nn.Linear, "_honours_no_bias", False):
        base = nn.Linear

        class Linear(base):
            _honours_no_bias = True

            def __init__(self, in_features, out_features, weight_attr=None, bias_attr=None, name=None):
                super().__init__(in_features, out_features, weight_attr, None if bias_attr is False else bias_attr, name)
                if bias_attr is False:
                    del self.bias
                    self.bias = None

            def forward(self, x):
                y = torch.matmul(x, self.weight)
                return y if self.bias is None else y + self.bias

        nn.Linear = Linear
    return paddle


def _load():
    _patch_shim()
    net = load_ref_module("models/multitask/aitm/net.py", "ref_aitm_net")
    sys.modules["net"] = net                         # dygraph_model.py: `import net`
    dm = load_ref_module("models/multitask/aitm/dygraph_model.py", "ref_aitm_dygraph").DygraphModel()
    return net, dm


def _batch(rng):
    B, sizes = RAND["B"], [n for _, n in RAND["vocab"]]
    ids = np.stack([rng.integers(0, n, B) for n in sizes], 1).astype(np.int64)
    ids[0, :] = 0                                    # id 0 is an ordinary row
    ids[1, :] = [n - 1 for n in sizes]               # the last row of every table
    ids[3, 2] = ids[2, 2]                            # a duplicate within a column
    ids[5, :] = ids[4, :]                            # ... and a whole duplicated sample
    click = rng.integers(0, 2, B).astype(np.int64)
    buy = (click & rng.integers(0, 2, B)).astype(np.int64)
    click[:3], buy[:3] = (0, 1, 1), (0, 0, 1)
    return ids, click, buy


def golden_rand(seed):
    _, dm = _load()
    r = RAND
    rng = np.random.default_rng(seed)
    cfg = {"hyper_parameters.feature_vocabulary": r["vocab"], "hyper_parameters.embedding_size": r["D"],
           "hyper_parameters.dims": r["dims"], "hyper_parameters.drop_prob": r["drop"],
           "hyper_parameters.optimizer.learning_rate": r["lr"]}
    m = dm.create_model(cfg)
    assert not any(k.startswith("attention_layer.") and k.endswith(".bias") for k in m.state_dict())
    with torch.no_grad():
        for _, q in sorted(m.named_parameters()):
            q.copy_(torch.as_tensor((0.5 if q.dim() == 2 else 0.2) * rng.standard_normal(tuple(q.shape)), dtype=torch.float32))
    opt = dm.create_optimizer(m, cfg)
    assert opt.defaults["weight_decay"] == r["l2"]
    rec = dict(lr=np.asarray([r["lr"]], np.float64), steps=np.asarray([STEPS], np.int64), seed=np.asarray([seed], np.int64),
               names=np.asarray([n for n, _ in r["vocab"]]))
    for k, v in m.state_dict().items():
        rec["p_" + k] = npy(v)
    for s in range(STEPS):
        ids, click, buy = _batch(rng)
        batch = [torch.from_numpy(click), torch.from_numpy(buy),
                 [torch.from_numpy(ids[:, f].copy()) for f in range(ids.shape[1])]]       # what the DataLoader collates
        c, v, feats = dm.create_feeds(batch, cfg)
        pc, pv = m.forward(feats)
        loss = dm.create_loss(pc, pv, c, v)
        loss.backward()
        gap = npy(pv) - npy(pc)
        if not ((gap > 1e-3).any() and (gap < -1e-3).any() and (np.abs(gap) > 1e-3).all()):
            return None                              # the hinge needs both sides, away from a tie
        rec["ids_%d" % s], rec["click_%d" % s], rec["buy_%d" % s] = ids, click, buy
        rec["pred_%d" % s] = np.stack([npy(pc), npy(pv)], 1)
        rec["loss_%d" % s] = npy(loss).reshape(1)
        for k, q in m.named_parameters():
            rec["g_%d_%s" % (s, k)] = npy(q.grad) + np.float32(r["l2"]) * npy(q)
        opt.step()
        opt.zero_grad(set_to_none=True)
        for k, q in m.state_dict().items():
            rec["n_%d_%s" % (s, k)] = npy(q)
    return rec


def check_against_ref(rec):
    """-> (worst float64 error over predictions / loss / gradients, worst float32 error, whether the float32 restatement
    alone passes the Adam-weights check against the recorded parameters of every step).  Each step is evaluated from the
    RECORDED state: the parameters the step before left and Adam's moments of the recorded gradients."""
    import aitm_ref as R
    from helpers import assert_adam_weights_close
    p = {k[2:]: rec[k] for k in rec if k.startswith("p_")}
    lr = float(rec["lr"][0])
    worst, ok = {np.float64: 0.0, np.float32: 0.0}, True
    cur, st = p, None
    for s in range(int(rec["steps"][0])):
        grads = {k[len("g_%d_" % s):]: rec[k] for k in rec if k.startswith("g_%d_" % s)}
        for dtype in (np.float64, np.float32):
            c, g, new, _ = R.train_step(cur, rec["ids_%d" % s], rec["click_%d" % s], rec["buy_%d" % s], lr, st, dtype=dtype)
            assert sorted(g) == sorted(grads), sorted(set(g) ^ set(grads))
            pairs = [(c["pred"], rec["pred_%d" % s]), (c["loss"], rec["loss_%d" % s])] + [(g[k], grads[k]) for k in g]
            worst[dtype] = max([worst[dtype]] + [R.relerr(a, b) for a, b in pairs])
            if dtype is np.float32:
                for k in p:
                    try:
                        assert_adam_weights_close(new[k], rec["n_%d_%s" % (s, k)], lr, 1, err_msg="step %d %s" % (s, k))
                    except AssertionError as e:
                        ok = False
                        print("  seed rejected:", str(e)[:160])
                        break
        _, st = R.adam_step(cur, grads, lr, st)
        cur = {k: rec["n_%d_%s" % (s, k)] for k in p}
    return worst[np.float64], worst[np.float32], ok


def golden_reader(sample):
    _patch_shim()
    with open(os.path.join(REF, "models/multitask/aitm/data/sample_data/train/train.csv")) as f:
        lines = f.readlines()[:1 + LINES]
    with open(sample, "w") as o:
        o.writelines(lines)
    rd = load_ref_module("models/multitask/aitm/aitm_reader.py", "ref_aitm_reader")
    ds = rd.RecDataset([sample, "/nonexistent/second/file"], {})              # only file_list[0] is read
    rows = [ds[i] for i in range(len(ds))]
    out = dict(ids=np.asarray([r[2] for r in rows], np.int64), click=np.asarray([r[0] for r in rows], np.int64),
               buy=np.asarray([r[1] for r in rows], np.int64), names=np.asarray(ds.feature_names))
    assert out["ids"].shape == (LINES, 18) and out["click"].shape == (LINES,)
    path = os.path.join(OUT, "aitm_reader.npz")
    np.savez_compressed(path, **out)
    print("aitm reader: %d lines -> %s (%d bytes; sample %d bytes)" % (LINES, path, os.path.getsize(path), os.path.getsize(sample)))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_reader(os.path.join(OUT, "aitm_sample.txt"))
    for seed in range(SEED0, SEED0 + 400):
        rec = golden_rand(seed)
        if rec is None:
            print("aitm_rand seed %d: the hinge does not have both sides away from a tie" % seed)
            continue
        e64, e32, ok = check_against_ref(rec)
        print("aitm_rand seed %d: aitm_ref float64 err %.3g, float32 err %.3g, float32 Adam check %s" % (seed, e64, e32, ok))
        if ok:
            break
    else:
        raise SystemExit("no seed passed")
    path = os.path.join(OUT, "aitm_rand.npz")
    np.savez_compressed(path, **rec)
    print("aitm_rand loss=%s keys=%d -> %s (%d bytes)" % ([float(rec["loss_%d" % s][0]) for s in range(STEPS)], len(rec), path,
                                                         os.path.getsize(path)))
