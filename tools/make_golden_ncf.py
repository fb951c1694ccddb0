#!/usr/bin/env python3
"""Generate tests/golden/ncf_neumf.npz, ncf_gmf.npz, ncf_mlp.npz, ncf_sample.txt and ncf_reader.npz by executing the
reference's UNMODIFIED models/recall/ncf/net.py, dygraph_model.py and movielens_reader.py over the paddle shim
(oracle/paddle_shim), the way tools/make_golden_ensfm.py pins recall/ensfm.  Runs only where the reference tree is
(PADDLEREC_REF); the tests use the committed fixtures.

    python tools/make_golden_ncf.py     # rewrites the five fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: paddle.flatten (torch's),
nn.initializer.KaimingUniform (uniform within sqrt(6 / fan_in); every parameter is overwritten afterwards),
paddle.io.IterableDataset, and optimizer.Adam (torch's Adam with epsilon 1e-8, which is Paddle's rule: lr_t = lr sqrt(1 -
b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + eps sqrt(1 - b2^t)) is the same expression).  The shim's Embedding is dense
(weight[ids]), its TruncatedNormal, L2Decay and log_loss (epsilon 1e-4) exist.  That these equal Paddle's rests on Paddle's
documentation: the tool runs on torch, not on Paddle.

ncf_*.npz: the layer of that mode built through DygraphModel.create_model with num_users 7, num_items 9, fc_layers
[8, 6, 5, 2] and mf_dim 3 (NeuMF) or 2 (GMF, MLP: the reference sizes `prediction` by fc_layers[3]).  Two consecutive Adam
steps (lr 0.001) on two batches of B 6, each holding one user three times, one item twice and both labels.  Every
parameter is overwritten with seeded draws of order 0.3.  Recorded: the feeds (`users_s`, `items_s`, `labels_s`), the
starting state_dict (`p_*`), per step `loss_s`, `pred_s`, every gradient (`g_s_*`, tables dense), the parameters (`n_s_*`)
and both moments (`m_s_*`, `v_s_*`) after the step, and one infer call on the final parameters (`inf_users`, `inf_items`,
`inf_pred`).  The seed is the first from SEED0 on at which tests/ncf_ref.py in float32 ALONE passes the bounds of
tests/ncf_checks.py against its float64 self and against the recording, and at which the recording itself meets them
against ncf_ref in float64; asserted here.
ncf_sample.txt: the reference's 100-line sample file (data; its train and test directories hold the same file).
ncf_reader.npz: what the reference reader yields for it.
"""
import math
import os
import shutil
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

U, I, B, LAYERS, SEED0, LR, STEPS = 7, 9, 6, [8, 6, 5, 2], 11, 0.001, 2
NETS = (("ncf_neumf.npz", "NCF_NeuMF", 3), ("ncf_gmf.npz", "NCF_GMF", 2), ("ncf_mlp.npz", "NCF_MLP", 2))


def _patch_shim():
    import paddle  # the shim
    import paddle.nn.initializer as init
    paddle.flatten = lambda x, start_axis=0, stop_axis=-1: torch.flatten(x, start_axis, stop_axis)

    class KaimingUniform:
        def __init__(self, fan_in=None):
            self.fan_in = fan_in

        def __call__(self, p):
            p.uniform_(-1.0, 1.0).mul_(math.sqrt(6.0 / (self.fan_in or p.shape[0])))
    init.KaimingUniform = KaimingUniform
    opt = types.ModuleType("paddle.optimizer")
    opt.Adam = lambda learning_rate, parameters: torch.optim.Adam(list(parameters), lr=learning_rate, betas=(0.9, 0.999), eps=1e-8)
    paddle.optimizer = opt
    io = types.ModuleType("paddle.io")
    io.IterableDataset = type("IterableDataset", (), {"__init__": lambda self: None})
    sys.modules["paddle.io"] = paddle.io = io
    return paddle


class _Cfg(dict):
    pass


def _feeds(rng):
    out = {}
    for s in range(STEPS):
        u, i = rng.integers(0, U, B), rng.integers(0, I, B)
        u[[0, 2, 5]] = u[0]                                  # one user three times
        i[[1, 4]] = i[1]                                     # one item twice
        y = rng.integers(0, 2, B)
        y[0], y[1] = 1, 0                                    # both labels
        out["users_%d" % s], out["items_%d" % s], out["labels_%d" % s] = u, i, y
    out["inf_users"], out["inf_items"] = rng.integers(0, U, 5), rng.integers(0, I, 5)
    return {k: np.ascontiguousarray(v, np.int64) for k, v in out.items()}


def golden_ncf(mode, mf_dim, seed):
    _patch_shim()
    torch.set_num_threads(1)                                 # the CPU embedding backward sums duplicate rows in thread order
    net = load_ref_module("models/recall/ncf/net.py", "ref_ncf_net")
    sys.modules["net"] = net                                 # dygraph_model.py: `import net`
    dm = load_ref_module("models/recall/ncf/dygraph_model.py", "ref_ncf_dygraph").DygraphModel()
    cfg = {"hyper_parameters.num_users": U, "hyper_parameters.num_items": I, "hyper_parameters.mf_dim": mf_dim,
           "hyper_parameters.mode": mode, "hyper_parameters.fc_layers": LAYERS, "hyper_parameters.optimizer.learning_rate": LR}
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = dm.create_model(cfg)
    with torch.no_grad():
        for v in model.state_dict().values():
            v.copy_(torch.as_tensor(0.3 * rng.standard_normal(tuple(v.shape)), dtype=torch.float32))
    feeds = _feeds(rng)
    rec = dict(seed=np.asarray([seed], np.int64), lr=np.asarray([LR], np.float64), steps=np.asarray([STEPS], np.int64),
               mode=np.asarray([mode]), mf_dim=np.asarray([mf_dim], np.int64), layers=np.asarray(LAYERS, np.int64),
               num_users=np.asarray([U], np.int64), num_items=np.asarray([I], np.int64), **feeds)
    for k, v in model.state_dict().items():
        rec["p_" + k] = npy(v)
    opt = dm.create_optimizer(model, cfg)
    assert set(k for k, _ in model.named_parameters()) == set(model.state_dict().keys())
    t = torch.from_numpy
    for s in range(STEPS):
        batch = [t(feeds["%s_%d" % (k, s)]) for k in ("users", "items", "labels")]
        opt.zero_grad()
        loss, _, printed = dm.train_forward(model, [], batch, cfg)
        inputs = dm.create_feeds(batch)
        pred = model.forward(inputs)
        assert pred.shape == (B, 1) and float(dm.create_loss(pred, inputs[2])) == float(loss)
        loss.backward()
        rec["pred_%d" % s], rec["loss_%d" % s] = npy(pred).reshape(-1), npy(loss).reshape(1)
        for k, v in model.named_parameters():
            rec["g_%d_%s" % (s, k)] = npy(v.grad)
        opt.step()
        for k, v in model.named_parameters():
            rec["n_%d_%s" % (s, k)] = npy(v)
            rec["m_%d_%s" % (s, k)], rec["v_%d_%s" % (s, k)] = npy(opt.state[v]["exp_avg"]), npy(opt.state[v]["exp_avg_sq"])
    with torch.no_grad():
        _, out = dm.infer_forward(model, [], [t(feeds["inf_users"]), t(feeds["inf_items"]), t(np.zeros(5, np.int64))], cfg)
    rec["inf_pred"] = npy(out["prediction"]).reshape(-1)
    return rec


def check_against_ref(name):
    """Whether the float32 restatement alone, and the recording, pass tests/ncf_checks.py's bounds on this recording."""
    import ncf_checks as K
    K.gold.cache_clear()
    G = K.gold(name)
    try:
        K.check_golden(G)                                    # the recording against ncf_ref float64
        for s in range(G["steps"]):                          # ncf_ref float32 ALONE against its float64 self ...
            K.check_step(G["r64"][s], G["r32"][s], G["lr"], s, G["r32"][s], "float32")
            rec = K.recorded_step(G, s)                      # ... and against the recording
            for k in G["p"]:
                K.assert_adam_weights_close(G["r32"][s]["n"][k], rec["n"][k], G["lr"], 1, err_msg=k)
                K.assert_close_scaled(G["r32"][s]["m"][k], rec["m"][k], 1e-5, err_msg="m " + k)
                K.assert_close_scaled(G["r32"][s]["v"][k], rec["v"][k], 1e-5, err_msg="v " + k)
    except AssertionError as e:
        print("  seed rejected:", str(e)[:200])
        return False
    return True


def golden_reader():
    _patch_shim()
    src = os.path.join(REF, "models/recall/ncf/data/train")
    (name,) = sorted(os.listdir(src))
    with open(os.path.join(src, name), "rb") as a, open(os.path.join(REF, "models/recall/ncf/data/test", name), "rb") as b:
        assert a.read() == b.read()
    shutil.copyfile(os.path.join(src, name), os.path.join(OUT, "ncf_sample.txt"))
    rd = load_ref_module("models/recall/ncf/movielens_reader.py", "ref_ncf_reader")
    rows = list(rd.RecDataset([os.path.join(OUT, "ncf_sample.txt")], None))
    out = {k: np.concatenate([r[c] for r in rows]).astype(np.int64) for c, k in enumerate(("users", "items", "labels"))}
    path = os.path.join(OUT, "ncf_reader.npz")
    np.savez_compressed(path, **out)
    print("ncf reader: %d lines -> %s (%d bytes)" % (len(rows), path, os.path.getsize(path)))


if __name__ == "__main__":
    for fname, mode, mf_dim in NETS:
        path = os.path.join(OUT, fname)
        for seed in range(SEED0, SEED0 + 400):
            rec = golden_ncf(mode, mf_dim, seed)
            np.savez_compressed(path, **rec)
            ok = check_against_ref(fname)
            print("%s seed %d: %s" % (fname, seed, "ok" if ok else "rejected"))
            if ok:
                break
        else:
            raise SystemExit("no seed passed")
        assert ok
        print("%s loss0=%.6f loss1=%.6f keys=%d -> %s (%d bytes)" % (fname, float(rec["loss_0"][0]), float(rec["loss_1"][0]),
                                                                     len(rec), path, os.path.getsize(path)))
    golden_reader()
