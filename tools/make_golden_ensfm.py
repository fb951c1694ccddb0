#!/usr/bin/env python3
"""Generate tests/golden/ensfm_rand.npz, ensfm_train_sample.csv, ensfm_test_sample.csv and ensfm_reader.npz by executing the
reference's UNMODIFIED models/recall/ensfm/net.py, dygraph_model.py and movielens_reader.py over the paddle shim
(oracle/paddle_shim), the way tools/make_golden_bst.py pins rank/bst.  Runs only where the reference tree is (PADDLEREC_REF);
the tests use the committed fixtures.

    python tools/make_golden_ensfm.py     # rewrites the four fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: paddle.einsum (torch's), paddle.ones,
paddle.get_default_dtype ("float32"), paddle.nn.functional.embedding (weight[ids]), paddle.to_tensor of a nested list as
float32, paddle.io.Dataset, and optimizer.Adagrad (torch's Adagrad with epsilon 1e-6: acc += g^2; p -= lr g / (sqrt(acc) +
eps), the accumulator starting at initial_accumulator_value).  That these equal Paddle's rests on Paddle's documentation:
the tool runs on torch, not on Paddle.

ensfm_rand.npz: ENSFMLayer built through DygraphModel.create_model with num_users 10, num_items 11 (tables of 10, 12, 10 and
11 rows), mf_dim 5; B 4, Fu 3, Fi 2, I 6, P 5, negative_weight 0.4, lr 0.05.  Batch 0: user 0 has an all-padding list, user 1 a
full one, user 2 the same item twice, user 3 item 0; user row 1 and item row 2 hold the same feature id twice; row I of the
item attributes is item 0's, as the reader builds it.  Every tensor is overwritten with seeded draws of order 0.3 (the
shipped initialisation, 0.01, leaves the gradients near Adagrad's 1e-4 knee, sqrt(initial accumulator)).  Recorded: two
consecutive Adagrad steps on two batches — the feeds (`u_s`, `ur_s`, `attr`), the starting state_dict (`p_*`), per step
`loss_s`, `pre_s`, `pos_r_s`, `q_emb_s`, `p_emb_s`, every gradient (`g_s_*`, tables dense), the parameters (`n_s_*`) and the
accumulators (`a_s_*`) after the step — and one infer call on the final parameters (`inf_u`, `inf_pre`).  The seed is the
first from SEED0 on at which tests/ensfm_ref.py in float32 ALONE passes the post-step parameter bound of
tests/ensfm_checks.py against both its float64 self and the recorded `n_*`, and at which the recording itself (the
reference in float32) meets the per-tensor rule of tests/ensfm_checks.py against ensfm_ref in float64 — the loss is a sum of
terms of both signs, and a draw where it nearly cancels would put a float32 recording outside a bound that is relative to
the loss's own magnitude; asserted here.
ensfm_train_sample.csv / ensfm_test_sample.csv: the reference's 100-line sample files (data).  ensfm_reader.npz: what the
reference reader yields for them in both modes, and the non-zeros of its Train_data / Test_data.
"""
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

B, FU, FI, D, I, P, SEED0, LR, W, STEPS = 4, 3, 2, 5, 6, 5, 11, 0.05, 0.4, 2
CFG = {"hyper_parameters.num_users": 10, "hyper_parameters.num_items": 11, "hyper_parameters.mf_dim": D,
       "hyper_parameters.negative_weight": W, "hyper_parameters.optimizer.class": "adagrad",
       "hyper_parameters.optimizer.learning_rate": LR}


def _patch_shim():
    import paddle  # the shim
    import paddle.nn.functional as F
    paddle.einsum = torch.einsum
    paddle.ones = lambda shape, dtype=None: torch.ones(list(shape), dtype=torch.float32)
    paddle.get_default_dtype = lambda: "float32"
    F.embedding = lambda x, weight, padding_idx=None, sparse=False: weight[x]
    base = paddle.to_tensor
    if not getattr(base, "_ensfm", False):
        def to_tensor(x, dtype=None):
            if isinstance(x, list):                      # paddle.to_tensor([[1.0]]) is float32, the default dtype
                return torch.tensor(x, dtype=torch.float32)
            return base(x, dtype)
        to_tensor._ensfm = True
        paddle.to_tensor = to_tensor
    opt = types.ModuleType("paddle.optimizer")
    opt.Adagrad = lambda learning_rate, parameters, epsilon=1e-6, initial_accumulator_value=0.0: torch.optim.Adagrad(
        list(parameters), lr=learning_rate, eps=epsilon, initial_accumulator_value=initial_accumulator_value)
    paddle.optimizer = opt
    io = types.ModuleType("paddle.io")
    io.Dataset = object
    sys.modules["paddle.io"] = paddle.io = io
    return paddle


def _feeds(rng):
    attr = rng.integers(0, CFG["hyper_parameters.num_items"], (I + 1, FI))
    attr[2] = attr[2, 0]                                     # one item row with the same feature id twice
    attr[I] = attr[0]                                        # movielens_reader.py:66-68
    out = dict(attr=attr)
    for s in range(STEPS):
        u = rng.integers(0, CFG["hyper_parameters.num_users"], (B, FU))
        u[1, 2] = u[1, 0]                                    # one user row with the same feature id twice
        ur = np.full((B, P), I)
        for b in range(B):
            n = int(rng.integers(1, P))
            ur[b, :n] = rng.choice(I, n, replace=False)
        if s == 0:
            ur[0] = I                                        # an all-padding list
            ur[1] = rng.choice(I, P, replace=False)          # a full list
            ur[2, :3] = (4, 2, 4)                            # the same item twice
            ur[3, :2] = (0, 5)                               # item 0, whose features the padding row copies
        out["u_%d" % s], out["ur_%d" % s] = u, ur
    return {k: np.ascontiguousarray(v, np.int64) for k, v in out.items()}


def golden_ensfm(seed):
    _patch_shim()
    torch.set_num_threads(1)                                 # the CPU embedding backward sums duplicate rows in thread order
    net = load_ref_module("models/recall/ensfm/net.py", "ref_ensfm_net")
    sys.modules["net"] = net                                 # dygraph_model.py: `import net`
    dm = load_ref_module("models/recall/ensfm/dygraph_model.py", "ref_ensfm_dygraph").DygraphModel()
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = dm.create_model(CFG)
    with torch.no_grad():
        for v in model.state_dict().values():
            v.copy_(torch.as_tensor(0.3 * rng.standard_normal(tuple(v.shape)), dtype=torch.float32))
    feeds = _feeds(rng)
    rec = dict(seed=np.asarray([seed], np.int64), lr=np.asarray([LR], np.float64), w=np.asarray([W], np.float64),
               steps=np.asarray([STEPS], np.int64), **feeds)
    for k, v in model.state_dict().items():
        rec["p_" + k] = npy(v)
    opt = dm.create_optimizer(model, CFG)
    assert set(k for k, _ in model.named_parameters()) == set(model.state_dict().keys())
    t = torch.from_numpy
    for s in range(STEPS):
        # the DataLoader stacks the per-sample copies of the attributes and of item_bind_M; create_feeds takes copy 0
        batch = [t(feeds["u_%d" % s]), t(np.stack([feeds["attr"]] * B)), t(feeds["ur_%d" % s]), t(np.full((B,), I, np.int64))]
        opt.zero_grad()
        pred = model.forward(*dm.create_feeds(batch))
        loss = dm.create_loss(pred, CFG)
        loss.backward()
        for name, v in zip(("pre", "pos_r", "q_emb", "p_emb"), pred):
            rec["%s_%d" % (name, s)] = npy(v)
        rec["loss_%d" % s] = npy(loss).reshape(1)
        for k, v in model.named_parameters():
            rec["g_%d_%s" % (s, k)] = npy(v.grad)
        opt.step()
        for k, v in model.named_parameters():
            rec["n_%d_%s" % (s, k)] = npy(v)
            rec["a_%d_%s" % (s, k)] = npy(opt.state[v]["sum"])
    rec["inf_u"] = np.ascontiguousarray(rng.integers(0, CFG["hyper_parameters.num_users"], (3, FU)), np.int64)
    with torch.no_grad():
        out = model.forward(*dm.create_feeds([t(rec["inf_u"]), t(np.stack([feeds["attr"]] * 3))]))
    assert len(out) == 1
    rec["inf_pre"] = npy(out[0])
    return rec


def check_against_ref(path):
    """-> (worst float64 error over the recorded arrays, worst float32 error, whether the float32 restatement alone passes the
    post-step parameter bound against its float64 self and the recording)."""
    import ensfm_checks as K
    import ensfm_ref as R
    K.gold.cache_clear()
    G = K.gold(os.path.basename(path))
    worst = [0.0, 0.0]
    ok = True
    for s in range(G["steps"]):
        for i, r in enumerate((G["r64"][s], G["r32"][s])):
            errs = [R.relerr(r[k], G["g"]["%s_%d" % (k, s)]) for k in R.FWD]
            errs += [R.relerr(r["g"][k], G["g"]["g_%d_%s" % (s, k)]) for k in R.PARAMS]
            worst[i] = max(worst[i], max(errs))
        for k in R.PARAMS:
            for got in (G["r32"][s]["n"][k], G["g"]["n_%d_%s" % (s, k)]):
                try:
                    K.assert_adagrad_weights_close(got, G["r64"][s]["n"][k], G["lr"], 1, err_msg=k)
                except AssertionError as e:
                    ok = False
                    print("  seed rejected:", str(e)[:160])
    try:
        K.check_golden(G)
    except AssertionError as e:
        ok = False
        print("  seed rejected: the float32 recording misses the per-tensor rule:", str(e)[:120])
    return worst[0], worst[1], ok


def golden_reader():
    _patch_shim()
    src = os.path.join(REF, "models/recall/ensfm/data/sample_data")
    for name in ("train", "test"):
        shutil.copyfile(os.path.join(src, name + ".csv"), os.path.join(OUT, "ensfm_%s_sample.csv" % name))
    rd = load_ref_module("models/recall/ensfm/movielens_reader.py", "ref_ensfm_reader")
    out = {}
    for mode in ("train", "test"):
        ds = rd.RecDataset([os.path.join(src, "train.csv")], {"runner.mode": mode})
        rows = [ds[i] for i in range(len(ds))]
        names = ("user_train", "item_map_list", "item_train", "item_bind_M") if mode == "train" else ("user_test", "item_map_list_test")
        for c, name in enumerate(names):
            col = [np.asarray(r[c]) for r in rows]
            assert all((x == col[0]).all() for x in col) or "map" not in name and "bind" not in name
            out[name] = np.asarray(col[0] if "map" in name or "bind" in name else np.stack(col), np.int64)
    d = ds.data
    out["train_pairs"] = np.stack(d.Train_data.nonzero(), 1).astype(np.int64)
    out["test_pairs"] = np.stack(d.Test_data.nonzero(), 1).astype(np.int64)
    out["sizes"] = np.asarray([d.user_field_M, d.item_field_M, d.user_bind_M, d.item_bind_M, d.max_positive_len], np.int64)
    path = os.path.join(OUT, "ensfm_reader.npz")
    np.savez_compressed(path, **out)
    print("ensfm reader: %d train users, %d test lines, I %d, P %d -> %s (%d bytes)"
          % (len(out["user_train"]), len(out["user_test"]), d.item_bind_M, d.max_positive_len, path, os.path.getsize(path)))


if __name__ == "__main__":
    path = os.path.join(OUT, "ensfm_rand.npz")
    for seed in range(SEED0, SEED0 + 400):
        rec = golden_ensfm(seed)
        np.savez_compressed(path, **rec)
        e64, e32, ok = check_against_ref(path)
        print("ensfm_rand seed %d: ensfm_ref float64 err %.3g, float32 err %.3g, float32 post-step check %s" % (seed, e64, e32, ok))
        if ok:
            break
    else:
        raise SystemExit("no seed passed")
    assert ok and e64 < 1e-5
    print("ensfm_rand loss0=%.6f loss1=%.6f keys=%d -> %s (%d bytes)" % (float(rec["loss_0"][0]), float(rec["loss_1"][0]), len(rec),
                                                                          path, os.path.getsize(path)))
    golden_reader()
