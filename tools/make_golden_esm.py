#!/usr/bin/env python3
"""Generate the fixtures of the entire-space multitask nets under tests/golden/ by executing the reference's UNMODIFIED
models/multitask/{esmm,escm2}/net.py, dygraph_model.py and esmm_reader.py / escm_reader.py over the paddle shim
(oracle/paddle_shim), the way tools/make_golden_mtl.py pins mmoe and ple.  Runs only where the reference tree is; the tests
use the committed fixtures.

    python tools/make_golden_esm.py     # rewrites the five fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: everything tools/make_golden_mtl.py sets
(F.relu, paddle.slice, paddle.optimizer.Adam = torch's Adam, paddle.metric.Auc, paddle.io.IterableDataset, Tensor.numpy() on
a tensor that carries a gradient, add_sublayer's parameter names, nn.Linear taking initializers directly), and for
escm2/dygraph_model.py paddle.subtract, maximum, full_like, reciprocal, divide and `tensor.stop_gradient = True`, which on a
torch tensor must DETACH (dygraph_model.py:122, 136 put the propensity factor IPS under stop-gradient that way; as a plain
attribute it would be ignored and the gradients would be another model's).  That these equal Paddle's rests on Paddle's
documentation.

esmm_rand.npz (ctr tower [6, 5], cvr tower [7]: unequal depth), escm2_ipw_rand.npz, escm2_dr_rand.npz (3 experts of size 6,
tower 4; 2 / 3 gates as net.py:35-38 decides from the mode; global_w 0.5, counterfactual_w 0.3): sparse_feature_number 61,
D 4, num_field 3, max_len 3, B 7, built through DygraphModel.create_model from a flat config, every parameter overwritten
with seeded normal draws (row 0 of the table back to zero), ids with padding, an all-padding field, duplicates within a
field and across samples; samples with click 0, click 1 / buy 0 and both 1; TWO consecutive Adam steps (create_feeds ->
forward -> create_loss -> backward -> step, train_forward's lines).  The seed is the first from SEED0 on at which
tests/esm_ref.py in float32 ALONE passes helpers.assert_adam_weights_close against the recorded parameters of both steps (the
first Adam steps are sign-like where a gradient is near eps; the fixture must not sit on such a coin flip).
Every file: lr, steps, seed, mode, global_w, counterfactual_w, p_<key> (the initial state_dict) and per step s: ids_s
[B, F, L], click_s, buy_s [B], outs_s [B, 9 or 10] (all of out_list side by side: ctr_out, ctr_prop_one, cvr_out,
cvr_prop_one, ctcvr_prop, ctcvr_prop_one and, in the DR mode, imp_prop_one), loss_s, g_s_<key> (the table's dense [61, 4]
gradient included), n_s_<key>.
aliccp_sample.txt: the first 4 lines of escm2/data/train/small.txt; aliccp_reader.npz: what the reference reader yields."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from make_golden_mtl import _patch_shim as _patch_mtl        # noqa: E402
from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

SEED0, LINES, STEPS = 41, 4, 2
RAND = dict(N=61, D=4, F=3, L=3, B=7, E=3, S=6, T=4, lr=0.001, global_w=0.5, counterfactual_w=0.3)


def _patch_shim():
    paddle = _patch_mtl()
    paddle.subtract = lambda x, y: x - y
    paddle.divide = lambda x, y: x / y
    paddle.maximum = torch.maximum
    paddle.reciprocal = torch.reciprocal
    paddle.full_like = lambda x, fill_value, dtype=None: torch.full_like(x, fill_value)
    if not isinstance(getattr(torch.Tensor, "stop_gradient", None), property):

        def _set(self, value):
            if value:
                self.detach_()

        torch.Tensor.stop_gradient = property(lambda self: not self.requires_grad, _set)
    return paddle


def _load(model):
    _patch_shim()
    net = load_ref_module("models/multitask/%s/net.py" % model, "ref_%s_net" % model)
    sys.modules["net"] = net                         # dygraph_model.py: `import net`
    dm = load_ref_module("models/multitask/%s/dygraph_model.py" % model, "ref_%s_dygraph" % model).DygraphModel()
    return net, dm


def _batch(rng):
    r = RAND
    B, F, L = r["B"], r["F"], r["L"]
    ids = rng.integers(1, r["N"], (B, F, L)).astype(np.int64)
    ids[rng.random((B, F, L)) < 0.25] = 0            # padding, also in front of a real id
    ids[2, 1, :] = 0                                 # an all-padding field
    ids[3, 0, 1] = ids[3, 0, 0] = 17                 # a duplicate within a field
    ids[4, 2, :] = ids[0, 2, :]                      # ... and across samples
    ids[5, 0, 2] = 17
    click = rng.integers(0, 2, B).astype(np.int64)
    buy = (click & rng.integers(0, 2, B)).astype(np.int64)
    click[:3], buy[:3] = (0, 1, 1), (0, 0, 1)
    return ids, click, buy


def golden_rand(model, mode, seed):
    import paddle
    net, dm = _load(model)
    r = RAND
    rng = np.random.default_rng(seed)
    cfg = {"hyper_parameters.sparse_feature_number": r["N"], "hyper_parameters.sparse_feature_dim": r["D"],
           "hyper_parameters.num_field": r["F"], "hyper_parameters.max_len": r["L"], "hyper_parameters.ctr_fc_sizes": [6, 5],
           "hyper_parameters.cvr_fc_sizes": [7], "hyper_parameters.optimizer.learning_rate": r["lr"]}
    gw, cw = 1.0, 0.0
    if model == "escm2":
        gw, cw = r["global_w"], r["counterfactual_w"]
        cfg.update({"hyper_parameters.global_w": gw, "hyper_parameters.counterfactual_w": cw, "hyper_parameters.expert_num": r["E"],
                    "hyper_parameters.expert_size": r["S"], "hyper_parameters.tower_size": r["T"], "hyper_parameters.gate_num": 3,
                    "hyper_parameters.feature_size": r["F"] * r["D"], "runner.counterfact_mode": mode})
    m = dm.create_model(cfg)
    with torch.no_grad():
        for _, q in sorted(m.named_parameters()):
            q.copy_(torch.as_tensor((0.5 if q.dim() == 2 else 0.2) * rng.standard_normal(tuple(q.shape)), dtype=torch.float32))
        m.embedding.weight[0].zero_()
    opt = dm.create_optimizer(m, cfg)
    rec = dict(lr=np.asarray([r["lr"]], np.float64), steps=np.asarray([STEPS], np.int64), seed=np.asarray([seed], np.int64),
               mode=np.asarray([mode]), global_w=np.asarray([gw], np.float64), counterfactual_w=np.asarray([cw], np.float64))
    for k, v in m.state_dict().items():
        rec["p_" + k] = npy(v)
    for s in range(STEPS):
        ids, click, buy = _batch(rng)
        batch = [torch.from_numpy(ids[:, f, :].copy()) for f in range(r["F"])] + \
                [torch.from_numpy(click.reshape(-1, 1)), torch.from_numpy(buy.reshape(-1, 1))]     # what the DataLoader collates
        sparse, label_ctr, label_ctcvr = dm.create_feeds(batch, cfg)
        outs = list(m.forward(sparse))
        if model == "esmm":
            loss = dm.create_loss(outs[1], label_ctr, outs[5], label_ctcvr)
        else:
            loss = dm.create_loss(outs[1], label_ctr, outs[5], label_ctcvr, outs[3], outs)
        loss.backward()
        rec["ids_%d" % s], rec["click_%d" % s], rec["buy_%d" % s] = ids, click, buy
        rec["outs_%d" % s] = np.concatenate([npy(o) for o in outs], 1)
        rec["loss_%d" % s] = npy(loss).reshape(1)
        for k, v in m.named_parameters():
            if v.grad is not None:
                g = v.grad.to_dense() if v.grad.is_sparse else v.grad
                rec["g_%d_%s" % (s, k)] = npy(g)
        opt.step()
        opt.zero_grad(set_to_none=True)
        for k, v in m.state_dict().items():
            rec["n_%d_%s" % (s, k)] = npy(v)
    return rec


def check_against_ref(rec):
    """-> (worst float64 error over outputs / loss / gradients, worst float32 error, whether the float32 restatement alone
    passes the Adam-weights check against the recorded parameters of every step).  Each step is evaluated from the RECORDED
    state: the parameters the step before left and Adam's moments of the recorded gradients."""
    import esm_ref as R
    from helpers import assert_adam_weights_close
    p = {k[2:]: rec[k] for k in rec if k.startswith("p_")}
    lr, cfg = float(rec["lr"][0]), R.cfg_of(rec)
    worst, ok = {np.float64: 0.0, np.float32: 0.0}, True
    cur, st = p, None
    for s in range(int(rec["steps"][0])):
        grads = {k[len("g_%d_" % s):]: rec[k] for k in rec if k.startswith("g_%d_" % s)}
        for dtype in (np.float64, np.float32):
            c, g, new, _ = R.train_step(cur, rec["ids_%d" % s], rec["click_%d" % s], rec["buy_%d" % s], lr, cfg, st, dtype=dtype)
            assert sorted(g) == sorted(grads), sorted(set(g) ^ set(grads))
            pairs = [(R.outs_of(c["pred"]), rec["outs_%d" % s]), (c["loss"], rec["loss_%d" % s])] + [(g[k], grads[k]) for k in g]
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
    with open(os.path.join(REF, "models/multitask/escm2/data/train/small.txt")) as f:
        lines = f.readlines()[:LINES]
    with open(sample, "w") as o:
        o.writelines(lines)
    out = {}
    for model, mod in (("esmm", "esmm_reader"), ("escm2", "escm_reader")):
        rd = load_ref_module("models/multitask/%s/%s.py" % (model, mod), "ref_%s" % mod)
        rows = list(rd.RecDataset([sample], {}))
        got = dict(ids=np.stack([np.stack(r[:-2]) for r in rows]), click=np.concatenate([r[-2] for r in rows]),
                   buy=np.concatenate([r[-1] for r in rows]))
        assert got["ids"].shape == (LINES, 23, 3) and got["ids"].dtype == np.int64 and got["click"].shape == (LINES,)
        assert not out or all(np.array_equal(out[k], got[k]) for k in got)        # the two readers are one
        out = got
    path = os.path.join(OUT, "aliccp_reader.npz")
    np.savez_compressed(path, **out)
    print("aliccp reader: %d lines -> %s (%d bytes; sample %d bytes)" % (LINES, path, os.path.getsize(path), os.path.getsize(sample)))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_reader(os.path.join(OUT, "aliccp_sample.txt"))
    for tag, model, mode in (("esmm_rand", "esmm", "ESMM"), ("escm2_ipw_rand", "escm2", "IPW"), ("escm2_dr_rand", "escm2", "DR")):
        for seed in range(SEED0, SEED0 + 400):
            rec = golden_rand(model, mode, seed)
            e64, e32, ok = check_against_ref(rec)
            print("%s seed %d: esm_ref float64 err %.3g, float32 err %.3g, float32 Adam check %s" % (tag, seed, e64, e32, ok))
            if ok:
                break
        else:
            raise SystemExit("no seed passed")
        path = os.path.join(OUT, "%s.npz" % tag)
        np.savez_compressed(path, **rec)
        print("%s loss=%s keys=%d -> %s (%d bytes)" % (tag, [float(rec["loss_%d" % s][0]) for s in range(STEPS)], len(rec), path,
                                                       os.path.getsize(path)))
