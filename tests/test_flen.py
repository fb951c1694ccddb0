"""rank/flen (paddlerec_amd/flen.py; reference: models/rank/flen/net.py, flen/dygraph_model.py, flen/avazu_reader.py).

tests/flen_ref.py is pinned to tests/golden/flen_D8.npz (the reference's unmodified net.py over the paddle shim,
tools/make_golden_flen.py: a train-mode record with the dropout off and an eval-mode record on running statistics of their
own, duplicate ids, the id 0 as a live row, non-zero biases).  The host mirror is checked against the fixture and the
restatement with the flen_ref-backed operator backend on the CPU (orchestration only; tests/flen_cpu_kernels.py) and with
the HIP kernels (`-m gpu`, tests/test_flen_gpu.py reuses the check_* functions with kernels=None).

Tolerances.  The float64 restatement against the fixture's float32 values and the layer against the fixture: rtol 1e-5
(the bar of test_gatenet.py).  The Adagrad trajectory (TRAJ_REL = 2e-5, the bar of the kernel tests): a step moves a weight
by lr * g / (sqrt(acc) + eps) with acc >= 1e-3, so an error dg of a gradient moves it by at most lr / sqrt(1e-3) * dg =
0.32 dg at the lr 0.01 used here; three steps of gradients that are good to 1e-5 of their scale stay inside 2e-5 of the
weights' scale.
"""
import logging
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import flen_ref as FR
from helpers import GOLDEN, assert_close_scaled, load_golden

S, G, D = 22, 3, 8
TRAJ_REL = 2e-5
DATA_KEYS = ("ids", "label", "D", "sizes", "pred", "loss", "pred_eval")


def _golden():
    g = load_golden("flen_D8")
    p = {k: g[k] for k in g if k not in DATA_KEYS and not k.startswith(("g_", "rs_", "eval_"))}
    return g, p


def _keys(n_layers):
    ks = [FR.EMB, FR.KMF, FR.KFM]
    for stem in (FR.FC, FR.HEAD, FR.HEAD_ALIAS) + tuple(FR.LIN % i for i in range(n_layers)):
        ks += [stem + ".weight", stem + ".bias"]
    for stem in (FR.FBN,) + tuple(FR.NORM % i for i in range(n_layers)):
        ks += [stem + ".weight", stem + ".bias", stem + "._mean", stem + "._variance"]
    return sorted(ks)


def _eval_params(g, p):
    return dict(p, **{k[len("eval_"):]: g[k] for k in g if k.startswith("eval_")})


def test_flen_ref_matches_reference_golden():
    g, p = _golden()
    assert g["ids"].shape == (10, S + 1) and [int(x) for x in g["sizes"]] == [16, 8] and p[FR.EMB].shape == (40, D)
    live = g["ids"][:, 1:]
    assert (live == 0).any() and len(np.unique(live)) < live.size                    # id 0 + duplicates
    assert all(np.abs(p[k]).max() > 0 for k in p if k.endswith(".bias"))             # a dropped bias term would show
    assert sorted(p) == _keys(2)
    assert p[FR.KMF].shape == (3, 1) and p[FR.KFM].shape == (3, 1)
    assert np.array_equal(p[FR.HEAD + ".weight"], p[FR.HEAD_ALIAS + ".weight"])
    o = FR.run(p, g["ids"], g["label"], training=True)
    assert_close_scaled(o["pred"], g["pred"], 1e-5, "pred")
    assert_close_scaled(o["loss"], g["loss"], 1e-5, "loss")
    assert sorted(o["grads"]) == sorted(k for k in p if not k.endswith(("._mean", "._variance")))
    for k, v in o["grads"].items():
        assert_close_scaled(v, g["g_" + k], 1e-5, "g " + k)
    assert not g["g_" + FR.KFM].any() and not o["grads"][FR.KFM].any()               # dead code: never a gradient
    assert g["g_" + FR.EMB][0].any()                                                 # no padding_idx: row 0 trains
    for k, v in o["stats"].items():
        assert_close_scaled(v, g["rs_" + k], 1e-5, "running " + k)
    # column 0 is never used
    other = g["ids"].copy()
    other[:, 0] = (other[:, 0] + 7) % 40
    assert np.array_equal(FR.run(p, other, training=True)["pred"], o["pred"])
    # eval mode on running statistics of their own
    pe = _eval_params(g, p)
    assert any(np.abs(pe[k] - p[k]).max() > 0.1 for k in pe if k.endswith("._mean"))
    assert_close_scaled(FR.run(pe, g["ids"])["pred"], g["pred_eval"], 1e-5, "pred (eval)")
    assert np.abs(g["pred_eval"] - g["pred"]).max() > 1e-3


def _layer(N, sizes, device, kernels, D_=D, **kw):
    from paddlerec_amd.flen import FLENLayer
    if kernels is not None:
        kw["kernels"] = kernels
    return FLENLayer(N, D_, S, G, sizes, device=device, **kw)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _merge(ids, rg, N, D_):
    out = np.zeros((N, D_), np.float64)
    np.add.at(out, ids[:, 1:].reshape(-1), rg.reshape(-1, D_))
    return out


def check_layer_on_fixture(device, kernels, rel):
    """One train_step leaves the fixture's pred, loss, gradients and running statistics in the layer; eval-mode forward
    gives the fixture's second record."""
    g, p = _golden()
    N = p[FR.EMB].shape[0]
    sizes = [int(x) for x in g["sizes"]]
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    m = _layer(N, sizes, device, kernels)
    bound = np.sqrt(6.0 / (N + D))
    assert 0.9 * bound < float(m.embedding.abs().max()) <= bound                     # XavierUniform, row 0 like any other
    assert m.rec.shape == (N, 32) and m.rec[0, :D].any() and not m.rec[:, D:].any()
    assert m.group_begin == [0, 13, 16, 22] and m.ld_x0 == 176 and m.dropout_rate == 0.0
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in p.items()}
    sd = m.state_dict()
    assert sd[FR.HEAD + ".weight"].data_ptr() == sd[FR.HEAD_ALIAS + ".weight"].data_ptr()
    assert sd[FR.HEAD + ".bias"].data_ptr() == sd[FR.HEAD_ALIAS + ".bias"].data_ptr()
    assert float(sd[FR.FBN + "._variance"].min()) == 1.0 and not sd[FR.FBN + "._mean"].any()
    m.set_dict(p)
    sparse_inputs = [T(g["ids"][:, s:s + 1]) for s in range(S + 1)]                  # the reference's list of [B,1]
    loss, pred = m.train_step(sparse_inputs, T(g["label"]), lr=1e-9)
    assert int(m.status.item()) == 0
    assert_close_scaled(_np(loss), g["loss"], rel, "loss")
    assert_close_scaled(_np(pred), g["pred"], rel, "pred (train_step)")
    gd = {k: _np(v) for k, v in m.grad_dict().items()}
    assert sorted(gd) == sorted(k for k in p if k != FR.EMB and not k.endswith(("._mean", "._variance")))
    for k in gd:
        assert_close_scaled(gd[k], g["g_" + k], rel, "g " + k)
    assert not gd[FR.KFM].any()                                                      # exactly zero
    rg = _np(m._last["row_grad"])
    assert rg.shape == (len(g["ids"]), S * D)
    assert_close_scaled(_merge(g["ids"], rg, N, D), g["g_" + FR.EMB], rel, "g " + FR.EMB)
    for k in p:
        if k.endswith(("._mean", "._variance")):
            assert_close_scaled(_np(m.state_dict()[k]), g["rs_" + k], rel, "running " + k)
    # eval mode: the running statistics, one [B,23] tensor in place of the list
    m.set_dict(_eval_params(g, p))
    assert_close_scaled(_np(m.forward(T(g["ids"]))), g["pred_eval"], rel, "pred (eval)")
    return m


def test_layer_host_logic_cpu_backend_matches_fixture():
    import flen_cpu_kernels
    check_layer_on_fixture("cpu", flen_cpu_kernels, 1e-5)


def _small_batch(rng, N, B):
    ids = rng.integers(0, N, (B, S + 1)).astype(np.int64)
    ids[1::2, 1:9] = ids[0::2, 1:9][:ids[1::2].shape[0]]       # duplicates WITHIN a step: (sum g)^2 != sum g^2
    ids[0, 3] = 0
    return ids, (rng.random((B, 1)) < 0.5).astype(np.int64)


def _state64(m):
    return {k: _np(v).copy() for k, v in m.state_dict().items()}


def _acc64(m, p):
    acc = {k: _np(m.dense.pm[k]).copy() for k in m.dense.names}
    acc[FR.EMB] = _np(m.sparse_state["m"]).copy()
    assert sorted(acc) == sorted(FR.trainable(p))
    return acc


def check_adagrad_trajectory(device, kernels, rel):
    """Three steps against the restatement: parameters, accumulators and running statistics; untouched rows and
    kernel_fm bit-unchanged; the accumulators start at 1e-3."""
    rng = np.random.default_rng(5)
    N, B, lr, sizes = 64, 12, 0.01, [16, D]
    m = _layer(N, sizes, device, kernels)
    m._ensure_sparse_state()
    for name in (FR.FBN, FR.NORM % 0, FR.NORM % 1, FR.FC, FR.LIN % 0, FR.LIN % 1, FR.HEAD):
        m.dense.p[name + ".bias"].copy_(torch.as_tensor(0.1 * rng.standard_normal(m.dense.p[name + ".bias"].shape)))
    p = _state64(m)
    acc = _acc64(m, p)
    assert all(np.all(a == np.float32(1e-3)) for a in acc.values())                  # initial_accumulator_value
    assert np.all(_np(m.sparse_state["acc"]) == np.float32(1e-3))
    table0, kfm0, acc0 = m.embedding.clone(), m.dense.p[FR.KFM].clone(), m.sparse_state["m"].clone()
    touched = np.zeros(N, bool)
    for step in range(3):
        ids, label = _small_batch(rng, N - 8, B)                                     # the last 8 rows are never touched
        touched[np.unique(ids[:, 1:])] = True
        o = FR.train_step(p, acc, ids, label, lr)
        uniq, merged = FR.merged_rows(ids[:, 1:], o["row_grad"], N)
        sq = np.zeros((N, D))
        np.add.at(sq, ids[:, 1:].reshape(-1), o["row_grad"].reshape(-1, D) ** 2)
        assert np.abs(merged ** 2 - sq[uniq]).max() > 1e-3 * np.abs(sq).max()        # the two readings differ here
        loss, _ = m.train_step(torch.as_tensor(ids).to(device), torch.as_tensor(label).to(device), lr=lr)
        assert_close_scaled(_np(loss), o["loss"], rel, "loss of step %d" % step)
    assert int(m.status.item()) == 0 and m.step_count == 3
    got, gacc = _state64(m), _acc64(m, p)
    for k in p:
        assert_close_scaled(got[k], p[k], rel, "after 3 steps: " + k)
    for k in acc:
        assert_close_scaled(gacc[k], acc[k], rel, "accumulator of " + k)
    assert touched.any() and not touched[-8:].any()
    assert torch.equal(m.embedding[~torch.as_tensor(touched)].cpu(), table0[~torch.as_tensor(touched)].cpu())
    assert torch.equal(m.sparse_state["m"][~torch.as_tensor(touched)].cpu(), acc0[~torch.as_tensor(touched)].cpu())
    assert bool((m.sparse_state["m"][torch.as_tensor(touched)] > acc0[torch.as_tensor(touched)]).any())
    assert torch.equal(m.dense.p[FR.KFM].cpu(), kfm0.cpu())                          # zero gradient: an exact no-op
    assert np.all(_np(m.dense.pm[FR.KFM]) == np.float32(1e-3))
    assert not torch.equal(m.dense.p[FR.KMF].cpu(), torch.as_tensor(p[FR.KMF] * 0).float())
    return m


def test_adagrad_trajectory_cpu_backend():
    import flen_cpu_kernels
    check_adagrad_trajectory("cpu", flen_cpu_kernels, TRAJ_REL)


def check_dropout_streams(device, kernels, rel, keep_fn):
    """Train mode with dropout: 3n + 1 mask streams per step, advancing by 3n + 1 from step to step; the masks of the
    engine's counter-based generator (keep_fn = dropout_keep) fed to the restatement reproduce the step."""
    rng = np.random.default_rng(9)
    N, B, lr, sizes, rate, seed = 64, 12, 0.01, [16, D], 0.2, 77
    n, ns = len(sizes), 3 * len(sizes) + 1
    m = _layer(N, sizes, device, kernels, dropout_rate=rate, dropout_seed=seed)
    m._ensure_sparse_state()
    p = _state64(m)
    acc = _acc64(m, p)
    widths = [16, 16, 16, D, D, D, D]                                                # the 3n matrices of the DNN, then fwbi
    assert len(widths) == ns
    for step in (1, 2):
        ids, label = _small_batch(rng, N, B)
        keeps = [keep_fn((B, widths[j]), rate, seed, step * ns + j) for j in range(ns)]
        assert all(0 < k.mean() < 1 for k in keeps[:3 * n])
        o = FR.train_step(p, acc, ids, label, lr, keeps=keeps, rate=rate)
        loss, pred = m.train_step(torch.as_tensor(ids).to(device), torch.as_tensor(label).to(device), lr=lr)
        assert_close_scaled(_np(loss), o["loss"], rel, "loss of step %d" % step)
        assert_close_scaled(_np(pred), o["pred"], rel, "pred of step %d" % step)
        assert_close_scaled(_np(m._last["row_grad"]), o["row_grad"].reshape(B, -1), rel, "row gradient of step %d" % step)
    got = _state64(m)
    for k in p:
        assert_close_scaled(got[k], p[k], rel, "after 2 steps with dropout: " + k)
    # eval mode has no dropout: forward is a function of the parameters alone
    x = torch.as_tensor(ids).to(device)
    assert torch.equal(m.forward(x), m.forward(x))
    return m


def test_dropout_streams_cpu_backend():
    import flen_cpu_kernels
    calls = []
    real = flen_cpu_kernels.dropout

    class Spy:
        def __getattr__(self, name):
            return getattr(flen_cpu_kernels, name)

        @staticmethod
        def dropout(x, p, seed, stream_a, stream_b=None, out=None, step_stride=0):
            calls.append((stream_a, stream_b, step_stride))
            return real(x, p, seed, stream_a, stream_b, out, step_stride)

    check_dropout_streams("cpu", Spy(), TRAJ_REL, flen_cpu_kernels.dropout_keep)
    # per step: n double passes + n + 1 single ones forward, the same backward; 7 streams, stride 7
    per_step = len(calls) // 2
    assert per_step == 2 * (2 * 2 + 1)
    for step, chunk in ((1, calls[:per_step]), (2, calls[per_step:])):
        used = sorted({s for a, b, _ in chunk for s in (a, b) if s is not None})
        assert used == list(range(7 * step, 7 * step + 7))
        assert all(st == 7 for _, _, st in chunk)
        assert sorted((a, b) for a, b, _ in chunk if b is not None) == sorted(
            [(7 * step + 3 * i, 7 * step + 3 * i + 1) for i in range(2)] * 2)


def check_batch_of_one(device, kernels):
    """B = 1 (the sample config.yaml): every BN output equals its bias, pred = sigmoid(linear.bias . ) of the biases and
    nothing upstream of a BN moves."""
    rng = np.random.default_rng(3)
    N, sizes = 20, [16, D]
    m = _layer(N, sizes, device, kernels)
    p = m.dense.p
    p[FR.HEAD + ".bias"].fill_(0.3)
    table0 = m.embedding.clone()
    up0 = {k: p[k].clone() for k in (FR.KMF, FR.FC + ".weight", FR.FC + ".bias", FR.LIN % 0 + ".weight",
                                     FR.LIN % 1 + ".weight", FR.NORM % 0 + ".weight", FR.FBN + ".weight")}
    ids = torch.as_tensor(rng.integers(0, N, (1, S + 1))).to(device)
    loss, pred = m.train_step(ids, torch.ones(1, 1, dtype=torch.int64, device=device), lr=0.04)
    # BN biases are 0 at construction, so the head sees zeros: pred = sigmoid(linear.bias)
    assert abs(float(pred) - 1.0 / (1.0 + np.exp(-np.float32(0.3)))) < 1e-6
    assert abs(float(loss) + np.log(float(pred))) < 1e-6
    assert torch.equal(m.embedding.cpu(), table0.cpu())                              # the table does not move
    for k, v in up0.items():
        assert torch.equal(p[k].cpu(), v.cpu()), k
    assert float(p[FR.HEAD + ".bias"]) > float(np.float32(0.3))                      # label 1: the head's bias moves up
    assert bool((p[FR.FBN + ".bias"] != 0).any())                                    # and so do the BN biases
    assert int(m.status.item()) == 0
    return m


def test_batch_of_one_cpu_backend():
    import flen_cpu_kernels
    check_batch_of_one("cpu", flen_cpu_kernels)


def test_constructor_rejects_bad_shapes():
    import flen_cpu_kernels
    from paddlerec_amd.flen import FLENLayer
    with pytest.raises(ValueError, match="must end in sparse_feature_dim"):
        FLENLayer(20, D, S, G, [16, D + 1], device="cpu", kernels=flen_cpu_kernels)
    with pytest.raises(ValueError, match="must end in sparse_feature_dim"):
        FLENLayer(20, D, S, G, [], device="cpu", kernels=flen_cpu_kernels)
    with pytest.raises(ValueError, match="sum to sparse_inputs_slots"):
        FLENLayer(20, D, S, G, [D], field_sizes=(13, 3, 5), device="cpu", kernels=flen_cpu_kernels)
    with pytest.raises(ValueError, match="sum to sparse_inputs_slots"):
        FLENLayer(20, D, S, G, [D], field_sizes=(16, 6), device="cpu", kernels=flen_cpu_kernels)
    m = FLENLayer(20, D, S, 4, [D], field_sizes=(5, 1, 2, 14), device="cpu", kernels=flen_cpu_kernels)
    assert m.group_begin == [0, 5, 6, 8, 22] and tuple(m.dense.p[FR.KMF].shape) == (6, 1)
    with pytest.raises(ValueError, match="23 sparse inputs"):
        m.forward(torch.zeros(2, S, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ reader, trainer
SAMPLE = os.path.join(GOLDEN, "flen_sample.txt")


def test_avazu_reader_parses_the_sample_lines():
    from paddlerec_amd import reader
    with open(SAMPLE) as f:
        lines = [line.strip().split(",") for line in f if line.strip()]
    assert len(lines) == 13 and [len(x) for x in lines] == [24] * 12 + [23]          # the appended malformed line
    want = np.asarray(lines[:12], dtype=np.int64)
    with open(SAMPLE, "rb") as f:
        label, ids, _ = reader.parse_avazu_csv(f.read())
    assert label.dtype == torch.int64 and ids.dtype == torch.int64
    assert np.array_equal(label.numpy(), want[:, -1]) and np.array_equal(ids.numpy(), want[:, :-1])
    batches = list(reader.AvazuReader([SAMPLE], 5, "cpu"))
    assert [tuple(b[0].shape) for b in batches] == [(5, 1), (5, 1)]                  # 12 lines: drop_last
    assert [tuple(b[1].shape) for b in batches] == [(5, S + 1), (5, S + 1)]
    assert np.array_equal(torch.cat([b[1] for b in batches]).numpy(), want[:10, :-1])
    assert np.array_equal(torch.cat([b[0] for b in batches]).numpy().reshape(-1), want[:10, -1])
    assert len({int(x) for x in want[:, 0]}) > 1                                     # column 0 is present in the batch ...
    import flen_cpu_kernels
    m = _layer(20, [D], "cpu", flen_cpu_kernels)
    other = batches[0][1].clone()
    other[:, 0] = 19 - other[:, 0]
    assert torch.equal(m.forward(batches[0][1]), m.forward(other))                   # ... and ignored by the layer
    # rank sharding of the files, as the other readers
    assert list(reader.AvazuReader([SAMPLE, SAMPLE], 12, "cpu", shard=(1, 2)))[0][1].shape == (12, S + 1)


def reference_config():
    """The values of the reference's flen/config.yaml, typed in (flat keys, as trainer.load_yaml makes them)."""
    return {"runner.train_data_dir": "data/sample_data/train", "runner.train_reader_path": "avazu_reader",
            "runner.use_gpu": False, "runner.use_auc": True, "runner.train_batch_size": 1, "runner.epochs": 1,
            "runner.print_interval": 2, "runner.model_save_path": "output_model_flen", "runner.infer_batch_size": 3,
            "runner.infer_reader_path": "avazu_reader", "runner.test_data_dir": "data/sample_data/train",
            "runner.infer_load_path": "output_model_flen", "runner.infer_start_epoch": 0, "runner.infer_end_epoch": 1,
            "hyper_parameters.optimizer.class": "Adagrad", "hyper_parameters.optimizer.learning_rate": 0.04,
            "hyper_parameters.optimizer.strategy": "async", "hyper_parameters.sparse_inputs_slots": 22,
            "hyper_parameters.sparse_feature_number": 20, "hyper_parameters.sparse_num_field": 3,
            "hyper_parameters.sparse_feature_dim": 32, "hyper_parameters.layer_sizes_dnn": [64, 32],
            "hyper_parameters.distributed_embedding": 0}


def test_dygraph_model_plugin_surface():
    import flen_cpu_kernels
    from paddlerec_amd import trainer
    from paddlerec_amd.flen import DygraphModel, FLENLayer
    assert "flen" in trainer.MODELS and "flen" in trainer.__doc__
    assert trainer.guess_model("/x/models/rank/flen/config.yaml") == "flen"
    dm = trainer._dygraph_model("flen")
    assert isinstance(dm, DygraphModel)
    net = dm.create_model(reference_config(), "cpu", kernels=flen_cpu_kernels)
    assert isinstance(net, FLENLayer) and net.field_sizes == (13, 3, 6) and net.dropout_rate == 0.2
    assert net.dropout_seed == 12345 and net.sparse_feature_dim == 32 and sorted(net.state_dict()) == _keys(2)
    # the reference's 24 arrays (label LAST) through the plugin methods, on the fixture's net
    g, p = _golden()
    small = dict(reference_config(), **{"hyper_parameters.sparse_feature_number": 40, "hyper_parameters.sparse_feature_dim": D,
                                        "hyper_parameters.layer_sizes_dnn": [16, 8],
                                        "hyper_parameters.optimizer.learning_rate": 1e-9})
    net = dm.create_model(small, "cpu", kernels=flen_cpu_kernels)
    net.dropout_rate = 0.0
    net.set_dict(_eval_params(g, p))
    metrics, names = dm.create_metrics("cpu")
    batch = [g["ids"][:, s:s + 1] for s in range(S + 1)] + [g["label"]]
    assert len(batch) == 24
    metrics, printed = dm.infer_forward(net, metrics, batch, small)
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == len(g["label"]) and sorted(printed) == ["logloss"]
    t = g["label"].astype(np.float64)
    want = -(t * np.log(g["pred_eval"]) + (1 - t) * np.log(1 - g["pred_eval"])).mean()
    assert_close_scaled(float(printed["logloss"]), want, 1e-5, "logloss")
    net.set_dict(p)
    loss, metrics, printed = dm.train_forward(net, metrics, batch, small)
    assert_close_scaled(float(loss), g["loss"], 1e-5, "loss")
    assert names == ["auc"] and sorted(printed) == ["loss"] and printed["loss"] is loss


def run_trainer_loops(tmp_path, device, kernels, caplog=None):
    """One epoch over the reference's own sample lines (tests/golden/flen_sample.txt, batch 3) -> a checkpoint -> infer
    over it -> a fresh model loaded from it holds the trained net bit for bit, accumulators included."""
    from paddlerec_amd import checkpoint, trainer
    d = tmp_path / "run"
    (d / "data").mkdir(parents=True)
    shutil.copy(SAMPLE, d / "data" / "part-0")
    cfg = dict(reference_config(), **{
        "config_abs_dir": str(d), "runner.train_data_dir": "data", "runner.test_data_dir": "data",
        "runner.train_batch_size": 3, "runner.model_save_path": str(tmp_path / "out"),
        "runner.infer_load_path": str(tmp_path / "out"), "hyper_parameters.optimizer.lazy_mode": True})
    if caplog is not None:
        caplog.set_level(logging.INFO, logger="paddlerec_amd.trainer")
    s, net = trainer.train(cfg, "flen", device, kernels)
    if caplog is not None:
        said = [r.getMessage() for r in caplog.records if "lazy_mode is ignored" in r.getMessage()]
        assert len(said) == 1 and "Adagrad" in said[0]
    assert [x["epoch"] for x in s] == [0] and s[0]["batches"] == 4 and s[0]["samples"] == 12
    assert np.isfinite(s[0]["loss"]) and 0.0 <= s[0]["auc"] <= 1.0
    assert int(net.status.item()) == 0 and net.step_count == 4
    with open(os.path.join(s[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert sorted(sd) == _keys(2) and sd[FR.EMB].shape == (20, 32) and sd[FR.LIN % 0 + ".weight"].shape == (704, 64)
    r = trainer.infer(cfg, "flen", device, kernels)
    assert [x["epoch"] for x in r] == [0] and 0.0 <= r[0]["auc"] <= 1.0 and r[0]["samples"] == 12
    fresh = trainer._dygraph_model("flen").create_model(cfg, device, **({"kernels": kernels} if kernels is not None else {}))
    checkpoint.load_model(s[-1]["model_dir"], fresh)
    for k, v in net.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    assert fresh.step_count == net.step_count
    assert torch.equal(fresh.sparse_state["m"].cpu(), net.sparse_state["m"].cpu())
    assert torch.equal(fresh.dense.m.cpu(), net.dense.m.cpu())
    return s, r


def test_train_checkpoint_infer_cpu_backend(tmp_path, caplog):
    import flen_cpu_kernels
    run_trainer_loops(tmp_path, "cpu", flen_cpu_kernels, caplog)


def check_resume_is_bit_identical(tmp_path, device, kernels):
    """Save after step 2, reload into a fresh layer: its step 3 equals the uninterrupted run's step 3 bit for bit —
    parameters, running statistics and accumulators (dropout on: the mask streams follow the restored step count)."""
    from paddlerec_amd import checkpoint
    rng = np.random.default_rng(11)
    N, B, lr, sizes = 48, 9, 0.04, [16, D]
    kw = dict(dropout_rate=0.2, dropout_seed=5)
    batches = [_small_batch(rng, N, B) for _ in range(3)]
    T = lambda a: torch.as_tensor(a).to(device)
    torch.manual_seed(1)
    a = _layer(N, sizes, device, kernels, **kw)
    for ids, label in batches[:2]:
        a.train_step(T(ids), T(label), lr=lr)
    path = checkpoint.save_model(a, None, str(tmp_path / "ck"), 0, prefix="rec")
    torch.manual_seed(2)                                                             # another initial draw
    b = _layer(N, sizes, device, kernels, **kw)
    checkpoint.load_model(path, b)
    assert b.step_count == 2
    la, _ = a.train_step(T(batches[2][0]), T(batches[2][1]), lr=lr)
    lb, _ = b.train_step(T(batches[2][0]), T(batches[2][1]), lr=lr)
    assert torch.equal(la.cpu(), lb.cpu())
    for k, v in a.state_dict().items():
        assert torch.equal(v.cpu(), b.state_dict()[k].cpu()), k
    assert torch.equal(a.sparse_state["m"].cpu(), b.sparse_state["m"].cpu())
    assert torch.equal(a.dense.m.cpu(), b.dense.m.cpu())
    assert bool((a.sparse_state["m"] != 1e-3).any()) and bool((a.dense.m != 1e-3).any())


def test_checkpoint_resume_is_bit_identical_cpu_backend(tmp_path):
    import flen_cpu_kernels
    check_resume_is_bit_identical(tmp_path, "cpu", flen_cpu_kernels)
