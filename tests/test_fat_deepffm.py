"""rank/fat_deepffm (paddlerec_amd/fat_deepffm.py; reference: models/rank/fat_deepffm/net.py, fat_deepffm/dygraph_model.py).

tests/fat_deepffm_ref.py is pinned to tests/golden/fat_deepffm_D9.npz (the reference's unmodified net.py over the paddle
shim, tools/make_golden_fat_deepffm.py: S 6, Dn 3, D 9, a two-layer tower, duplicate ids, the id 0 as a live row, a
constant cen.dense_w row and a dense value of 0 for the max pool's ties, non-zero biases).  The host mirror is checked
against the fixture and the restatement with the fat_deepffm_ref-backed operator backend on the CPU (orchestration only;
tests/fat_deepffm_cpu_kernels.py) and with the HIP kernels (`-m gpu`, tests/test_fat_deepffm_gpu.py).  The argument checks
of the rec_fatffm_* entry points run here too: they return before any launch."""
import logging
import os
import pickle

import numpy as np
import pytest
import torch

import fat_deepffm_ref as FR
from helpers import assert_adam_weights_close, assert_close_scaled, load_golden

S, DN, D = 6, 3, 9
F = S + DN
R = F * D                   # 81
DATA_KEYS = ("ids", "dense", "label", "D", "fc", "pred", "loss")
KEYS = sorted(["bias", "cen.dense_w", "cen.embedding.weight", "cen.fc.ReductionLinear.weight",
               "cen.fc.ReductionLinear.bias", "cen.fc.AdditionLinear.weight", "cen.fc.AdditionLinear.bias"] +
              ["dnn.linear_%d.%s" % (i, w) for i in range(3) for w in ("weight", "bias")])


def _golden():
    g = load_golden("fat_deepffm_D9")
    p = {k: g[k] for k in g if k not in DATA_KEYS and not k.startswith("g_")}
    return g, p


def test_ref_matches_reference_golden():
    g, p = _golden()
    assert g["ids"].shape == (10, S) and g["dense"].shape[1] == DN and [int(x) for x in g["fc"]] == [16, 8]
    assert (g["ids"] == 0).sum() >= 2 and len(np.unique(g["ids"])) < g["ids"].size   # id 0 + duplicates
    assert (g["dense"] == 0).sum() == 1
    assert all(np.abs(p[k]).max() > 0 for k in p if k.endswith("bias"))              # a dropped bias term would show
    assert sorted(p) == KEYS and p["cen.embedding.weight"].shape == (301, R)
    assert p["cen.fc.ReductionLinear.weight"].shape == (F * F, F * F) and p["dnn.linear_0.weight"].shape == (36 * D, 16)
    dw = p["cen.dense_w"].reshape(DN, R)
    assert sum(bool((row == row[0]).all()) for row in dw) == 1                       # one constant row: its slices tie
    # the conditions the fixture was made under: an unsaturated logit and no gradient at noise level
    assert 0.05 < g["pred"].min() and g["pred"].max() < 0.95
    assert min(float(np.abs(g["g_" + k]).max()) for k in p) >= 1e-4
    o = FR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D)
    f = o["f"]
    for x in (f["a"], f["z1"]):                                                       # both ReLU masks are live
        assert 0.2 < float((x == 0).mean()) < 0.8
    E = f["E"]
    assert ((E == E.max(axis=3, keepdims=True)).sum(axis=3) > 1).any()               # ties of the max pool
    assert_close_scaled(o["pred"], g["pred"], 1e-5, "pred")
    assert_close_scaled(o["loss"], g["loss"], 1e-5, "loss")
    assert sorted(o["g"]) == sorted(p)
    for k in p:
        assert_close_scaled(o["g"][k], g["g_" + k], 1e-5, "g " + k)
    assert g["g_cen.embedding.weight"][0].any()                                       # no padding_idx: row 0 trains


def _merge(ids, rg, N):
    out = np.zeros((N, R), np.float64)
    np.add.at(out, ids.reshape(-1), rg[:, :R])
    return out


def _layer(N, fc, device, kernels, **kw):
    from paddlerec_amd.fat_deepffm import FAT_DeepFFMLayer
    if kernels is not None:
        kw["kernels"] = kernels
    return FAT_DeepFFMLayer(N, D, DN, S, fc, device=device, **kw)


def check_layer_on_fixture(device, kernels, rel):
    """Forward = the fixture's pred; one train_step leaves the fixture's loss and gradients in the layer.  rel: one bound
    for every tensor, or {key: bound} with "pred" / "loss" / the parameter names."""
    g, p = _golden()
    tol = (lambda k: rel[k]) if isinstance(rel, dict) else (lambda k: rel)
    N = p["cen.embedding.weight"].shape[0]
    fc = [int(x) for x in g["fc"]]
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    m = _layer(N, fc, device, kernels)
    std = 0.1 / np.sqrt(D)
    assert 1.9 * std < float(m.embedding.abs().max()) <= 2 * std * 1.0001            # TruncatedNormal(std, 2 std)
    assert m.emb_table.shape == (N, 84) and not m.emb_table[:, R:].any() and m.emb_table[0, :R].any()
    assert float(m.dense.p["cen.dense_w"].min()) == 1.0 == float(m.dense.p["cen.dense_w"].max())
    assert float(m.dense.p["bias"]) == 0.0 and not m.dense.p["cen.fc.ReductionLinear.bias"].any()
    assert (m.num_fields, m.num_pairs, m.input_size, m.ld_attn, m.ld_pair) == (F, 36, 324, 84, 324)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in p.items()}
    m.set_dict(p)
    sparse_inputs = [T(g["ids"][:, s:s + 1]) for s in range(S)]             # the reference's list of [B,1]
    pred = m.forward(sparse_inputs, T(g["dense"]))
    assert_close_scaled(pred.cpu().numpy(), g["pred"], tol("pred"), "pred")
    loss, pred2 = m.train_step(sparse_inputs, T(g["dense"]), T(g["label"]), lr=1e-9)
    assert int(m.status.item()) == 0
    assert_close_scaled(loss.cpu().numpy(), g["loss"], tol("loss"), "loss")
    assert_close_scaled(pred2.cpu().numpy(), g["pred"], tol("pred"), "pred (train_step)")
    gd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.grad_dict().items()}
    assert sorted(gd) == sorted(k for k in p if k != "cen.embedding.weight")
    for k in gd:
        assert_close_scaled(gd[k], g["g_" + k], tol(k), "g " + k)
    rg = m._last["row_grad"].cpu().numpy()
    assert rg.shape == (len(g["ids"]) * S, 84) and not rg[:, R:].any()
    assert_close_scaled(_merge(g["ids"], rg, N), g["g_cen.embedding.weight"], tol("cen.embedding.weight"),
                        "g cen.embedding.weight")
    return m


def test_layer_host_logic_cpu_backend_matches_fixture():
    import fat_deepffm_cpu_kernels
    check_layer_on_fixture("cpu", fat_deepffm_cpu_kernels, 1e-5)


def test_state_dict_keys_are_the_references():
    import fat_deepffm_cpu_kernels
    g, p = _golden()
    m = _layer(301, [16, 8], "cpu", fat_deepffm_cpu_kernels)
    assert sorted(m.state_dict()) == sorted(p) == KEYS
    assert tuple(m.state_dict()["cen.dense_w"].shape) == (1, DN, R)
    m.state_dict()["cen.embedding.weight"][5, 3] = 7.0                       # the key is a view of the padded table
    assert float(m.emb_table[5, 3]) == 7.0
    # initialisers: XavierUniform for the CENet's Linears (paddle.nn.Linear's default), Normal(std 1 / sqrt(fan_in)) for
    # the tower
    q = _layer(11, [256, 64], "cpu", fat_deepffm_cpu_kernels).dense.p
    bound = np.sqrt(6.0 / (2 * F * F))
    for k in ("cen.fc.ReductionLinear.weight", "cen.fc.AdditionLinear.weight"):
        assert 0.98 * bound < float(q[k].abs().max()) <= bound
        assert abs(float(q[k].std()) - bound / np.sqrt(3)) < 0.05 * bound
    assert abs(float(q["dnn.linear_0.weight"].std()) * np.sqrt(36 * D) - 1.0) < 0.05
    assert abs(float(q["dnn.linear_1.weight"].std()) * np.sqrt(256) - 1.0) < 0.05


def _small_batch(rng, N, B=12):
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    ids[:, 0] = 5                                                             # a hot row
    ids[::5, 3] = 0                                                           # id 0: a live row
    dense = rng.random((B, DN), dtype=np.float32)
    dense[1, 2] = 0.0
    label = (rng.random((B, 1)) < 0.4).astype(np.int64)
    return ids, dense, label


def check_adam_trajectory(device, kernels, lazy, rel, drop=None, l2_dnn=0.0):
    """Three steps against the plain restatement's trajectory (fat_deepffm_ref.Trainer): loss and prediction of every
    step, weights, table and the table's moments after the last.  The two Adam forms part on the rows that only the first
    batch touched: lazy=False decays their moments (and moves them) in steps 2 and 3 as well, lazy=True leaves them as
    step 1 wrote them.  drop = (rate, seed): train mode.
    The fixture's constant cen.dense_w row is redrawn first: Adam's first step moves every element by exactly +-lr, so a
    constant row becomes a row of values that tie up to the last bit, and which of them the max pool picks in step 2 is
    decided by float32 round-off on either side (the single-step tests keep the ties)."""
    g, p = _golden()
    N, fc = p["cen.embedding.weight"].shape[0], [int(x) for x in g["fc"]]
    p = dict(p, **{"cen.dense_w": p["cen.dense_w"].copy()})
    p["cen.dense_w"][0, 1] = np.random.default_rng(3).normal(0, 0.25, R).astype(np.float32)
    kw = {} if drop is None else dict(dropout_rate=drop[0], dropout_seed=drop[1])
    m = _layer(N, fc, device, kernels, l2_dnn=l2_dnn, **kw)
    m.lazy_mode = lazy
    m.set_dict(p)
    tr = FR.Trainer(p, D, lazy=lazy, drop=drop, l2_dnn=l2_dnn)
    rng = np.random.default_rng(8)
    T = lambda a: torch.as_tensor(a).to(device)
    touched = np.zeros(N, bool)
    batches = []
    for step in range(3):
        ids, dense, label = _small_batch(rng, N)
        batches.append(ids)
        touched[ids.reshape(-1)] = True
        loss, pred = m.train_step(T(ids), T(dense), T(label), lr=1e-2)
        ol, op = tr.train_step(ids, dense, label, lr=1e-2)
        np.testing.assert_allclose(float(loss), ol, rtol=rel)
        np.testing.assert_allclose(pred.cpu().numpy(), op, rtol=rel, atol=1e-6)
    assert int(m.status.item()) == 0 and m.step_count == 3
    assert not m.emb_table[:, R:].any()                                       # the pad columns never move
    for k, v in m.state_dict().items():
        assert_adam_weights_close(v.detach().cpu().numpy(), tr.p[k], lr=1e-2, steps=3, err_msg=k)
    assert_close_scaled(m.sparse_state["m"].cpu().numpy()[:, :R], tr.m[FR.EMB], rel, "m of the table")
    assert_close_scaled(m.sparse_state["v"].cpu().numpy()[:, :R], tr.v[FR.EMB], rel, "v of the table")
    moved = (m.embedding.cpu().numpy() != p["cen.embedding.weight"]).any(axis=1)
    assert touched[0] and moved[0] and moved[touched].all() and not moved[~touched].any()
    first = np.zeros(N, bool)                                                 # rows only the FIRST batch touched
    first[batches[0].reshape(-1)] = True
    first[np.concatenate([b.reshape(-1) for b in batches[1:]])] = False
    assert first.any()
    other = FR.Trainer(p, D, lazy=not lazy, drop=drop, l2_dnn=l2_dnn)         # the trajectory of the other Adam form
    rng = np.random.default_rng(8)
    for step in range(3):
        other.train_step(*_small_batch(rng, N), lr=1e-2)
    assert (other.m[FR.EMB][first] != m.sparse_state["m"].cpu().numpy()[first][:, :R]).any()
    return m


@pytest.mark.parametrize("lazy", [False, True])
def test_adam_trajectory_cpu_backend(lazy):
    import fat_deepffm_cpu_kernels
    check_adam_trajectory("cpu", fat_deepffm_cpu_kernels, lazy, 1e-5)


def check_dropout_streams(device, kernels, rel):
    """Train mode: 2n + 1 mask streams per step, the LAST Linear's [B,1] output dropped too (net.py:200-202); L2Decay on
    the three DNN weights only."""
    from oracle import dcn_v2_ref as X
    g, p = _golden()
    N, fc = p["cen.embedding.weight"].shape[0], [int(x) for x in g["fc"]]
    rate, seed, l2 = 0.5, 77, 1e-3
    m = _layer(N, fc, device, kernels, dropout_rate=rate, dropout_seed=seed, l2_dnn=l2)
    m.set_dict(p)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    ev = m.forward(T(g["ids"]), T(g["dense"])).cpu().numpy()
    assert_close_scaled(ev, g["pred"], rel, "forward() is eval mode")
    B, n = len(g["ids"]), len(fc)
    for step in (1, 2):
        loss, pred = m.train_step(T(g["ids"]), T(g["dense"]), T(g["label"]), lr=1e-9)
        o = FR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D, drop=(rate, seed, step), l2_dnn=l2)
        assert_close_scaled(pred.cpu().numpy(), o["pred"], rel, "pred, step %d" % step)
        assert_close_scaled(loss.cpu().numpy(), o["loss"], rel, "loss, step %d" % step)
        # the last Linear's stream is base + 2n with base = step * (2n + 1): where it drops, the logit is y1 + bias alone
        keep = X.dropout_keep((B, 1), rate, seed, step * (2 * n + 1) + 2 * n)
        assert keep.any() and not keep.all()
        f = o["f"]
        alone = 1.0 / (1.0 + np.exp(-(f["y1"].reshape(B, 1) + np.asarray(p["bias"], np.float64))))
        assert_close_scaled(pred.cpu().numpy()[~keep], alone[~keep], rel, "dropped y_dnn, step %d" % step)
        assert (np.abs(pred.cpu().numpy() - alone)[keep] > 1e-4).any()
        gd = m.grad_dict()
        for k in gd:
            assert_close_scaled(gd[k].cpu().numpy(), o["g"][k], rel, "g %s, step %d" % (k, step))
    # the L2 term is in the DNN weights' gradients and in no other
    o0 = FR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D, drop=(rate, seed, 2), l2_dnn=0.0)
    for k in o["g"]:
        same = np.array_equal(o0["g"][k], o["g"][k])
        assert same != (k.startswith("dnn.") and k.endswith(".weight")), k
    return m


def test_dropout_streams_and_l2_cpu_backend():
    import fat_deepffm_cpu_kernels
    check_dropout_streams("cpu", fat_deepffm_cpu_kernels, 1e-5)


def reference_config():
    """The values of the reference's fat_deepffm/config.yaml, typed in (flat keys, as trainer.load_yaml makes them)."""
    return {"runner.train_data_dir": "data/sample_data/train", "runner.train_reader_path": "criteo_reader",
            "runner.use_gpu": False, "runner.use_auc": True, "runner.train_batch_size": 1, "runner.epochs": 1,
            "runner.print_interval": 10, "runner.model_save_path": "output_model_fat_deepffm",
            "runner.infer_batch_size": 1, "runner.infer_reader_path": "criteo_reader",
            "runner.test_data_dir": "data/sample_data/train", "runner.infer_load_path": "output_model_fat_deepffm",
            "runner.infer_start_epoch": 0, "runner.infer_end_epoch": 1,
            "hyper_parameters.optimizer.class": "Adam", "hyper_parameters.optimizer.learning_rate": 0.0001,
            "hyper_parameters.sparse_inputs_slots": 27, "hyper_parameters.sparse_feature_number": 1000001,
            "hyper_parameters.sparse_feature_dim": 10, "hyper_parameters.dense_input_dim": 13,
            "hyper_parameters.distributed_embedding": 0, "hyper_parameters.layer_sizes_dnn": [1600, 1600]}


def test_dygraph_model_plugin_surface():
    import fat_deepffm_cpu_kernels
    from paddlerec_amd.fat_deepffm import DygraphModel, FAT_DeepFFMLayer
    dm = DygraphModel()
    cfg = dict(reference_config(), **{"hyper_parameters.sparse_feature_number": 101})
    net = dm.create_model(cfg, "cpu", kernels=fat_deepffm_cpu_kernels)
    assert isinstance(net, FAT_DeepFFMLayer) and net.sparse_num_field == 26 and net.num_fields == 39   # slots - 1
    assert net.sparse_feature_dim == 10 and net.row_width == 390 and net.emb_table.shape == (101, 392)
    assert net.layer_sizes == [1600, 1600] and net.input_size == 7410 and (net.ld_attn, net.ld_pair) == (1524, 7412)
    assert net.dropout_rate == 0.5 and net.l2_dnn == 1e-7 and net.lazy_mode is False
    assert net.dense.p["dnn.linear_0.weight"].shape == (7410, 1600) and net.dense.p["dnn.linear_2.weight"].shape == (1600, 1)
    # the reference's arrays through the plugin methods, on the fixture's net
    g, p = _golden()
    small = dict(cfg, **{"hyper_parameters.sparse_feature_number": p["cen.embedding.weight"].shape[0],
                         "hyper_parameters.sparse_inputs_slots": S + 1, "hyper_parameters.dense_input_dim": DN,
                         "hyper_parameters.sparse_feature_dim": D,
                         "hyper_parameters.layer_sizes_dnn": [int(x) for x in g["fc"]],
                         "hyper_parameters.optimizer.learning_rate": 1e-9})
    net = dm.create_model(small, "cpu", kernels=fat_deepffm_cpu_kernels)
    net.set_dict(p)
    metrics, names = dm.create_metrics("cpu")
    batch = [g["label"]] + [g["ids"][:, s:s + 1] for s in range(S)] + [g["dense"]]
    assert len(batch) == S + 2
    metrics, _ = dm.infer_forward(net, metrics, batch, small)                # eval mode: the fixture's prediction
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == len(g["label"])
    loss, metrics, print_dict = dm.train_forward(net, metrics, batch, small)
    assert np.isfinite(float(loss)) and names == ["auc"] and set(print_dict) == {"loss"}   # dygraph_model.py:92


def test_trainer_knows_fat_deepffm(tmp_path):
    from paddlerec_amd import trainer
    assert "fat_deepffm" in trainer.MODELS
    d = tmp_path / "models" / "rank" / "fat_deepffm"
    d.mkdir(parents=True)
    assert trainer.guess_model(str(d / "config.yaml")) == "fat_deepffm"
    from paddlerec_amd.fat_deepffm import DygraphModel
    assert isinstance(trainer._dygraph_model("fat_deepffm"), DygraphModel)
    assert "fat_deepffm" in trainer.__doc__


YAML = """
runner:
  train_data_dir: "data/train"
  train_reader_path: "criteo_reader"
  use_gpu: False
  use_auc: True
  train_batch_size: 16
  epochs: 1
  print_interval: 2
  model_save_path: "{out}"
  test_data_dir: "data/train"
  infer_batch_size: 20
  infer_load_path: "{out}"
  infer_start_epoch: 0
  infer_end_epoch: 1
hyper_parameters:
  optimizer:
    class: Adam
    learning_rate: 0.0001
    strategy: async
    lazy_mode: {lazy}
  sparse_inputs_slots: 27
  sparse_feature_number: 30011
  sparse_feature_dim: 4
  dense_input_dim: 13
  distributed_embedding: 0
  layer_sizes_dnn: [32, 16]
"""


def run_trainer_loops(tmp_path, device, kernels, lazy, caplog=None):
    """A fat_deepffm YAML: train (a checkpoint) -> infer over it -> a fresh model loaded from the checkpoint predicts
    exactly like the trained net; the checkpoint holds the reference's keys and shapes."""
    from test_ffm import _slot_lines
    from paddlerec_amd import checkpoint, trainer
    d = tmp_path / "models" / "rank" / "fat_deepffm"
    (d / "data" / "train").mkdir(parents=True)
    (d / "data" / "train" / "part-0").write_text("\n".join(_slot_lines()) + "\n")
    (d / "config.yaml").write_text(YAML.format(out=str(tmp_path / "out"), lazy=str(lazy)))
    cfg = trainer.load_yaml(str(d / "config.yaml"))
    model = trainer.guess_model(str(d / "config.yaml"))
    assert model == "fat_deepffm"
    if caplog is not None:
        caplog.set_level(logging.INFO, logger="paddlerec_amd.trainer")
    s, net = trainer.train(cfg, model, device, kernels)
    if caplog is not None:
        said = [r.getMessage() for r in caplog.records if r.getMessage().startswith("fat_deepffm train mode")]
        assert len(said) == 1 and "last Linear" in said[0] and "saturates" in said[0] and "Dropout(0.50)" in said[0]
    assert net.lazy_mode is lazy and net.dropout_rate == 0.5 and net.l2_dnn == 1e-7
    assert [x["epoch"] for x in s] == [0] and s[0]["batches"] == 5 and s[0]["samples"] == 80
    assert np.isfinite(s[0]["loss"]) and 0.0 <= s[0]["auc"] <= 1.0
    assert int(net.status.item()) == 0 and net.step_count == 5
    with open(os.path.join(s[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    F2, RW = 39 * 39, 39 * 4
    want = {"bias": (1,), "cen.dense_w": (1, 13, RW), "cen.embedding.weight": (30011, RW),
            "cen.fc.ReductionLinear.weight": (F2, F2), "cen.fc.ReductionLinear.bias": (F2,),
            "cen.fc.AdditionLinear.weight": (F2, F2), "cen.fc.AdditionLinear.bias": (F2,),
            "dnn.linear_0.weight": (741 * 4, 32), "dnn.linear_0.bias": (32,), "dnn.linear_1.weight": (32, 16),
            "dnn.linear_1.bias": (16,), "dnn.linear_2.weight": (16, 1), "dnn.linear_2.bias": (1,)}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    r = trainer.infer(cfg, model, device, kernels)
    assert [x["epoch"] for x in r] == [0] and 0.0 <= r[0]["auc"] <= 1.0 and r[0]["samples"] == 80
    dm = trainer._dygraph_model(model)
    fresh = dm.create_model(cfg, device, **({"kernels": kernels} if kernels is not None else {}))
    checkpoint.load_model(s[-1]["model_dir"], fresh)
    for k, v in net.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    assert fresh.step_count == net.step_count
    assert torch.equal(fresh.sparse_state["m"].cpu(), net.sparse_state["m"].cpu())
    assert torch.equal(fresh.dense.m.cpu(), net.dense.m.cpu())
    ids = torch.as_tensor(np.random.default_rng(0).integers(0, 30011, (7, 26)), device=device)
    dense = torch.as_tensor(np.random.default_rng(1).random((7, 13), dtype=np.float32), device=device)
    assert torch.equal(fresh.forward(ids, dense).cpu(), net.forward(ids, dense).cpu())
    return s, r


@pytest.mark.parametrize("lazy", [True, False])
def test_train_checkpoint_infer_cpu_backend(tmp_path, caplog, lazy):
    import fat_deepffm_cpu_kernels
    run_trainer_loops(tmp_path, "cpu", fat_deepffm_cpu_kernels, lazy, caplog)


def check_entry_points_reject_bad_arguments(L):
    """Host checks of the rec_fatffm_* entry points: every call below is refused (or is the empty-batch no-op) before any
    launch, so it runs with dummy non-null pointer values."""
    import ctypes as C
    from paddlerec_amd._lib import FatFFMDesc, FFMDesc
    p = C.c_void_p(4096)                                     # never dereferenced
    n = C.c_size_t(0)
    err = lambda: L.rec_last_error()

    def desc(B=4, S_=6, Dn=3, D_=9, N=100, stride=84, gs=84, lda=81, ldh=324):
        return C.byref(FatFFMDesc(FFMDesc(B, S_, Dn, D_, N, stride, gs), lda, ldh))

    def pool(ids=p, dense=p, W=p, dw=p, out=p, **kw):
        return L.rec_fatffm_pool_fwd(desc(**kw), ids, dense, W, dw, out, p, None)

    def inter(ids=p, dense=p, W=p, dw=p, a=p, H=p, y1=p, **kw):
        return L.rec_fatffm_inter_fwd(desc(**kw), ids, dense, W, dw, a, H, y1, p, None)

    def attn(ids=p, dense=p, W=p, dw=p, a=p, dH=p, dz=p, out=p, **kw):
        return L.rec_fatffm_attn_bwd(desc(**kw), ids, dense, W, dw, a, dH, dz, out, p, None)

    def bwd(ids=p, dense=p, W=p, dw=p, a=p, dH=p, dz=p, dp=p, rg=p, ddw=p, ws=p, ws_bytes=1 << 30, **kw):
        return L.rec_fatffm_bwd(desc(**kw), ids, dense, W, dw, a, dH, dz, dp, rg, ddw, ws, C.c_size_t(ws_bytes), p, None)

    def wsb(**kw):
        return L.rec_fatffm_bwd_workspace_bytes(desc(**kw), C.byref(n))

    for call in (pool, inter, attn, bwd, wsb):
        assert call(D_=0) == -1 and b"bad sizes" in err()
        assert call(S_=0) == -1 and call(B=-1) == -1 and call(N=0) == -1 and call(Dn=-1) == -1
        assert call(S_=52, Dn=13, D_=1, stride=68, gs=68, lda=65 * 65, ldh=65 * 32) == -2 and b"65 fields" in err()   # F 65
        assert call(S_=1, Dn=0, D_=33, stride=36, gs=36, lda=1, ldh=0) == -2 and b"dim 33" in err()                    # D 33
        assert call(stride=80) == -1 and b"row_stride" in err()
    for call in (pool, inter, attn, bwd):
        assert call(lda=80) == -1 and b"ld_attn 80 < fields^2 81" in err()
        assert call(ids=None) == -1 and b"null pointer" in err()
        assert call(W=None) == -1 and call(dense=None) == -1 and call(dw=None) == -1
        assert call(B=0, ids=None, W=None) == 0                                  # an empty batch launches nothing
    for call in (inter, attn, bwd):
        assert call(ldh=323) == -1 and b"ld_pair 323 < pairs x dim 324" in err()
        assert call(a=None) == -1 and b"null pointer" in err()
    assert pool(out=None) == -1 and inter(H=None) == -1 and inter(y1=None) == -1
    assert attn(dH=None) == -1 and attn(dz=None) == -1 and attn(out=None) == -1
    assert bwd(dH=None) == -1 and bwd(dz=None) == -1 and bwd(dp=None) == -1 and bwd(rg=None) == -1
    assert bwd(ddw=None) == -1 and bwd(ws=None) == -1
    assert bwd(gs=80) == -1 and b"grad_stride" in err()
    # the planning query: one [Dn, R] partial per block of the persistent grid (at most 2 per CU, one per sample)
    assert wsb() == 0 and n.value == 4 * 3 * 81 * 4
    assert wsb(B=100000) == 0 and n.value == 512 * 3 * 81 * 4
    assert wsb(B=0) == 0 and n.value == 0
    assert L.rec_fatffm_bwd_workspace_bytes(desc(), None) == -1 and L.rec_fatffm_bwd_workspace_bytes(None, C.byref(n)) == -1
    assert bwd(ws_bytes=4 * 3 * 81 * 4 - 1) == -3 and b"workspace" in err()
    assert L.rec_fatffm_pool_fwd(None, p, p, p, p, p, p, None) == -1 and b"null desc" in err()


def test_fatffm_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    check_entry_points_reject_bad_arguments(engine_lib)
