"""rank/deepfefm (paddlerec_amd/deepfefm.py; reference: models/rank/deepfefm/net.py, deepfefm/dygraph_model.py).

tests/deepfefm_ref.py is pinned to tests/golden/deepfefm_D9.npz (the reference's unmodified net.py over the paddle shim,
tools/make_golden_deepfefm.py).  The host mirror is checked against the fixture and the restatement with the
deepfefm_ref-backed operator backend on the CPU (orchestration only; tests/deepfefm_cpu_kernels.py) and with the HIP
kernels (`-m gpu`, tests/test_deepfefm_gpu.py)."""
import os
import pickle

import numpy as np
import pytest
import torch

import deepfefm_ref as FR
from helpers import assert_close_scaled, load_golden

S, DN, D = 26, 13, 9
F = S + DN
P = F * (F - 1) // 2        # 741
N_FULL = 1100005
FE_KEY = "fefm.field_embeddings"


def _golden():
    g = load_golden("deepfefm_D9")
    n = len(g["fc"]) + 1
    p = {"W": g["W"], "W1": g["W1"], "dense_w_one": g["dense_w_one"], "FE": g["FE"],
         "lin_w": [g["lin_w%d" % i] for i in range(n)], "lin_b": [g["lin_b%d" % i] for i in range(n)]}
    return g, p


def _state_dict(p, bias=None):
    sd = {"fefm.embedding.weight": p["W"], "fefm.embedding_one.weight": p["W1"], "fefm.dense_w_one": p["dense_w_one"],
          FE_KEY: p["FE"]}
    for i, (w, b) in enumerate(zip(p["lin_w"], p["lin_b"])):
        sd["dnn.linear_%d.weight" % i], sd["dnn.linear_%d.bias" % i] = w, b
    if bias is not None:
        sd["bias"] = bias
    return sd


def test_deepfefm_ref_matches_reference_golden():
    g, p = _golden()
    assert g["ids"].shape[1] == S and g["dense"].shape[1] == DN and g["FE"].shape == (P, D, D)
    assert (g["ids"] == 0).any() and len(np.unique(g["ids"])) < g["ids"].size        # padding ids + duplicates
    o = FR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D)
    assert np.array_equal(o["ids_all"][:, S:], g["dense_ids"])
    assert g["dense_ids"].min() >= 2 and g["dense_ids"].max() < g["W"].shape[0]
    for k in ("pred", "loss", "y1", "y2", "t", "gW", "gW1", "g_dense_w_one", "gFE"):
        assert_close_scaled(o[k], g[k], 1e-5, k)
    for i in range(len(p["lin_w"])):
        assert_close_scaled(o["g_lin_w"][i], g["g_lin_w%d" % i], 1e-5, "g_lin_w%d" % i)
        assert_close_scaled(o["g_lin_b"][i], g["g_lin_b%d" % i], 1e-5, "g_lin_b%d" % i)
    assert not g["gW"][0].any() and not g["gW1"][0].any()                               # padding_idx = 0
    assert np.abs(g["gFE"]).max() > 0        # autograd reaches the pair matrices although the module does not register them
    # the float32 restatement (what the D 48 bound of the GPU test is measured with) agrees at float32 level
    o32 = FR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D, torch.float32)
    assert_close_scaled(o32["gFE"], o["gFE"], 1e-5, "gFE f32")


def test_derived_ids_are_three_rounded_f32_operations():
    """A guard on the ORACLE only (deepfefm_ref.derived_ids, numpy): it rounds three times, and on uniform values that
    differs from a contracted multiply-add on a few values per thousand, so the comparison the GPU test makes
    (tests/test_deepfefm_gpu.py: the kernel's ids against this function, exactly) can tell the two apart.  No code of
    the engine runs here."""
    d = np.random.default_rng(0).random(2000000, dtype=np.float32)
    d[0], d[-1] = 0.0, 1.0
    want = FR.derived_ids(d.reshape(-1, 1)).reshape(-1)
    # multiply and first add contracted into one FMA (one rounding of the exact d * 1e5 + 1e6), then + 2
    one_fma = ((d.astype(np.float64) * 1e5 + 1e6).astype(np.float32) + np.float32(2)).astype(np.int64)
    assert 1000 < (want != one_fma).sum() < len(d) // 100   # a few thousand values land on another row
    assert want[0] == 1000002 and want[-1] == 1100002 and want.max() < N_FULL


def _merge(rows, grads, N, width):
    out = np.zeros((N, width), np.float64)
    for r, gr in zip(rows.reshape(-1), grads.reshape(len(rows.reshape(-1)), -1)):
        if r != 0:
            out[r] += gr[:width]
    return out


def check_layer_on_fixture(device, kernels, rel):
    """Forward = the fixture's pred; one train_step (eval arithmetic: dropout_rate 0, pair matrices trained so that
    d_FE is produced) leaves the fixture's gradients in the layer's buffers, L2 terms on top."""
    from paddlerec_amd.deepfefm import DeepFEFMLayer, L2_DNN, L2_EMB
    g, p = _golden()
    N = g["W"].shape[0]
    fc = [int(x) for x in g["fc"]]
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    kw = {"kernels": kernels} if kernels is not None else {}
    m = DeepFEFMLayer(N, D, DN, S, fc, device=device, train_field_embeddings=True, **kw)
    std = 0.1 / np.sqrt(D)
    assert float(m.embedding.abs().max()) <= 2 * std + 1e-7 and not m.emb_table[0].any()
    assert float(m.dense.p[FE_KEY].abs().max()) <= 2 * std + 1e-7 and float(m.dense.p["bias"]) == 0.0
    assert m.emb_table.shape == (N, 12) and m.input_size == S * D + DN + P == 988
    m.set_dict(_state_dict(p, bias=g["bias"]))
    sparse_inputs = [T(g["ids"][:, s:s + 1]) for s in range(S)]             # the reference's list of [B,1]
    pred = m.forward(sparse_inputs, T(g["dense"]))
    assert_close_scaled(pred.cpu().numpy(), g["pred"], rel, "pred")
    loss, pred2 = m.train_step(sparse_inputs, T(g["dense"]), T(g["label"]), lr=1e-9)
    assert int(m.status.item()) == 0
    assert_close_scaled(float(loss), g["loss"], rel, "loss")
    assert_close_scaled(pred2.cpu().numpy(), g["pred"], rel, "pred (train_step)")
    gd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.grad_dict().items()}
    assert_close_scaled(gd["fefm.dense_w_one"] - L2_EMB * g["dense_w_one"], g["g_dense_w_one"], rel, "g dense_w_one")
    assert_close_scaled(gd[FE_KEY] - L2_DNN * g["FE"], g["gFE"], rel, "g FE")
    for i in range(len(fc) + 1):
        assert_close_scaled(gd["dnn.linear_%d.weight" % i] - L2_DNN * g["lin_w%d" % i], g["g_lin_w%d" % i], rel, "gw%d" % i)
        assert_close_scaled(gd["dnn.linear_%d.bias" % i], g["g_lin_b%d" % i], rel, "gb%d" % i)
    assert not gd["bias"].any()                                               # never used by forward: no gradient
    last = m._last
    ia = last["ids_all"].cpu().numpy()
    assert np.array_equal(ia[:, S:], g["dense_ids"]) and np.array_equal(ia[:, :S], g["ids"])
    rg = last["row_grad"].cpu().numpy()
    assert not rg[:, D:].any()
    assert_close_scaled(_merge(ia, rg, N, D), g["gW"], rel, "gW")
    dz = last["dz"].cpu().numpy().reshape(-1, 1)
    assert_close_scaled(_merge(g["ids"], np.repeat(dz, S, axis=1).reshape(-1, 1), N, 1), g["gW1"], rel, "gW1")
    return m


def test_layer_host_logic_cpu_backend_matches_fixture():
    import deepfefm_cpu_kernels
    check_layer_on_fixture("cpu", deepfefm_cpu_kernels, 1e-5)


def _small_batch(rng, N, B=24):
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    ids[:, 0] = 5
    dense = (np.float32(-10.0) + rng.random((B, DN), dtype=np.float32) * np.float32(1e-3)).astype(np.float32)
    label = (rng.random((B, 1)) < 0.4).astype(np.int64)
    return ids, dense, label


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("train_fe", [False, True])
def test_state_dict_bias_and_field_embeddings(lazy, train_fe):
    """The reference's keys + fefm.field_embeddings; `bias` never moves; the frozen default leaves the pair matrices
    bit-identical, train_field_embeddings=True moves them; a dict without the extra key keeps the current matrices; the
    trajectory equals the restatement's (dropout on)."""
    import deepfefm_cpu_kernels
    from paddlerec_amd.deepfefm import DeepFEFMLayer
    g, p = _golden()
    N, fc = g["W"].shape[0], [int(x) for x in g["fc"]]
    m = DeepFEFMLayer(N, D, DN, S, fc, device="cpu", kernels=deepfefm_cpu_kernels, dropout_rate=0.2, dropout_seed=31,
                      train_field_embeddings=train_fe)
    m.lazy_mode = lazy
    want_keys = {"bias": (1,), "fefm.dense_w_one": (DN,), "fefm.embedding_one.weight": (N, 1),
                 "fefm.embedding.weight": (N, D), FE_KEY: (P, D, D)}
    sizes = [988] + fc + [1]
    for i in range(len(fc) + 1):
        want_keys["dnn.linear_%d.weight" % i] = (sizes[i], sizes[i + 1])
        want_keys["dnn.linear_%d.bias" % i] = (sizes[i + 1],)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want_keys
    assert len(want_keys) == 10 + 2 * (len(fc) - 2) + 1      # the reference's 10 + 2 per extra Linear, + the extra key
    drawn = m.dense.p[FE_KEY].clone()
    sd = _state_dict(p, bias=g["bias"])
    del sd[FE_KEY]
    m.set_dict(sd)                                            # a checkpoint of the reference: no pair matrices
    assert torch.equal(m.dense.p[FE_KEY], drawn)
    m.set_dict({FE_KEY: p["FE"]})
    tr = FR.Trainer(p, D, lazy=lazy, train_fe=train_fe, rate=0.2, seed=31)
    rng = np.random.default_rng(8)
    T = torch.as_tensor
    for step in range(3):
        ids, dense, label = _small_batch(rng, N)
        loss, pred = m.train_step(T(ids), T(dense), T(label), lr=1e-2)
        ol, op = tr.train_step(ids, dense, label, lr=1e-2)
        np.testing.assert_allclose(float(loss), ol, rtol=1e-5)
        np.testing.assert_allclose(pred.numpy(), op, rtol=1e-5, atol=1e-6)
    assert int(m.status.item()) == 0
    assert float(m.dense.p["bias"]) == float(g["bias"][0])                    # in the state_dict, never moves
    fe = m.dense.p[FE_KEY]
    if train_fe:
        assert not torch.equal(fe, T(p["FE"])) and float((fe - T(p["FE"])).abs().max()) > 1e-3
    else:
        assert torch.equal(fe, T(p["FE"]))                                    # bit-identical after N steps
    assert not m.emb_table[0].any() and not m.embedding_one[0].any() and not m.emb_table[:, D:].any()


def test_frozen_matrices_ignore_loaded_moments(tmp_path):
    """A checkpoint of a run that trained the pair matrices carries non-zero Adam moments for them.  Loaded with its
    optimizer state into a frozen model they must not move: frozen means Adam never visits them, not that their
    gradient happens to be zero."""
    import deepfefm_cpu_kernels
    from paddlerec_amd import checkpoint
    from paddlerec_amd.deepfefm import DeepFEFMLayer
    g, p = _golden()
    N, fc = g["W"].shape[0], [int(x) for x in g["fc"]]
    mk = lambda tfe: DeepFEFMLayer(N, D, DN, S, fc, device="cpu", kernels=deepfefm_cpu_kernels, dropout_rate=0.2,
                                   dropout_seed=31, train_field_embeddings=tfe)
    a = mk(True)
    a.set_dict(_state_dict(p, bias=g["bias"]))
    rng = np.random.default_rng(4)
    T = torch.as_tensor
    for _ in range(2):
        ids, dense, label = _small_batch(rng, N)
        a.train_step(T(ids), T(dense), T(label), lr=1e-2)
    assert float(a.dense.pm[FE_KEY].abs().max()) > 0 and float(a.dense.pv[FE_KEY].abs().max()) > 0
    checkpoint.save_model(a, None, str(tmp_path), 0)
    b = mk(False)
    checkpoint.load_model(os.path.join(str(tmp_path), "0"), b)
    assert torch.equal(b.dense.pm[FE_KEY], a.dense.pm[FE_KEY]) and b.step_count == 2
    fe0 = b.dense.p[FE_KEY].clone()
    assert torch.equal(fe0, a.dense.p[FE_KEY])
    w0 = b.dense.p["dnn.linear_0.weight"].clone()
    for _ in range(2):
        ids, dense, label = _small_batch(rng, N)
        b.train_step(T(ids), T(dense), T(label), lr=1e-2)
    assert torch.equal(b.dense.p[FE_KEY], fe0)                                # bit-identical
    assert torch.equal(b.dense.pm[FE_KEY], a.dense.pm[FE_KEY])                # and their moments untouched
    assert not torch.equal(b.dense.p["dnn.linear_0.weight"], w0)             # the rest trains


def test_dygraph_model_plugin_surface():
    import deepfefm_cpu_kernels
    from paddlerec_amd.deepfefm import DygraphModel
    g, p = _golden()
    N = g["W"].shape[0]
    dm = DygraphModel()
    cfg = {"hyper_parameters.sparse_feature_number": N, "hyper_parameters.sparse_feature_dim": D,
           "hyper_parameters.dense_input_dim": DN, "hyper_parameters.sparse_inputs_slots": S + 1,
           "hyper_parameters.fc_sizes": [int(x) for x in g["fc"]], "hyper_parameters.optimizer.learning_rate": 0.001}
    net = dm.create_model(cfg, "cpu", kernels=deepfefm_cpu_kernels)
    assert net.sparse_num_field == S and net.num_fields == F and net.dropout_rate == 0.2
    assert net.train_field_embeddings is False
    assert dm.create_model(dict(cfg, **{"hyper_parameters.train_field_embeddings": True}), "cpu",
                           kernels=deepfefm_cpu_kernels).train_field_embeddings is True
    net.set_dict(_state_dict(p))
    metrics, names = dm.create_metrics("cpu")
    batch = [g["label"]] + [g["ids"][:, s:s + 1] for s in range(S)] + [g["dense"]]   # the reference's 28 arrays
    metrics, _ = dm.infer_forward(net, metrics, batch, cfg)                  # eval mode: the fixture's arithmetic
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == len(g["label"])
    pred = net.forward([torch.as_tensor(b) for b in batch[1:-1]], torch.as_tensor(g["dense"]))
    assert_close_scaled(pred.numpy(), g["pred"], 1e-5, "pred")
    loss, metrics, _ = dm.train_forward(net, metrics, batch, cfg)            # train mode: dropout on
    assert np.isfinite(float(loss)) and names == ["auc"]


def test_trainer_knows_deepfefm(tmp_path):
    from paddlerec_amd import trainer
    assert "deepfefm" in trainer.MODELS
    d = tmp_path / "models" / "rank" / "deepfefm"
    d.mkdir(parents=True)
    assert trainer.guess_model(str(d / "config.yaml")) == "deepfefm"
    assert trainer.guess_model(str(d / "config_bigdata.yaml")) == "deepfefm"
    from paddlerec_amd.deepfefm import DygraphModel
    assert isinstance(trainer._dygraph_model("deepfefm"), DygraphModel)


YAML = """
runner:
  train_data_dir: "data/train"
  train_reader_path: "criteo_reader"
  use_gpu: False
  use_auc: True
  train_batch_size: 16
  epochs: 2
  print_interval: 2
  model_save_path: "{out}"
  test_data_dir: "data/train"
  infer_batch_size: 16
  infer_load_path: "{out}"
  infer_start_epoch: 0
  infer_end_epoch: 2
hyper_parameters:
  optimizer:
    class: Adam
    learning_rate: 0.001
    strategy: async
    lazy_mode: {lazy}
  sparse_inputs_slots: 27
  sparse_feature_number: {rows}
  sparse_feature_dim: 9
  dense_input_dim: 13
  fc_sizes: [32, 16]
"""


def _slot_lines(n=32, seed=11):
    """Slot-text lines in the format of the reference's Criteo sample data (criteo_reader.py): dense values in [0, 1) as
    the reader clamps them (their derived ids start at 1 000 002), a small id range so that rows repeat across batches,
    a few missing slots (-> padding id 0)."""
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(n):
        parts = ["click:%d" % int(rng.random() < 0.4)]
        parts += ["dense_feature:%s" % repr(round(float(rng.random()), 6)) for _ in range(DN)]
        for slot in range(1, S + 1):
            if rng.random() < 0.04:
                continue
            parts.append("%d:%d" % (slot, int(rng.integers(1, 200)) + 1000 * slot))
        lines.append(" ".join(parts))
    return lines


def _write_run(tmp_path, lazy, rows):
    d = tmp_path / "models" / "rank" / "deepfefm"
    (d / "data" / "train").mkdir(parents=True)
    (d / "data" / "train" / "part-0").write_text("\n".join(_slot_lines()) + "\n")
    (d / "config.yaml").write_text(YAML.format(out=str(tmp_path / "out"), lazy=str(lazy), rows=rows))
    return str(d / "config.yaml")


def run_trainer_loops(tmp_path, device, kernels, lazy):
    """train (2 epochs of 2 batches, a checkpoint each) -> infer over both checkpoints -> a fresh model loaded from the
    last checkpoint predicts exactly like the trained net.  The table keeps the reference's 1 100 005 rows: the derived
    dense ids start at 1 000 002."""
    from paddlerec_amd import checkpoint, trainer
    path = _write_run(tmp_path, lazy, N_FULL)
    cfg = trainer.load_yaml(path)
    model = trainer.guess_model(path)
    assert model == "deepfefm"
    s, net = trainer.train(cfg, model, device, kernels)
    assert net.lazy_mode is lazy and net.dropout_rate == 0.2 and net.train_field_embeddings is False
    assert [x["epoch"] for x in s] == [0, 1] and all(x["batches"] == 2 and x["samples"] == 32 for x in s)
    assert all(np.isfinite(x["loss"]) and 0.0 <= x["auc"] <= 1.0 for x in s)
    assert int(net.status.item()) == 0
    with open(os.path.join(s[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "bias": (1,), "fefm.dense_w_one": (DN,), "fefm.embedding_one.weight": (N_FULL, 1),
        "fefm.embedding.weight": (N_FULL, D), "dnn.linear_0.weight": (988, 32), "dnn.linear_0.bias": (32,),
        "dnn.linear_1.weight": (32, 16), "dnn.linear_1.bias": (16,), "dnn.linear_2.weight": (16, 1),
        "dnn.linear_2.bias": (1,), FE_KEY: (P, D, D)}
    assert float(sd["bias"][0]) == 0.0
    r = trainer.infer(cfg, model, device, kernels)
    assert [x["epoch"] for x in r] == [0, 1] and all(0.0 <= x["auc"] <= 1.0 and x["samples"] == 32 for x in r)
    dm = trainer._dygraph_model(model)
    fresh = dm.create_model(cfg, device, **({"kernels": kernels} if kernels is not None else {}))
    assert not torch.equal(fresh.dense.p[FE_KEY].cpu(), net.dense.p[FE_KEY].cpu())      # a new draw ...
    checkpoint.load_model(s[-1]["model_dir"], fresh)                                     # ... replaced by the saved one
    for k, v in net.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    assert fresh.step_count == net.step_count == 4
    assert torch.equal(fresh.sparse_state["m"].cpu(), net.sparse_state["m"].cpu())
    rng = np.random.default_rng(0)
    ids = torch.as_tensor(rng.integers(0, 30000, (7, S)), device=device)
    dense = torch.as_tensor(rng.random((7, DN), dtype=np.float32), device=device)
    assert torch.equal(fresh.forward(ids, dense).cpu(), net.forward(ids, dense).cpu())
    return s, r


@pytest.mark.parametrize("lazy", [True, False])
def test_train_checkpoint_infer_cpu_backend(tmp_path, lazy):
    import deepfefm_cpu_kernels
    run_trainer_loops(tmp_path, "cpu", deepfefm_cpu_kernels, lazy)


def test_short_table_ends_with_the_status_flag(tmp_path):
    """30 011 rows cannot hold the derived dense ids (1 000 002 ..): the run must end with the out-of-range error of the
    status flag — not with an index error, and not silently on a wrong row."""
    import deepfefm_cpu_kernels
    from paddlerec_amd import trainer
    from paddlerec_amd._lib import RecError
    path = _write_run(tmp_path, True, 30011)
    cfg = trainer.load_yaml(path)
    with pytest.raises(RecError, match="outside"):
        trainer.train(cfg, "deepfefm", "cpu", deepfefm_cpu_kernels)


REF_DIR = "/root/reference/models/rank/deepfefm"


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason="reference tree not mounted (only in the build container)")
@pytest.mark.parametrize("name,dim,fc", [("config.yaml", 9, [512, 256, 128, 32]),
                                         ("config_bigdata.yaml", 48, [1024, 1024, 1024])])
def test_reference_yamls_build_the_model(name, dim, fc):
    """The reference's own YAML files select the model and give its shapes (the directory ships no sample data, so the
    loops run on written lines above)."""
    from paddlerec_amd import trainer
    path = os.path.join(REF_DIR, name)
    cfg = trainer.load_yaml(path)
    assert trainer.guess_model(path) == "deepfefm"
    assert cfg["hyper_parameters.sparse_feature_number"] == N_FULL and cfg["hyper_parameters.sparse_feature_dim"] == dim
    assert cfg["hyper_parameters.fc_sizes"] == fc and cfg["hyper_parameters.sparse_inputs_slots"] == S + 1
