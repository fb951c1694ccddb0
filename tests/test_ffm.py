"""rank/ffm (paddlerec_amd/ffm.py; reference: models/rank/ffm/net.py, ffm/dygraph_model.py).

tests/ffm_ref.py is pinned to tests/golden/ffm_D9.npz (the reference's unmodified net.py over the paddle shim,
tools/make_golden_ffm.py).  The host mirror is checked against golden + a NumPy Adam trainer with the ffm_ref-backed
operator backend on the CPU (orchestration only; tests/ffm_cpu_kernels.py) and with the HIP kernels (`-m gpu`)."""
import os

import numpy as np
import pytest
import torch

import ffm_ref
from helpers import assert_adam_weights_close, assert_sibling_moments, load_golden
from oracle import deepfm_ref as R

S, DN, D = 26, 13, 9
F = S + DN
RW = F * D                  # 351
RP = (RW + 3) // 4 * 4      # 352


def _params(g):
    return {k: g[k].copy() for k in ("W", "W1", "dense_w", "dense_w_one", "bias")}


def _state_dict(p):
    return {"ffm.embedding.weight": p["W"], "ffm.embedding_one.weight": p["W1"], "ffm.dense_w": p["dense_w"],
            "ffm.dense_w_one": p["dense_w_one"], "bias": p["bias"]}


def _merged(o, key, N, width):
    uniq, merged, _ = R.merge_rows(o["rows"], o["row_valid"], o[key].astype(np.float32))
    out = np.zeros((N, width), np.float32)
    out[uniq] = merged
    return out


def test_ffm_ref_matches_reference_golden():
    g = load_golden("ffm_D9")
    assert g["W"].shape[1] == RW and g["dense_w"].shape == (1, DN, RW)
    o = ffm_ref.loss_and_grads(g["ids"], g["dense"], g["label"], _params(g), D)
    np.testing.assert_allclose(o["y1"], g["y1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o["y2"], g["y2"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o["pred"], g["pred"], rtol=1e-6)
    np.testing.assert_allclose(o["loss"], g["loss"], rtol=1e-6)
    np.testing.assert_allclose(o["d_bias"], g["g_bias"], rtol=1e-5)
    np.testing.assert_allclose(o["d_dense_w"].reshape(g["g_dense_w"].shape), g["g_dense_w"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(o["d_dense_w_one"], g["g_dense_w_one"], rtol=1e-5, atol=1e-7)
    N = g["W"].shape[0]
    np.testing.assert_allclose(_merged(o, "row_grad", N, RW), g["gW"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(_merged(o, "row_grad1", N, 1), g["gW1"], rtol=1e-5, atol=1e-7)
    assert (g["ids"] == 0).any() and len(np.unique(g["ids"])) < g["ids"].size     # id 0 + duplicates
    assert np.abs(g["gW"][0]).max() > 0          # ffm/net.py:59-75: no padding_idx — row 0 is looked up and trained


class _NumpyFFMTrainer:
    """Adam on the padded table [N, RP] (the pad column's gradient is 0) — lazy or the dygraph default."""

    def __init__(self, p, lr, lazy):
        N = p["W"].shape[0]
        W = np.zeros((N, RP), np.float32)
        W[:, :RW] = p["W"]
        self.p = dict(p, W=W)
        self.p = {k: np.array(v, np.float32) for k, v in self.p.items()}
        self.lr, self.step, self.lazy = lr, 0, lazy
        self.st = {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in self.p.items()}

    def train_step(self, ids, dense, label):
        self.step += 1
        o = ffm_ref.loss_and_grads(ids, dense, label, self.p, D)
        # dloss/dlogit in float32, as the engine's sigmoid_logloss forms it, then the backward from that dz
        p32, t = o["pred"].astype(np.float32), label.astype(np.float32)
        e = np.float32(ffm_ref.LOG_EPS)
        dz = ((-t / (p32 + e) + (1 - t) / (1 - p32 + e)) / np.float32(len(ids))) * (p32 * (1 - p32))
        o["row_grad"], o["d_dense_w"], o["d_dense_w_one"] = ffm_ref.backward(ids, dense, self.p, D, dz, RP)
        o["row_grad1"] = np.repeat(dz.reshape(-1), S).reshape(-1, 1)
        o["d_bias"] = dz.sum(dtype=np.float32).reshape(1)
        upd = R.adam_update_rows if self.lazy else R.adam_update_dense_equivalent
        for key, gk in (("W", "row_grad"), ("W1", "row_grad1")):
            uniq, merged, _ = R.merge_rows(o["rows"], o["row_valid"], o[gk].astype(np.float32))
            upd(self.p[key], self.st[key][0], self.st[key][1], uniq, merged, self.step, lr=self.lr)
        for key, gr in (("dense_w", o["d_dense_w"]), ("dense_w_one", o["d_dense_w_one"]), ("bias", o["d_bias"])):
            R.adam_update(self.p[key], self.st[key][0], self.st[key][1],
                          gr.reshape(self.p[key].shape).astype(np.float32), self.step, lr=self.lr)
        return o["loss"], o["pred"]


def check_layer(device, kernels, tol, lazy):
    from paddlerec_amd.ffm import FFMLayer
    rtol = tol
    g = load_golden("ffm_D9")
    N = g["W"].shape[0]
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    m = FFMLayer(N, D, DN, F, device=device, kernels=kernels)
    m.lazy_mode = lazy
    assert float(m.dense.p["ffm.dense_w"].min()) == 1.0 and float(m.dense.p["ffm.dense_w_one"].max()) == 1.0
    assert float(m.dense.p["bias"]) == 0.0 and m.emb_table.shape == (N, RP)
    assert float(m.emb_table[:, RW:].abs().max()) == 0.0
    std = 0.1 / np.sqrt(D)
    assert float(m.embedding.abs().max()) <= 2 * std + 1e-7                  # TruncatedNormal cut at 2 sigma
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "ffm.embedding.weight": (N, RW), "ffm.embedding_one.weight": (N, 1), "ffm.dense_w_one": (DN,),
        "ffm.dense_w": (1, DN, RW), "bias": (1,)}
    m.set_dict(_state_dict(_params(g)))
    sparse_inputs = [T(g["ids"][:, s:s + 1]) for s in range(S)]             # the reference's list of [B,1]
    pred = m.forward(sparse_inputs, T(g["dense"]))
    np.testing.assert_allclose(pred.cpu().numpy(), g["pred"], rtol=rtol)
    tr = _NumpyFFMTrainer(_params(g), lr=1e-2, lazy=lazy)
    rng = np.random.default_rng(3)
    for step in range(3):
        ids = rng.integers(0, N, (48, S), dtype=np.int64)
        ids[:, 0] = 0                                                         # heavy duplicates on row 0
        dense = rng.random((48, DN), dtype=np.float32)
        label = (rng.random((48, 1)) < 0.4).astype(np.int64)
        loss, pred = m.train_step(T(ids), T(dense), T(label), lr=1e-2)
        ol, op = tr.train_step(ids, dense, label)
        np.testing.assert_allclose(loss.cpu().numpy()[0], ol, rtol=rtol)
        np.testing.assert_allclose(pred.cpu().numpy(), op, rtol=rtol, atol=1e-6)
    assert int(m.status.item()) == 0
    assert float(m.emb_table[:, RW:].abs().max()) == 0.0                           # the pad column never moves
    assert float(m.sparse_state["m"][:, RW:].abs().max()) == 0.0
    assert float(m.sparse_state["v"][:, RW:].abs().max()) == 0.0
    got = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for k, ok in (("ffm.embedding.weight", "W"), ("ffm.embedding_one.weight", "W1"), ("ffm.dense_w", "dense_w"),
                  ("ffm.dense_w_one", "dense_w_one"), ("bias", "bias")):
        want = tr.p[ok][:, :RW] if ok == "W" else tr.p[ok]
        assert_adam_weights_close(got[k], want, lr=1e-2, steps=3, err_msg=k)
    # moments at 3e-5 of their scale: an element of d_dense_w sums 48 samples' products of cancelling signs over a
    # 351-wide cube, fp32 noise of the terms
    assert assert_sibling_moments(m, tr.st, rel=3e-5) >= 3
    return m


@pytest.mark.parametrize("lazy", [True, False])
def test_ffm_layer_host_logic_cpu_backend(lazy):
    import ffm_cpu_kernels
    check_layer("cpu", ffm_cpu_kernels, 1e-6, lazy)


def test_ffm_dygraph_model_plugin_surface():
    import ffm_cpu_kernels
    from paddlerec_amd.ffm import DygraphModel
    g = load_golden("ffm_D9")
    N = g["W"].shape[0]
    dm = DygraphModel()
    cfg = {"hyper_parameters.sparse_feature_number": N, "hyper_parameters.sparse_feature_dim": D,
           "hyper_parameters.dense_input_dim": DN, "hyper_parameters.sparse_inputs_slots": S + 1,
           "hyper_parameters.optimizer.learning_rate": 0.001}
    net = dm.create_model(cfg, "cpu", kernels=ffm_cpu_kernels)
    assert net.sparse_num_field == F and net.embedding.shape == (N, RW)      # dygraph_model.py:31-32
    net.set_dict(_state_dict(_params(g)))
    metrics, names = dm.create_metrics("cpu")
    batch = [g["label"]] + [g["ids"][:, s:s + 1] for s in range(S)] + [g["dense"]]   # the reference's 28 arrays
    assert len(batch) == 28
    metrics, _ = dm.infer_forward(net, metrics, batch, cfg)
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == len(g["label"])
    loss, metrics, _ = dm.train_forward(net, metrics, batch, cfg)
    np.testing.assert_allclose(float(loss.reshape(-1)[0]), float(g["loss"]), rtol=1e-6)   # loss of the pre-step net
    assert names == ["auc"] and int(metrics[0][0].sum() + metrics[0][1].sum()) == 2 * len(g["label"])


def test_trainer_knows_ffm(tmp_path):
    from paddlerec_amd import trainer
    assert "ffm" in trainer.MODELS
    d = tmp_path / "models" / "rank" / "ffm"
    d.mkdir(parents=True)
    assert trainer.guess_model(str(d / "config.yaml")) == "ffm"
    from paddlerec_amd.ffm import DygraphModel
    assert isinstance(trainer._dygraph_model("ffm"), DygraphModel)


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
  infer_batch_size: 20
  infer_load_path: "{out}"
  infer_start_epoch: 0
  infer_end_epoch: 2
hyper_parameters:
  optimizer:
    class: Adam
    learning_rate: 0.01
    strategy: async
    lazy_mode: {lazy}
  sparse_inputs_slots: 27
  sparse_feature_number: 30011
  sparse_feature_dim: 9
  dense_input_dim: 13
"""


def _slot_lines(n=80, seed=11):
    """Slot-text lines in the format of the reference's Criteo sample data (criteo_reader.py:60-91): a small id range
    so that rows repeat across batches, a few missing slots (-> id 0, an ordinary row for ffm)."""
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


def run_trainer_loops(tmp_path, device, kernels, lazy):
    """train (2 epochs, a checkpoint each) -> infer over both checkpoints -> a fresh model loaded from the last
    checkpoint predicts exactly like the trained net; the checkpoint holds the reference's keys and shapes."""
    import pickle

    from paddlerec_amd import checkpoint, trainer
    d = tmp_path / "models" / "rank" / "ffm"
    (d / "data" / "train").mkdir(parents=True)
    (d / "data" / "train" / "part-0").write_text("\n".join(_slot_lines()) + "\n")
    (d / "config.yaml").write_text(YAML.format(out=str(tmp_path / "out"), lazy=str(lazy)))
    cfg = trainer.load_yaml(str(d / "config.yaml"))
    model = trainer.guess_model(str(d / "config.yaml"))
    assert model == "ffm"
    s, net = trainer.train(cfg, model, device, kernels)
    assert net.lazy_mode is lazy
    assert [x["epoch"] for x in s] == [0, 1] and all(x["batches"] == 5 and x["samples"] == 80 for x in s)
    assert all(np.isfinite(x["loss"]) and 0.0 <= x["auc"] <= 1.0 for x in s)
    with open(os.path.join(s[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "ffm.embedding.weight": (30011, RW), "ffm.embedding_one.weight": (30011, 1), "ffm.dense_w_one": (DN,),
        "ffm.dense_w": (1, DN, RW), "bias": (1,)}
    r = trainer.infer(cfg, model, device, kernels)
    assert [x["epoch"] for x in r] == [0, 1] and all(0.0 <= x["auc"] <= 1.0 and x["samples"] == 80 for x in r)
    dm = trainer._dygraph_model(model)
    fresh = dm.create_model(cfg, device, **({"kernels": kernels} if kernels is not None else {}))
    checkpoint.load_model(s[-1]["model_dir"], fresh)
    for k, v in net.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    assert fresh.step_count == net.step_count
    assert torch.equal(fresh.sparse_state["m"].cpu(), net.sparse_state["m"].cpu())
    ids = torch.as_tensor(np.random.default_rng(0).integers(0, 30011, (7, S)), device=device)
    dense = torch.rand(7, DN, device=device)
    assert torch.equal(fresh.forward(ids, dense).cpu(), net.forward(ids, dense).cpu())
    return s, r


@pytest.mark.parametrize("lazy", [True, False])
def test_train_checkpoint_infer_cpu_backend(tmp_path, lazy):
    import ffm_cpu_kernels
    run_trainer_loops(tmp_path, "cpu", ffm_cpu_kernels, lazy)


REF_FFM = "/root/reference/models/rank/ffm"


@pytest.mark.skipif(not os.path.isdir(REF_FFM), reason="reference tree not mounted (only in the build container)")
def test_reference_yaml_and_sample_data_run_unchanged(tmp_path):
    """The reference's OWN ffm/config.yaml and sample data drive the loops as they are (bs 2, D 9, 1000001 rows) —
    only the output directory and the number of epochs are redirected, and the stand-in's Adam is the lazy one (a
    NumPy pass over the whole 1.4 GB table per step would take minutes on the host)."""
    import ffm_cpu_kernels
    from paddlerec_amd import trainer
    yaml_path = os.path.join(REF_FFM, "config.yaml")
    cfg = trainer.load_yaml(yaml_path, ["runner.epochs=1", "runner.model_save_path=" + str(tmp_path / "out"),
                                        "runner.infer_load_path=" + str(tmp_path / "out"),
                                        "runner.infer_start_epoch=0", "runner.infer_end_epoch=1",
                                        "hyper_parameters.optimizer.lazy_mode=True"])
    assert trainer.guess_model(yaml_path) == "ffm"
    s, net = trainer.train(cfg, "ffm", "cpu", ffm_cpu_kernels)
    assert len(s) == 1 and np.isfinite(s[0]["loss"]) and 0.0 <= s[0]["auc"] <= 1.0
    assert s[0]["samples"] > 0 and s[0]["samples"] % cfg["runner.train_batch_size"] == 0
    assert int(net.status.item()) == 0
    r = trainer.infer(cfg, "ffm", "cpu", ffm_cpu_kernels)
    assert r[0]["samples"] > 0 and 0.0 <= r[0]["auc"] <= 1.0
