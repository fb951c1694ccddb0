"""rank/dcn (paddlerec_amd/dcn.py; reference: models/rank/dcn/net.py, dcn/dygraph_model.py).

tests/dcn_ref.py is pinned to tests/golden/dcn_D9.npz (the reference's unmodified net.py over the paddle shim,
tools/make_golden_dcn.py: cross_num 3, a two-layer DNN, duplicate and padding ids, non-zero biases).  The host mirror is
checked against the fixture and the restatement with the dcn_ref-backed operator backend on the CPU (orchestration only;
tests/dcn_cpu_kernels.py) and with the HIP kernels (`-m gpu`, tests/test_dcn_gpu.py).  The argument checks of the three
rec_dcn_cross_* entry points run here too: they return before any launch."""
import logging
import os
import pickle

import numpy as np
import pytest
import torch

import dcn_ref as DR
from helpers import assert_adam_weights_close, assert_close_scaled, load_golden

S, DN, D = 26, 13, 9
WIDTH = S * D + DN          # 247
DATA_KEYS = ("ids", "dense", "label", "D", "fc", "cross_num", "pred", "l2", "loss", "cross_out")


def _golden():
    g = load_golden("dcn_D9")
    p = {k: g[k] for k in g if k not in DATA_KEYS and not k.startswith("g_")}
    return g, p, int(g["cross_num"])


def test_dcn_ref_matches_reference_golden():
    g, p, L = _golden()
    assert g["ids"].shape[1] == S and g["dense"].shape[1] == DN and L == 3 and p["layer_w"].shape == (WIDTH,)
    assert (g["ids"] == 0).any() and len(np.unique(g["ids"])) < g["ids"].size        # padding ids + duplicates
    assert all(np.abs(p[k]).max() > 0 for k in p if k.endswith(".bias"))             # a dropped bias term would show
    assert np.abs(g["dense"]).max() > 1.0 and g["dense"].min() < 0                    # raw values: no log1p
    o = DR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D, L)
    for k in ("pred", "l2", "loss", "cross_out"):
        assert_close_scaled(o[k], g[k], 1e-5, k)
    assert sorted(o["g"]) == sorted(p)
    for k in p:
        assert_close_scaled(o["g"][k], g["g_" + k], 1e-5, "g " + k)
    assert not g["g_embedding.weight"][0].any()                                       # padding_idx = 0
    # the l2 term is a batch SUM with coefficient 1: it is more than half of this fixture's loss
    assert float(g["l2"][0]) > 0.5 * float(g["loss"][0])
    # the closed form the backward kernel rebuilds x_l with: x_l = x_0 * (1 + s_0 + .. + s_{l-1}) + l * b
    f = DR.forward(g["ids"], g["dense"], p, D, L)
    for l in range(L + 1):
        A = 1.0 + f["s"][:, :l].sum(axis=1, keepdims=True)
        assert_close_scaled(f["feat"] * A + l * p["layer_b"].astype(np.float64), f["xs"][l], 1e-12, "x_%d" % l)


def _merge(ids, dfeat, N):
    out = np.zeros((N, D), np.float64)
    rows = dfeat[:, :S * D].reshape(-1, D)
    for r, gr in zip(ids.reshape(-1), rows):
        if r != 0:
            out[r] += gr
    return out


def check_layer_on_fixture(device, kernels, rel):
    """Forward = the fixture's pred; one train_step leaves the fixture's loss, l2 and gradients in the layer."""
    from paddlerec_amd.dcn import DeepCroLayer
    g, p, L = _golden()
    N = p["embedding.weight"].shape[0]
    fc = [int(x) for x in g["fc"]]
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    kw = {"kernels": kernels} if kernels is not None else {}
    m = DeepCroLayer(N, D, DN, S, fc, L, 100.0, 5e-5, False, device=device, **kw)
    std = 0.1 / np.sqrt(D)
    assert float(m.embedding.abs().max()) <= 2 * std + 1e-7 and not m.rec[0].any()
    assert float(m.dense.p["layer_w"].abs().max()) <= 2 * std + 1e-7 and float(m.dense.p["fc.bias"]) == 0.0
    assert m.rec.shape == (N, 32) and m.d == WIDTH and m.d_pad == 248
    assert (m.clip_by_norm, m.l2_reg_cross, m.is_sparse) == (100.0, 5e-5, False)      # stored, never used
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in p.items()}
    m.set_dict(p)
    sparse_inputs = [T(g["ids"][:, s:s + 1]) for s in range(S)]             # the reference's list of [B,1]
    pred = m.forward(sparse_inputs, T(g["dense"]))
    assert_close_scaled(pred.cpu().numpy(), g["pred"], rel, "pred")
    pred_l2, l2 = m.forward_with_l2(sparse_inputs, T(g["dense"]))
    assert_close_scaled(l2.cpu().numpy(), g["l2"], rel, "l2 (forward)")
    assert torch.equal(pred_l2.cpu(), pred.cpu())
    loss, pred2 = m.train_step(sparse_inputs, T(g["dense"]), T(g["label"]), lr=1e-9)
    assert int(m.status.item()) == 0
    assert_close_scaled(loss.cpu().numpy(), g["loss"], rel, "loss")
    assert_close_scaled(m.last_losses[1].cpu().numpy(), g["l2"], rel, "l2")
    assert_close_scaled(pred2.cpu().numpy(), g["pred"], rel, "pred (train_step)")
    gd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.grad_dict().items()}
    assert sorted(gd) == sorted(k for k in p if k != "embedding.weight")
    for k in gd:
        assert_close_scaled(gd[k], g["g_" + k], rel, "g " + k)
    dfeat = m._last_dfeat.cpu().numpy()
    assert dfeat.shape == (len(g["ids"]), WIDTH)
    assert_close_scaled(_merge(g["ids"], dfeat, N), g["g_embedding.weight"], rel, "g embedding.weight")
    return m


def test_layer_host_logic_cpu_backend_matches_fixture():
    import dcn_cpu_kernels
    check_layer_on_fixture("cpu", dcn_cpu_kernels, 1e-5)


def test_state_dict_keys_are_the_references():
    import dcn_cpu_kernels
    from paddlerec_amd.dcn import DeepCroLayer
    g, p, L = _golden()
    m = DeepCroLayer(301, D, DN, S, [16, 8], L, device="cpu", kernels=dcn_cpu_kernels)
    assert sorted(m.state_dict()) == sorted(p) == sorted(
        ["layer_w", "layer_b", "embedding.weight", "linear_0.weight", "linear_0.bias", "linear_1.weight", "linear_1.bias",
         "fc.weight", "fc.bias"])
    # fc.weight: Normal(std 1 / sqrt(H + 26 + 13)) — the field count, not S*D (net.py:100-104)
    big = DeepCroLayer(11, D, DN, S, [512, 256, 128], 2, device="cpu", kernels=dcn_cpu_kernels)
    fcw = big.dense.p["fc.weight"]
    assert tuple(fcw.shape) == (128 + WIDTH, 1)
    assert abs(float(fcw.std()) * np.sqrt(128 + S + DN) - 1.0) < 0.15
    assert abs(float(big.dense.p["linear_0.weight"].std()) * np.sqrt(WIDTH) - 1.0) < 0.05


def _small_batch(rng, N, B=24):
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    ids[:, 0] = 5                                                             # a hot row
    ids[::5, 3] = 0                                                           # padding ids
    dense = (rng.standard_normal((B, DN)) * 1.5).astype(np.float32)
    label = (rng.random((B, 1)) < 0.4).astype(np.int64)
    return ids, dense, label


def check_adam_trajectory(device, kernels, lazy, rtol):
    """Three steps against the plain restatement's trajectory (dcn_ref.Trainer): loss and prediction of every step,
    weights and table after the last."""
    from paddlerec_amd.dcn import DeepCroLayer
    g, p, L = _golden()
    N, fc = p["embedding.weight"].shape[0], [int(x) for x in g["fc"]]
    kw = {"kernels": kernels} if kernels is not None else {}
    m = DeepCroLayer(N, D, DN, S, fc, L, device=device, **kw)
    m.lazy_mode = lazy
    m.set_dict(p)
    tr = DR.Trainer(p, D, L, lazy=lazy)
    rng = np.random.default_rng(8)
    T = lambda a: torch.as_tensor(a).to(device)
    for step in range(3):
        ids, dense, label = _small_batch(rng, N)
        loss, pred = m.train_step(T(ids), T(dense), T(label), lr=1e-2)
        ol, op = tr.train_step(ids, dense, label, lr=1e-2)
        np.testing.assert_allclose(float(loss), ol, rtol=rtol)
        np.testing.assert_allclose(pred.cpu().numpy(), op, rtol=rtol, atol=1e-6)
    assert int(m.status.item()) == 0 and m.step_count == 3
    assert not m.rec[0].any() and not m.rec[:, D:].any()                       # padding row and pad columns never move
    for k, v in m.state_dict().items():
        assert_adam_weights_close(v.detach().cpu().numpy(), tr.p[k], lr=1e-2, steps=3, err_msg=k)
    assert_close_scaled(m.sparse_state["m"].cpu().numpy(), tr.m["embedding.weight"], 1e-5, "m of the table")
    assert_close_scaled(m.sparse_state["v"].cpu().numpy(), tr.v["embedding.weight"], 1e-5, "v of the table")
    return m


@pytest.mark.parametrize("lazy", [False, True])
def test_adam_trajectory_cpu_backend(lazy):
    import dcn_cpu_kernels
    check_adam_trajectory("cpu", dcn_cpu_kernels, lazy, 1e-5)


def test_dygraph_model_plugin_surface():
    import dcn_cpu_kernels
    from paddlerec_amd.dcn import DygraphModel
    g, p, L = _golden()
    N = p["embedding.weight"].shape[0]
    dm = DygraphModel()
    cfg = {"hyper_parameters.sparse_feature_number": N, "hyper_parameters.sparse_feature_dim": D,
           "hyper_parameters.dense_input_dim": DN, "hyper_parameters.sparse_inputs_slots": S + 1,
           "hyper_parameters.fc_sizes": [int(x) for x in g["fc"]], "hyper_parameters.cross_num": L,
           "hyper_parameters.l2_reg_cross": 0.00005, "hyper_parameters.clip_by_norm": 100.0,
           "hyper_parameters.is_sparse": False, "hyper_parameters.optimizer.learning_rate": 1e-9}
    net = dm.create_model(cfg, "cpu", kernels=dcn_cpu_kernels)
    assert net.sparse_num_field == S and net.cross_num == L and net.lazy_mode is False
    assert (net.l2_reg_cross, net.clip_by_norm, net.is_sparse) == (0.00005, 100.0, False)
    net.set_dict(p)
    metrics, names = dm.create_metrics("cpu")
    batch = [g["label"]] + [g["ids"][:, s:s + 1] for s in range(S)] + [g["dense"]]   # the reference's 28 arrays
    assert len(batch) == 28
    metrics, _ = dm.infer_forward(net, metrics, batch, cfg)
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == len(g["label"])
    loss, metrics, print_dict = dm.train_forward(net, metrics, batch, cfg)
    assert_close_scaled(float(loss), g["loss"], 1e-5, "loss")                # mean log-loss + l2 of the pre-step net
    assert names == ["auc"] and print_dict is None


def test_trainer_knows_dcn(tmp_path):
    from paddlerec_amd import trainer
    assert "dcn" in trainer.MODELS and "dcn_v2" in trainer.MODELS
    d = tmp_path / "models" / "rank" / "dcn"
    d.mkdir(parents=True)
    assert trainer.guess_model(str(d / "config.yaml")) == "dcn"
    assert trainer.guess_model(str(d / "config_bigdata.yaml")) == "dcn"
    from paddlerec_amd.dcn import DygraphModel
    assert isinstance(trainer._dygraph_model("dcn"), DygraphModel)


YAML = """
runner:
  train_data_dir: "data/sample_data"
  train_reader_path: "reader"
  use_gpu: False
  use_auc: True
  train_batch_size: 8
  epochs: 2
  print_interval: 2
  model_save_path: "{out}"
  test_data_dir: "data/sample_data"
  infer_reader_path: "reader"
  infer_batch_size: 8
  infer_load_path: "{out}"
  infer_start_epoch: 0
  infer_end_epoch: 2
hyper_parameters:
  optimizer:
    class: Adam
    learning_rate: 0.0001
    strategy: async
    lazy_mode: {lazy}
  sparse_inputs_slots: 27
  sparse_feature_number: 30011
  sparse_feature_dim: 9
  dense_input_dim: 13
  fc_sizes: [32, 16]
  distributed_embedding: 0
  cross_num: 2
  l2_reg_cross: 0.00005
  dnn_use_bn: False
  clip_by_norm: 100.0
  is_sparse: False
"""


def _slot_lines(n=32, seed=11):
    """Slot-text lines in the format of the reference's dcn/data/sample_data: a small id range so that rows repeat across
    batches, a few missing slots (-> padding id 0), dense values as the slot files hold them (the reader applies no
    log1p for this model)."""
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


def run_trainer_loops(tmp_path, device, kernels, lazy, caplog=None):
    """train (2 epochs of 4 batches, a checkpoint each) -> infer over both checkpoints -> a fresh model loaded from the
    last checkpoint predicts exactly like the trained net; the checkpoint holds the reference's keys and shapes."""
    from paddlerec_amd import checkpoint, trainer
    d = tmp_path / "models" / "rank" / "dcn"
    (d / "data" / "sample_data").mkdir(parents=True)
    (d / "data" / "sample_data" / "sample_train.txt").write_text("\n".join(_slot_lines()) + "\n")
    (d / "config.yaml").write_text(YAML.format(out=str(tmp_path / "out"), lazy=str(lazy)))
    cfg = trainer.load_yaml(str(d / "config.yaml"))
    model = trainer.guess_model(str(d / "config.yaml"))
    assert model == "dcn"
    if caplog is not None:
        caplog.set_level(logging.INFO, logger="paddlerec_amd.trainer")
    s, net = trainer.train(cfg, model, device, kernels)
    if caplog is not None:
        said = [r.getMessage() for r in caplog.records if "l2_reg_cross" in r.getMessage()]
        assert len(said) == 1 and "never used" in said[0] and "summed over the batch" in said[0]
    assert net.lazy_mode is lazy and net.cross_num == 2 and net.l2_reg_cross == 0.00005 and net.clip_by_norm == 100.0
    assert [x["epoch"] for x in s] == [0, 1] and all(x["batches"] == 4 and x["samples"] == 32 for x in s)
    assert all(np.isfinite(x["loss"]) and 0.0 <= x["auc"] <= 1.0 for x in s)
    assert int(net.status.item()) == 0
    with open(os.path.join(s[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "layer_w": (WIDTH,), "layer_b": (WIDTH,), "embedding.weight": (30011, D), "linear_0.weight": (WIDTH, 32),
        "linear_0.bias": (32,), "linear_1.weight": (32, 16), "linear_1.bias": (16,), "fc.weight": (16 + WIDTH, 1),
        "fc.bias": (1,)}
    r = trainer.infer(cfg, model, device, kernels)
    assert [x["epoch"] for x in r] == [0, 1] and all(0.0 <= x["auc"] <= 1.0 and x["samples"] == 32 for x in r)
    dm = trainer._dygraph_model(model)
    fresh = dm.create_model(cfg, device, **({"kernels": kernels} if kernels is not None else {}))
    checkpoint.load_model(s[-1]["model_dir"], fresh)
    for k, v in net.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    assert fresh.step_count == net.step_count == 8
    assert torch.equal(fresh.sparse_state["m"].cpu(), net.sparse_state["m"].cpu())
    assert torch.equal(fresh.dense.m.cpu(), net.dense.m.cpu())
    rng = np.random.default_rng(0)
    ids = torch.as_tensor(rng.integers(0, 30011, (7, S)), device=device)
    dense = torch.as_tensor(rng.random((7, DN), dtype=np.float32), device=device)
    assert torch.equal(fresh.forward(ids, dense).cpu(), net.forward(ids, dense).cpu())
    return s, r


@pytest.mark.parametrize("lazy", [True, False])
def test_train_checkpoint_infer_cpu_backend(tmp_path, caplog, lazy):
    import dcn_cpu_kernels
    run_trainer_loops(tmp_path, "cpu", dcn_cpu_kernels, lazy, caplog)


def test_dcn_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    """Host checks of rec_dcn_cross_*: every call below is refused (or is the batch == 0 no-op) before any launch, so
    it runs on a GPU-less host with dummy non-null pointer values (tests/test_dcn_gpu.py runs the kernels)."""
    import ctypes as C
    from paddlerec_amd import _lib
    L = engine_lib
    p = C.c_void_p(4096)                                     # never dereferenced
    n = C.c_size_t(0)

    def desc(B=8, d=247, layers=2, ld_x0=248, ld_out=376, ld_dxl=247, ld_dx0=248, coeff=1.0, acc=0):
        return _lib.DcnCrossDesc(B, d, layers, ld_x0, ld_out, ld_dxl, ld_dx0, coeff, acc)

    def fwd(dsc, x0=p, xl=p, l2=None, ws=None, ws_bytes=0):
        return L.rec_dcn_cross_fwd(C.byref(dsc), x0, p, p, xl, None, l2, ws, C.c_size_t(ws_bytes), None)

    def bwd(dsc, dxl=p, dz=None, u=None, ws_bytes=1 << 30, dx0=p):
        return L.rec_dcn_cross_bwd(C.byref(dsc), p, p, p, p, dxl, dz, u, dx0, p, p, p, C.c_size_t(ws_bytes), None)

    # the planning query: one partial of 2 * d floats per 768-thread block (12 rows) at d <= 256, per 1024-thread block
    # (16 rows) above; capped at the resident grid (2 resp. 1 block per CU of 256)
    assert L.rec_dcn_cross_bwd_workspace_bytes(C.byref(desc(B=4096)), C.byref(n)) == 0
    assert n.value == ((4096 + 11) // 12) * 2 * 247 * 4
    assert L.rec_dcn_cross_bwd_workspace_bytes(C.byref(desc(B=65536)), C.byref(n)) == 0 and n.value == 512 * 2 * 247 * 4
    assert L.rec_dcn_cross_bwd_workspace_bytes(C.byref(desc(B=65536, d=512, ld_x0=512)), C.byref(n)) == 0
    assert n.value == 256 * 2 * 512 * 4
    assert L.rec_dcn_cross_bwd_workspace_bytes(C.byref(desc(B=0)), C.byref(n)) == 0 and n.value == 0
    assert L.rec_dcn_cross_bwd_workspace_bytes(C.byref(desc()), None) == -1
    assert L.rec_dcn_cross_bwd_workspace_bytes(None, C.byref(n)) == -1
    for bad in (desc(d=0), desc(d=513, ld_x0=520, ld_out=520, ld_dxl=520, ld_dx0=520), desc(layers=0), desc(layers=65),
                desc(B=-1), desc(ld_x0=246), desc(coeff=-1.0), desc(coeff=float("nan"))):
        assert L.rec_dcn_cross_bwd_workspace_bytes(C.byref(bad), C.byref(n)) == -1
        assert fwd(bad) == -1 and bwd(bad) == -1
    assert fwd(desc(d=513, ld_x0=520, ld_out=520)) == -1 and b"1 <= d <= 512" in L.rec_last_error()
    assert fwd(desc(layers=65)) == -1 and b"num_layers" in L.rec_last_error()
    assert fwd(desc(ld_out=246)) == -1 and b"ld_out" in L.rec_last_error()
    assert bwd(desc(ld_dx0=246)) == -1 and b"ld_dx0" in L.rec_last_error()
    assert bwd(desc(ld_dxl=246)) == -1 and b"ld_dxl" in L.rec_last_error()
    assert bwd(desc(ld_dxl=0), dxl=None, dz=p, u=p, dx0=None) == -1          # rank-1 form: ld_dxl is not looked at ...
    assert b"null pointer" in L.rec_last_error()                              # ... the refusal is the missing dX0
    assert bwd(desc(), dxl=None) == -1                                        # neither dXL nor dz / u
    assert fwd(desc(), x0=None) == -1 and b"null pointer" in L.rec_last_error()
    # workspace: the backward always needs its partials, the forward only with the l2 output
    assert bwd(desc(), ws_bytes=8 * 2 * 247 * 4 // 12) == -3 and b"workspace" in L.rec_last_error()
    assert fwd(desc(), l2=p, ws=p, ws_bytes=0) == -3
    assert fwd(desc(), l2=p, ws=None, ws_bytes=1 << 20) == -1
    # batch == 0: a no-op, null pointers and all
    assert L.rec_dcn_cross_fwd(C.byref(desc(B=0)), None, None, None, None, None, None, None, C.c_size_t(0), None) == 0
    assert L.rec_dcn_cross_bwd(C.byref(desc(B=0)), *[None] * 11, C.c_size_t(0), None) == 0


REF_DIR = "/root/reference/models/rank/dcn"


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason="reference tree not mounted (only in the build container)")
def test_reference_yaml_and_sample_data_run_unchanged(tmp_path):
    """The reference's OWN dcn/config.yaml and sample data drive the loops as they are (bs 8, D 9, 1000001 rows, cross_num
    2, fc 512-256-128) — only the output directory and the number of epochs are redirected, and the stand-in's Adam is the
    lazy one (a NumPy pass over the whole table per step would take minutes on the host)."""
    import dcn_cpu_kernels
    from paddlerec_amd import trainer
    yaml_path = os.path.join(REF_DIR, "config.yaml")
    cfg = trainer.load_yaml(yaml_path, ["runner.epochs=1", "runner.model_save_path=" + str(tmp_path / "out"),
                                        "runner.infer_load_path=" + str(tmp_path / "out"),
                                        "runner.infer_start_epoch=0", "runner.infer_end_epoch=1",
                                        "hyper_parameters.optimizer.lazy_mode=True"])
    assert trainer.guess_model(yaml_path) == "dcn"
    s, net = trainer.train(cfg, "dcn", "cpu", dcn_cpu_kernels)
    assert net.d == WIDTH and net.cross_num == 2 and net.layer_sizes == [512, 256, 128]
    assert len(s) == 1 and np.isfinite(s[0]["loss"]) and 0.0 <= s[0]["auc"] <= 1.0
    assert s[0]["samples"] > 0 and s[0]["samples"] % cfg["runner.train_batch_size"] == 0
    assert int(net.status.item()) == 0
    r = trainer.infer(cfg, "dcn", "cpu", dcn_cpu_kernels)
    assert r[0]["samples"] > 0 and 0.0 <= r[0]["auc"] <= 1.0
