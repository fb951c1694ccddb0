"""rank/gatenet (paddlerec_amd/gatenet.py; reference: models/rank/gatenet/net.py, gatenet/dygraph_model.py).

tests/gatenet_ref.py is pinned to tests/golden/gatenet_D9.npz (the reference's unmodified net.py over the paddle shim,
tools/make_golden_gatenet.py: both gates on, a two-layer tower, duplicate ids, the id 0 as a live row, non-zero biases).
The host mirror is checked against the fixture and the restatement with the gatenet_ref-backed operator backend on the CPU
(orchestration only; tests/gatenet_cpu_kernels.py) and with the HIP kernels (`-m gpu`, tests/test_gatenet_gpu.py).  The
argument checks of the rec_gate_* entry points run here too: they return before any launch."""
import logging
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import gatenet_ref as GR
from helpers import GOLDEN, assert_adam_weights_close, assert_close_scaled, load_golden

S, DN, D = 26, 13, 9
WIDTH = S * D + DN          # 247
DATA_KEYS = ("ids", "dense", "label", "D", "fc", "pred", "loss")


def _golden():
    g = load_golden("gatenet_D9")
    p = {k: g[k] for k in g if k not in DATA_KEYS and not k.startswith("g_")}
    return g, p


def _keys(n_layers, emb_gate=True, hidden_gate=True):
    ks = ["embedding.weight", "last_layer.weight", "last_layer.bias"]
    ks += ["embedding_gate_weight_%d" % s for s in range(S)] if emb_gate else []
    for i in range(n_layers):
        ks += ["linear_%d.weight" % i, "linear_%d.bias" % i] + (["hidden_gate_weight_%d" % i] if hidden_gate else [])
    return sorted(ks)


def test_gatenet_ref_matches_reference_golden():
    g, p = _golden()
    assert g["ids"].shape == (10, S) and g["dense"].shape[1] == DN and [int(x) for x in g["fc"]] == [16, 8]
    assert (g["ids"] == 0).any() and len(np.unique(g["ids"])) < g["ids"].size        # id 0 + duplicates
    assert all(np.abs(p[k]).max() > 0 for k in p if k.endswith(".bias"))             # a dropped bias term would show
    assert np.abs(g["dense"]).max() > 1.0 and g["dense"].min() < 0                    # raw values: no log1p
    assert sorted(p) == _keys(2)
    assert all(p["embedding_gate_weight_%d" % s].shape == (1,) for s in range(S))    # ONE scalar per field
    assert p["hidden_gate_weight_0"].shape == (16, 16) and p["hidden_gate_weight_1"].shape == (8, 8)
    o = GR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D)
    assert_close_scaled(o["pred"], g["pred"], 1e-5, "pred")
    assert_close_scaled(o["loss"], g["loss"], 1e-5, "loss")
    assert sorted(o["g"]) == sorted(p)
    for k in p:
        assert_close_scaled(o["g"][k], g["g_" + k], 1e-5, "g " + k)
    assert g["g_embedding.weight"][0].any()                                           # no padding_idx: row 0 trains
    # the mask of the ReLU is y's: some gated outputs are negative where y is positive
    f = GR.forward(g["ids"], g["dense"], p, D)
    assert any(((x < 0) & (y > 0)).any() for x, y in zip(f["xs"][1:], f["ys"]))


def _merge(ids, de, N):
    out = np.zeros((N, D), np.float64)
    np.add.at(out, ids.reshape(-1), de[:, :S * D].reshape(-1, D))
    return out


def _layer(N, fc, device, kernels, emb_gate=True, hidden_gate=True):
    from paddlerec_amd.gatenet import GateDNNLayer
    kw = {"kernels": kernels} if kernels is not None else {}
    return GateDNNLayer(N, D, DN, S, fc, emb_gate, hidden_gate, device=device, **kw)


def check_layer_on_fixture(device, kernels, rel):
    """Forward = the fixture's pred; one train_step leaves the fixture's loss and gradients in the layer."""
    g, p = _golden()
    N = p["embedding.weight"].shape[0]
    fc = [int(x) for x in g["fc"]]
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    m = _layer(N, fc, device, kernels)
    assert float(m.embedding.abs().max()) <= 1.0 and float(m.embedding.abs().max()) > 0.9     # U[-1, 1]
    assert m.rec[0, :D].any() and not m.rec[:, D:].any()                     # row 0 is drawn like any other
    assert float(m.dense.p["last_layer.bias"]) == 0.0 and not m.dense.p["linear_0.bias"].any()
    assert m.rec.shape == (N, 32) and m.d == WIDTH and m.d_pad == 248 and m.padding_idx is None
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in p.items()}
    m.set_dict(p)
    sparse_inputs = [T(g["ids"][:, s:s + 1]) for s in range(S)]             # the reference's list of [B,1]
    pred = m.forward(sparse_inputs, T(g["dense"]))
    assert_close_scaled(pred.cpu().numpy(), g["pred"], rel, "pred")
    loss, pred2 = m.train_step(sparse_inputs, T(g["dense"]), T(g["label"]), lr=1e-9)
    assert int(m.status.item()) == 0
    assert_close_scaled(loss.cpu().numpy(), g["loss"], rel, "loss")
    assert_close_scaled(pred2.cpu().numpy(), g["pred"], rel, "pred (train_step)")
    gd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.grad_dict().items()}
    assert sorted(gd) == sorted(k for k in p if k != "embedding.weight")
    for k in gd:
        assert_close_scaled(gd[k], g["g_" + k], rel, "g " + k)
    # the S scalars are ONE tensor inside the layer: their gradients are compared as that vector too
    gv = np.concatenate([gd["embedding_gate_weight_%d" % s] for s in range(S)])
    assert_close_scaled(gv, np.concatenate([g["g_embedding_gate_weight_%d" % s] for s in range(S)]), rel, "g gate vector")
    de = m._last_dfeat.cpu().numpy()
    assert de.shape == (len(g["ids"]), WIDTH)
    assert_close_scaled(_merge(g["ids"], de, N), g["g_embedding.weight"], rel, "g embedding.weight")
    return m


def test_layer_host_logic_cpu_backend_matches_fixture():
    import gatenet_cpu_kernels
    check_layer_on_fixture("cpu", gatenet_cpu_kernels, 1e-5)


def test_state_dict_keys_are_the_references():
    import gatenet_cpu_kernels
    g, p = _golden()
    m = _layer(301, [16, 8], "cpu", gatenet_cpu_kernels)
    assert sorted(m.state_dict()) == sorted(p) == _keys(2)
    assert m.dense.names[0] == "embedding_gate_weight" and tuple(m.dense.p["embedding_gate_weight"].shape) == (S,)
    m.state_dict()["embedding_gate_weight_3"].fill_(7.0)                     # the keys are views of the vector
    assert float(m.dense.p["embedding_gate_weight"][3]) == 7.0
    # initialisers: Normal(std 1 / sqrt(fan_in)) for the tower, the gates and the head; N(0, 1) gate scalars
    big = _layer(11, [512, 256], "cpu", gatenet_cpu_kernels)
    q = big.dense.p
    assert abs(float(q["linear_0.weight"].std()) * np.sqrt(WIDTH) - 1.0) < 0.05
    assert abs(float(q["hidden_gate_weight_0"].std()) * np.sqrt(512) - 1.0) < 0.05
    assert abs(float(q["hidden_gate_weight_1"].std()) * np.sqrt(256) - 1.0) < 0.05
    assert abs(float(q["last_layer.weight"].std()) * np.sqrt(256) - 1.0) < 0.2
    many = _layer(11, [4], "cpu", gatenet_cpu_kernels)
    many2 = _layer(11, [4], "cpu", gatenet_cpu_kernels)
    both = torch.cat([many.dense.p["embedding_gate_weight"], many2.dense.p["embedding_gate_weight"]])
    assert 0.5 < float(both.std()) < 1.5


def _small_batch(rng, N, B=24):
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    ids[:, 0] = 5                                                             # a hot row
    ids[::5, 3] = 0                                                           # id 0: a live row
    dense = (rng.standard_normal((B, DN)) * 1.5).astype(np.float32)
    label = (rng.random((B, 1)) < 0.4).astype(np.int64)
    return ids, dense, label


def check_adam_trajectory(device, kernels, lazy, rel):
    """Three steps against the plain restatement's trajectory (gatenet_ref.Trainer): loss and prediction of every step,
    weights, table and the table's moments after the last.  The two Adam forms part on the rows that only the first batch
    touched: lazy=False decays their moments (and moves them) in steps 2 and 3 as well, lazy=True leaves them as step 1
    wrote them.  Each form must agree with the oracle of its own kind and differ from the other kind on those rows."""
    g, p = _golden()
    N, fc = p["embedding.weight"].shape[0], [int(x) for x in g["fc"]]
    m = _layer(N, fc, device, kernels)
    m.lazy_mode = lazy
    m.set_dict(p)
    tr = GR.Trainer(p, D, lazy=lazy)
    rng = np.random.default_rng(8)
    T = lambda a: torch.as_tensor(a).to(device)
    touched = np.zeros(N, bool)
    for step in range(3):
        ids, dense, label = _small_batch(rng, N)
        touched[ids.reshape(-1)] = True
        loss, pred = m.train_step(T(ids), T(dense), T(label), lr=1e-2)
        ol, op = tr.train_step(ids, dense, label, lr=1e-2)
        np.testing.assert_allclose(float(loss), ol, rtol=rel)
        np.testing.assert_allclose(pred.cpu().numpy(), op, rtol=rel, atol=1e-6)
    assert int(m.status.item()) == 0 and m.step_count == 3
    assert not m.rec[:, D:].any()                                             # the pad columns never move
    for k, v in m.state_dict().items():
        assert_adam_weights_close(v.detach().cpu().numpy(), tr.p[k], lr=1e-2, steps=3, err_msg=k)
    assert_close_scaled(m.sparse_state["m"].cpu().numpy(), tr.m["embedding.weight"], 1e-5, "m of the table")
    assert_close_scaled(m.sparse_state["v"].cpu().numpy(), tr.v["embedding.weight"], 1e-5, "v of the table")
    moved = (m.embedding.cpu().numpy() != p["embedding.weight"]).any(axis=1)
    assert touched[0] and moved[0] and moved[touched].all() and not moved[~touched].any()
    first = np.zeros(N, bool)                                                 # rows only the FIRST batch touched
    rng = np.random.default_rng(8)
    batches = [_small_batch(rng, N)[0] for _ in range(3)]
    first[batches[0].reshape(-1)] = True
    first[np.concatenate([b.reshape(-1) for b in batches[1:]])] = False
    assert first.any()
    other = GR.Trainer(p, D, lazy=not lazy)                                   # the trajectory of the other Adam form
    rng = np.random.default_rng(8)
    for step in range(3):
        other.train_step(*_small_batch(rng, N), lr=1e-2)
    assert (other.m["embedding.weight"][first] != m.sparse_state["m"].cpu().numpy()[first]).any()
    return m


@pytest.mark.parametrize("lazy", [False, True])
def test_adam_trajectory_cpu_backend(lazy):
    import gatenet_cpu_kernels
    check_adam_trajectory("cpu", gatenet_cpu_kernels, lazy, 1e-5)


@pytest.mark.parametrize("emb_gate,hidden_gate", [(True, True), (True, False), (False, True), (False, False)])
def test_gate_switches_cpu_backend(emb_gate, hidden_gate):
    check_gate_switches("cpu", __import__("gatenet_cpu_kernels"), emb_gate, hidden_gate, 1e-5)


def check_gate_switches(device, kernels, emb_gate, hidden_gate, rel):
    """Each on / off combination against the restatement, which follows the keys present in the state_dict."""
    g, p = _golden()
    N = p["embedding.weight"].shape[0]
    p = {k: v for k, v in p.items() if (emb_gate or not k.startswith("embedding_gate")) and
         (hidden_gate or not k.startswith("hidden_gate"))}
    m = _layer(N, [16, 8], device, kernels, emb_gate, hidden_gate)
    assert sorted(m.state_dict()) == sorted(p) == _keys(2, emb_gate, hidden_gate)
    m.set_dict(p)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    o = GR.loss_and_grads(g["ids"], g["dense"], g["label"], p, D)
    pred = m.forward(T(g["ids"]), T(g["dense"]))
    assert_close_scaled(pred.cpu().numpy(), o["pred"], rel, "pred")
    loss, _ = m.train_step(T(g["ids"]), T(g["dense"]), T(g["label"]), lr=1e-9)
    assert int(m.status.item()) == 0
    assert_close_scaled(loss.cpu().numpy(), o["loss"], rel, "loss")
    gd = m.grad_dict()
    assert sorted(gd) == sorted(k for k in p if k != "embedding.weight")
    for k in gd:
        assert_close_scaled(gd[k].cpu().numpy(), o["g"][k], rel, "g " + k)
    assert_close_scaled(_merge(g["ids"], m._last_dfeat.cpu().numpy(), N), o["g"]["embedding.weight"], rel, "g table")
    return m


def reference_config():
    """The values of the reference's gatenet/config.yaml, typed in (flat keys, as trainer.load_yaml makes them)."""
    return {"runner.train_data_dir": "data/sample_data/train", "runner.train_reader_path": "criteo_reader",
            "runner.use_gpu": False, "runner.use_auc": True, "runner.train_batch_size": 2, "runner.epochs": 3,
            "runner.print_interval": 2, "runner.model_save_path": "output_model_gatenet", "runner.infer_batch_size": 2,
            "runner.infer_reader_path": "criteo_reader", "runner.test_data_dir": "data/sample_data/train",
            "runner.infer_load_path": "output_model_gatenet", "runner.infer_start_epoch": 2, "runner.infer_end_epoch": 3,
            "hyper_parameters.optimizer.class": "Adam", "hyper_parameters.optimizer.learning_rate": 0.001,
            "hyper_parameters.sparse_inputs_slots": 27, "hyper_parameters.sparse_feature_number": 1000001,
            "hyper_parameters.sparse_feature_dim": 9, "hyper_parameters.dense_input_dim": 13,
            "hyper_parameters.fc_sizes": [512, 256, 128, 32], "hyper_parameters.distributed_embedding": 0,
            "hyper_parameters.use_embedding_gate": True, "hyper_parameters.use_hidden_gate": True}


def test_dygraph_model_plugin_surface():
    import gatenet_cpu_kernels
    from paddlerec_amd.gatenet import DygraphModel, GateDNNLayer
    dm = DygraphModel()
    cfg = reference_config()
    net = dm.create_model(cfg, "cpu", kernels=gatenet_cpu_kernels)
    assert isinstance(net, GateDNNLayer) and net.num_field == S and net.sparse_feature_number == 1000001
    assert net.layer_sizes == [512, 256, 128, 32] and net.use_embedding_gate and net.use_hidden_gate
    assert net.lazy_mode is False and net.d == WIDTH and sorted(net.state_dict()) == _keys(4)
    off = dm.create_model(dict(cfg, **{"hyper_parameters.use_embedding_gate": False, "hyper_parameters.sparse_feature_number": 11,
                                       "hyper_parameters.use_hidden_gate": False}), "cpu", kernels=gatenet_cpu_kernels)
    assert sorted(off.state_dict()) == _keys(4, False, False)
    # the reference's 28 arrays through the plugin methods, on the fixture's net
    g, p = _golden()
    small = dict(cfg, **{"hyper_parameters.sparse_feature_number": p["embedding.weight"].shape[0],
                         "hyper_parameters.fc_sizes": [int(x) for x in g["fc"]],
                         "hyper_parameters.optimizer.learning_rate": 1e-9})
    net = dm.create_model(small, "cpu", kernels=gatenet_cpu_kernels)
    net.set_dict(p)
    metrics, names = dm.create_metrics("cpu")
    batch = [g["label"]] + [g["ids"][:, s:s + 1] for s in range(S)] + [g["dense"]]
    assert len(batch) == 28
    metrics, _ = dm.infer_forward(net, metrics, batch, small)
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == len(g["label"])
    loss, metrics, print_dict = dm.train_forward(net, metrics, batch, small)
    assert_close_scaled(float(loss), g["loss"], 1e-5, "loss")
    assert names == ["auc"] and print_dict is None


def test_trainer_knows_gatenet(tmp_path):
    from paddlerec_amd import trainer
    assert "gatenet" in trainer.MODELS
    d = tmp_path / "models" / "rank" / "gatenet"
    d.mkdir(parents=True)
    assert trainer.guess_model(str(d / "config.yaml")) == "gatenet"
    from paddlerec_amd.gatenet import DygraphModel
    assert isinstance(trainer._dygraph_model("gatenet"), DygraphModel)
    assert "gatenet" in trainer.__doc__


def run_trainer_loops(tmp_path, device, kernels, lazy, caplog=None):
    """One epoch over the reference's own sample lines (tests/golden/criteo_slot_sample.txt, batch 2) -> a checkpoint ->
    infer over it -> a fresh model loaded from it predicts exactly like the trained net."""
    from paddlerec_amd import checkpoint, trainer
    d = tmp_path / "run"
    (d / "data").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "criteo_slot_sample.txt"), d / "data" / "part-0")
    cfg = dict(reference_config(), **{
        "config_abs_dir": str(d), "runner.train_data_dir": "data", "runner.test_data_dir": "data", "runner.epochs": 1,
        "runner.model_save_path": str(tmp_path / "out"), "runner.infer_load_path": str(tmp_path / "out"),
        "runner.infer_start_epoch": 0, "runner.infer_end_epoch": 1, "hyper_parameters.fc_sizes": [32, 16],
        "hyper_parameters.optimizer.lazy_mode": lazy})
    if caplog is not None:
        caplog.set_level(logging.INFO, logger="paddlerec_amd.trainer")
    s, net = trainer.train(cfg, "gatenet", device, kernels)
    if caplog is not None:
        said = [r.getMessage() for r in caplog.records if "ONE scalar per field" in r.getMessage()]
        assert len(said) == 1 and "gatenet" in said[0]
    assert net.lazy_mode is lazy and net.use_embedding_gate and net.use_hidden_gate
    assert [x["epoch"] for x in s] == [0] and s[0]["batches"] == 3 and s[0]["samples"] == 6
    assert np.isfinite(s[0]["loss"]) and 0.0 <= s[0]["auc"] <= 1.0
    assert int(net.status.item()) == 0 and net.step_count == 3
    with open(os.path.join(s[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    want = {"embedding.weight": (1000001, D), "linear_0.weight": (WIDTH, 32), "linear_0.bias": (32,),
            "hidden_gate_weight_0": (32, 32), "linear_1.weight": (32, 16), "linear_1.bias": (16,),
            "hidden_gate_weight_1": (16, 16), "last_layer.weight": (16, 1), "last_layer.bias": (1,)}
    want.update(("embedding_gate_weight_%d" % i, (1,)) for i in range(S))
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    r = trainer.infer(cfg, "gatenet", device, kernels)
    assert [x["epoch"] for x in r] == [0] and 0.0 <= r[0]["auc"] <= 1.0 and r[0]["samples"] == 6
    dm = trainer._dygraph_model("gatenet")
    fresh = dm.create_model(cfg, device, **({"kernels": kernels} if kernels is not None else {}))
    checkpoint.load_model(s[-1]["model_dir"], fresh)
    for k, v in net.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    assert fresh.step_count == net.step_count
    assert torch.equal(fresh.sparse_state["m"].cpu(), net.sparse_state["m"].cpu())
    assert torch.equal(fresh.dense.m.cpu(), net.dense.m.cpu())
    rng = np.random.default_rng(0)
    ids = torch.as_tensor(rng.integers(0, 1000001, (7, S)), device=device)
    dense = torch.as_tensor(rng.random((7, DN), dtype=np.float32), device=device)
    assert torch.equal(fresh.forward(ids, dense).cpu(), net.forward(ids, dense).cpu())
    return s, r


@pytest.mark.parametrize("lazy", [True, False])
def test_train_checkpoint_infer_cpu_backend(tmp_path, caplog, lazy):
    import gatenet_cpu_kernels
    run_trainer_loops(tmp_path, "cpu", gatenet_cpu_kernels, lazy, caplog)


def test_gate_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    """Host checks of the rec_gate_* entry points: every call below is refused (or is the empty-batch no-op) before any
    launch, so it runs on a GPU-less host with dummy non-null pointer values (tests/test_gatenet_gpu.py runs the
    kernels)."""
    import ctypes as C
    L = engine_lib
    p = C.c_void_p(4096)                                     # never dereferenced
    n = C.c_size_t(0)
    err = lambda: L.rec_last_error()

    def fwd(n_=52, S_=26, D_=9, rs=32, N=100, ids=p, W=p, gw=p, out=p, ld=248, st=p):
        return L.rec_gate_emb_fwd(n_, S_, D_, rs, N, -1, ids, W, gw, out, ld, st, None)

    def bwd(n_=52, S_=26, D_=9, rs=32, N=100, ids=p, W=p, gw=p, g=p, ld=248, dw=p, st=p, ws=p, ws_bytes=1 << 30):
        return L.rec_gate_emb_bwd(n_, S_, D_, rs, N, -1, ids, W, gw, g, ld, dw, st, ws, C.c_size_t(ws_bytes), None)

    for call in (fwd, bwd):
        assert call(D_=0) == -1 and b"bad sizes" in err()
        assert call(S_=0) == -1 and call(n_=-26) == -1 and call(N=0) == -1 and call(rs=8) == -1
        assert call(n_=53) == -1 and b"multiple of num_fields" in err()
        assert call(ld=233) == -1 and b"stride" in err() and b"234" in err()      # below S * D
        assert call(ids=None) == -1 and b"null pointer" in err()
        assert call(W=None) == -1 and call(gw=None) == -1 and call(st=None) == -1
        assert call(D_=65, rs=65, ld=26 * 65) == -2                                # no row shape for D 65
    assert fwd(out=None) == -1 and bwd(g=None) == -1 and bwd(dw=None) == -1 and bwd(ws=None) == -1
    assert bwd(S_=1025, n_=1025, ld=1025 * 9) == -2 and b"num_fields" in err()
    # the planning query: one partial row of S floats per block, at most 2048 blocks (8 per CU); 4 lookups per block
    # at the widest row group
    assert L.rec_gate_emb_bwd_workspace_bytes(52, 26, C.byref(n)) == 0 and n.value == 13 * 26 * 4
    assert L.rec_gate_emb_bwd_workspace_bytes(65536 * 26, 26, C.byref(n)) == 0 and n.value == 2048 * 26 * 4
    assert L.rec_gate_emb_bwd_workspace_bytes(0, 26, C.byref(n)) == 0 and n.value == 0
    assert L.rec_gate_emb_bwd_workspace_bytes(52, 26, None) == -1 and L.rec_gate_emb_bwd_workspace_bytes(52, 0, C.byref(n)) == -1
    assert bwd(ws_bytes=4 * 26 * 4 - 1) == -3 and b"workspace" in err()          # D 9: 16 lookups per block, 4 blocks
    # an empty batch: a no-op, null pointers and all
    assert L.rec_gate_emb_fwd(0, 26, 9, 32, 100, -1, None, None, None, None, 248, None, None) == 0
    assert L.rec_gate_emb_bwd(0, 26, 9, 32, 100, -1, None, None, None, None, 248, None, None, None, C.c_size_t(0), None) == 0

    def hf(B=8, n_=32, y=p, t=p, x=p, ld=(32, 32, 32)):
        return L.rec_gate_hidden_fwd(B, n_, y, ld[0], t, ld[1], x, ld[2], None)

    def hb(B=8, n_=32, u=p, y=p, h=p, dt=C.c_void_p(8192), uh=C.c_void_p(12288), ld=(32,) * 5):
        return L.rec_gate_hidden_bwd(B, n_, u, ld[0], y, ld[1], h, ld[2], dt, ld[3], uh, ld[4], None)

    def rm(B=8, n_=32, dy=C.c_void_p(8192), y=p, ld=(32, 32)):
        return L.rec_relu_mask_inplace(B, n_, dy, ld[0], y, ld[1], None)

    for call in (hf, hb, rm):
        assert call(n_=0) == -1 and b"bad sizes" in err()
        assert call(B=-1) == -1
        assert call(y=None) == -1 and b"null pointer" in err()
        assert call(B=0, y=None) == 0                                            # an empty batch launches nothing
    assert hf(ld=(32, 31, 32)) == -1 and b"row stride" in err()
    assert hb(ld=(32, 32, 32, 32, 31)) == -1 and b"row stride" in err()
    assert rm(ld=(31, 32)) == -1 and b"row stride" in err()
    assert hf(t=None) == -1 and hf(x=None) == -1 and hb(dt=None) == -1 and hb(uh=None) == -1 and rm(dy=None) == -1
    assert hb(dt=p) == -1 and b"alias" in err()
    assert rm(dy=p) == -1 and b"must not be y" in err()
