"""rank/autofis without a GPU (paddlerec_amd/autofis.py; reference: models/rank/autofis/net.py, optimizer.py,
dygraph_model.py, trainer.py).  tests/golden/autofis_D5.npz holds what the reference's UNMODIFIED net.py / optimizer.py
computed over the paddle shim (tools/make_golden_autofis.py); autofis_ref is the float64 NumPy restatement the kernels are
compared with; autofis_cpu_kernels runs the host mirror's orchestration on CPU tensors.  The check_* functions take
(device, kernels) so that tests/test_autofis_gpu.py runs the same checks on the HIP kernels.
"""
import logging
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import autofis_ref as AR
from helpers import GOLDEN, assert_close_scaled, load_golden

REL = 1e-5
SAMPLE_X, SAMPLE_Y = os.path.join(GOLDEN, "autofis_sample_x.txt"), os.path.join(GOLDEN, "autofis_sample_y.txt")


def golden():
    g = load_golden("autofis_D5")
    N, S, D, width, depth, B = (int(x) for x in g["sizes"])
    return g, dict(N=N, S=S, D=D, width=width, depth=depth, B=B, P=S * (S - 1) // 2)


def param_keys(depth):
    keys = [AR.MASK, AR.WEMB, AR.VEMB] + [AR.LIN % i + s for i in range(depth + 1) for s in (".weight", ".bias")]
    for name in [AR.BN % i for i in range(depth)] + [AR.BN2]:
        keys += [name + s for s in (".weight", ".bias", "._mean", "._variance")]
    return sorted(keys)


def params(g, pre, depth):
    return {k: g[pre + k] for k in param_keys(depth)}


def check_record(g, pre, p, comb_mask, got_pred, got_loss, got_grads, got_rs, rel, what):
    """The bias of a Linear in front of a BatchNorm has a gradient of exactly zero (the BatchNorm removes any constant):
    the fixture holds float32 summation noise there, 6e-8 at most.  Such a gradient is held to `rel` of the scale of the
    terms it sums, the same layer's weight gradient, on both sides; every other tensor to `rel` of its own scale."""
    assert_close_scaled(got_pred, g[pre + "pred"], rel, what + " pred")
    assert_close_scaled(got_loss, g[pre + "loss"], rel, what + " loss")
    depth = AR.depth_of(p)
    dead = {AR.LIN % i + ".bias": AR.LIN % i + ".weight" for i in range(depth)}
    for k in p:
        if k.endswith("._mean") or k.endswith("._variance"):
            assert_close_scaled(got_rs[k], g[pre + "rs_" + k], rel, what + " running " + k)
        elif k in dead:
            bound = rel * float(np.abs(g[pre + "g_" + dead[k]]).max())
            assert float(np.abs(g[pre + "g_" + k]).max()) <= bound and float(np.abs(got_grads[k]).max()) <= bound, k
        else:
            assert_close_scaled(got_grads[k], g[pre + "g_" + k], rel, what + " grad " + k)


def test_restatement_matches_reference_golden():
    g, z = golden()
    for pre, comb in (("a_", None), ("c_", g["c_comb_mask"])):
        p = params(g, pre, z["depth"])
        pred, c = AR.forward(p, g["ids"], comb)
        gr = AR.backward(pred, g["label"], c)
        check_record(g, pre, p, comb, pred, AR.loss_of(pred, g["label"]), gr, c["rs"], REL, "restatement " + pre)
    cols, rows = AR.generate_pairs(z["S"], g["c_comb_mask"])
    assert 2 not in cols + rows and len(cols) == int(g["c_comb_mask"].sum()) == g["c_mask"].shape[1]
    assert not gr[AR.VEMB][np.setdiff1d(np.arange(z["N"]), g["ids"])].any()
    pred, _ = AR.forward(params(g, "d_", z["depth"]), g["ids"], None, training=False)
    assert_close_scaled(pred, g["d_pred"], REL, "restatement eval")


def test_restatement_grda_matches_reference_golden():
    g, _ = golden()
    opt = AR.Grda(g["grda_acc0"].astype(np.float64), 1.0, *g["grda"])
    m = g["grda_mask0"].astype(np.float64)
    for t in (1, 2, 3):
        m = opt.step(m, g["grda_grad%d" % t].astype(np.float64))
        assert_close_scaled(opt.acc, g["grda_acc%d" % t], REL, "acc %d" % t)
        assert abs(opt.l1_accumulation - float(g["grda_l1_%d" % t][0])) <= 1e-12
        np.testing.assert_array_equal(m == 0, g["grda_mask%d" % t] == 0)
        assert_close_scaled(m, g["grda_mask%d" % t], REL, "mask %d" % t)
    assert (m == 0).any() and (m != 0).any()


# ---------------------------------------------------------------- the layer on a backend
def make_layer(z, device, kernels, stage=0, comb_mask=None, **kw):
    from paddlerec_amd.autofis import AutoDeepFMLayer
    return AutoDeepFMLayer(z["S"], z["N"], z["D"], z["width"], z["depth"], z["P"], stage, comb_mask=comb_mask,
                           device=device, kernels=kernels, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def dense_table_grad(net, ids, z):
    """The dense gradient of both tables from the step's per-lookup gradients."""
    last = net._last
    rg = _np(last["row_grad"]).reshape(len(ids), z["S"], z["D"]).astype(np.float64)
    dz = _np(last["dz"]).reshape(-1).astype(np.float64)
    gv, gw = np.zeros((z["N"], z["D"])), np.zeros((z["N"], 1))
    np.add.at(gv, ids, rg)
    np.add.at(gw, ids, np.broadcast_to(dz[:, None, None], ids.shape + (1,)))
    return gv, gw


def check_layer_on_fixture(device, kernels, rel):
    """Records (a), (c), (d): pred, loss, every gradient, the running statistics, eval pred; state_dict keys."""
    g, z = golden()
    T = lambda a: torch.as_tensor(a).to(device)
    for pre, stage, comb in (("a_", 0, None), ("c_", 1, g["c_comb_mask"])):
        net = make_layer(z, device, kernels, stage, comb)
        assert sorted(net.state_dict()) == param_keys(z["depth"]) == sorted(
            k[len(pre):] for k in g if k.startswith(pre) and k[len(pre):] in param_keys(z["depth"]))
        p = params(g, pre, z["depth"])
        net.set_dict(p)
        loss, pred = net.train_step(T(g["ids"]), T(g["label"]), lr=1e-12)
        grads = {k: _np(v) for k, v in net.grad_dict().items()}
        grads[AR.VEMB], grads[AR.WEMB] = dense_table_grad(net, g["ids"], z)
        check_record(g, pre, p, comb, _np(pred).reshape(-1), _np(loss), grads, {k: _np(v) for k, v in net.buffers.items()},
                     rel, "layer " + pre)
        assert int(net.status.item()) == 0
    net = make_layer(z, device, kernels)
    net.set_dict(params(g, "d_", z["depth"]))
    pred = net.forward(T(g["ids"]))
    assert tuple(pred.shape) == (z["B"],)
    assert_close_scaled(_np(pred), g["d_pred"], rel, "layer eval pred")


def test_layer_host_logic_cpu_backend_matches_fixture():
    import autofis_cpu_kernels
    check_layer_on_fixture("cpu", autofis_cpu_kernels, REL)


def check_grda_trajectory(device, kernels, rel):
    """Record (b) through the layer's own _grda_step: accumulator, l1_accumulation, the entries that hit exactly 0, and
    that the comb_mask written from it drops exactly those."""
    g, z = golden()
    net = make_layer(z, device, kernels, grad_c=float(g["grda"][0]), grad_mu=float(g["grda"][1]))
    net.dense.p[AR.MASK].copy_(torch.as_tensor(g["grda_mask0"]))
    net.grda_acc.copy_(torch.as_tensor(g["grda_acc0"]).reshape(-1))
    for t in (1, 2, 3):
        net.dense.g[AR.MASK].copy_(torch.as_tensor(g["grda_grad%d" % t]))
        net._grda_step()
        assert_close_scaled(_np(net.grda_acc), g["grda_acc%d" % t], rel, "acc %d" % t)
        assert abs(net.grda_l1 - float(g["grda_l1_%d" % t][0])) <= 1e-12 and net.grda_iterations == t
        m = _np(net.dense.p[AR.MASK])
        np.testing.assert_array_equal(m == 0, g["grda_mask%d" % t] == 0)
        assert_close_scaled(m, g["grda_mask%d" % t], rel, "mask %d" % t)
    comb = net.comb_mask_of_mask()
    np.testing.assert_array_equal(comb, (g["grda_mask3"].reshape(-1) != 0).astype(int))
    assert 0 < comb.sum() < z["P"]
    nxt = make_layer(z, device, kernels, 1, comb)
    assert nxt.num_pairs == int(comb.sum()) and tuple(nxt.dense.p[AR.MASK].shape) == (1, int(comb.sum()))


def test_grda_trajectory_cpu_backend():
    import autofis_cpu_kernels
    check_grda_trajectory("cpu", autofis_cpu_kernels, REL)


# ---------------------------------------------------------------- the lr decay of the model's own trainer
def reference_lr_schedule(lr, gamma, num_batches, epochs):
    """A transcription of autofis/trainer.py:106-116: the lr each batch trains with."""
    used = []
    decay_steps = num_batches // 5
    for _ in range(epochs):
        for batch_id in range(num_batches):
            if (batch_id + 1) % decay_steps == 0:
                lr = lr * gamma
            used.append(lr)
    return used


def test_lr_decay_schedule_matches_the_reference_rule(caplog):
    from paddlerec_amd.autofis import StepDecay
    caplog.set_level(logging.INFO, logger="paddlerec_amd.autofis")
    d = StepDecay(0.001, 0.7, 12)
    got = [d.before_batch(b) for _ in range(2) for b in range(12)]
    assert got == reference_lr_schedule(0.001, 0.7, 12, 2)
    assert got[0] == 0.001 and got[1] == got[2] == 0.001 * 0.7 and len(set(got)) == 13    # decay_steps 2: 12 decays
    assert not [r for r in caplog.records if "fewer than 5" in r.getMessage()]
    d = StepDecay(0.001, 0.7, 4)                                  # the reference: ZeroDivisionError
    assert [d.before_batch(b) for _ in range(2) for b in range(4)] == [0.001] * 8
    said = [r.getMessage() for r in caplog.records if "fewer than 5" in r.getMessage()]
    assert len(said) == 1 and "constant" in said[0]
    with pytest.raises(ZeroDivisionError):
        reference_lr_schedule(0.001, 0.7, 4, 1)


# ---------------------------------------------------------------- reader, trainer, checkpoint
def test_reader_parses_the_sample_lines():
    from paddlerec_amd.reader import AutofisReader
    rd = AutofisReader([SAMPLE_X, SAMPLE_Y], 5, "cpu")
    batches = list(rd)
    assert len(rd) == len(batches) == 2                           # drop_last: 12 lines
    label, ids = batches[1]
    assert tuple(label.shape) == (5, 1) and tuple(ids.shape) == (5, 39) and ids.dtype == label.dtype == torch.int64
    x, y = np.loadtxt(SAMPLE_X, dtype=np.int64), np.loadtxt(SAMPLE_Y, dtype=np.int64)
    np.testing.assert_array_equal(ids.numpy(), x[5:10])
    np.testing.assert_array_equal(label.numpy().reshape(-1), y[5:10])
    with pytest.raises(ValueError):
        AutofisReader([SAMPLE_X], 5, "cpu")


def reference_config():
    """The values of the reference's autofis/config.yaml, typed in (flat keys, as trainer.load_yaml makes them), with the
    width and depth cut down: the trainer tests are about the loops."""
    return {"runner.train_data_dir": "data/sample_data", "runner.train_reader_path": "criteo_reader",
            "runner.use_gpu": False, "runner.use_auc": False, "runner.train_batch_size": 2, "runner.epochs": 1,
            "runner.print_interval": 1, "runner.model_save_path": "output_model_autofis",
            "runner.test_data_dir": "data/sample_data", "runner.infer_reader_path": "criteo_reader",
            "runner.infer_batch_size": 2, "runner.infer_load_path": "output_model_autofis",
            "runner.infer_start_epoch": 0, "runner.infer_end_epoch": 1, "hyper_parameters.optimizer.class": "Adam",
            "hyper_parameters.optimizer.learning_rate": 0.001, "hyper_parameters.optimizer.gamma": 0.7,
            "hyper_parameters.num_inputs": 39, "hyper_parameters.input_size": 1178909,
            "hyper_parameters.embedding_size": 40, "hyper_parameters.width": 700, "hyper_parameters.depth": 5,
            "hyper_parameters.n_col": 741, "hyper_parameters.grad_c": 0.0005, "hyper_parameters.grad_mu": 0.8,
            "hyper_parameters.pairs": 741}


def run_trainer_loops(tmp_path, device, kernels, caplog, monkeypatch, input_size=1178909, emb=4, width=8, depth=2):
    """Stage 0 over the reference's own sample lines -> comb_mask.npy in the working directory -> stage 1 reads it ->
    --infer over the stage-1 checkpoint.  grad_c is raised so that stage 0 drops some pairs, not all, in 6 steps."""
    from paddlerec_amd import checkpoint, trainer
    d = tmp_path / "run"
    (d / "data").mkdir(parents=True)
    shutil.copy(SAMPLE_X, d / "data" / "sample_train_x.txt")
    shutil.copy(SAMPLE_Y, d / "data" / "sample_train_y.txt")
    monkeypatch.chdir(d)
    cfg = dict(reference_config(), **{
        "config_abs_dir": str(d), "runner.train_data_dir": "data", "runner.test_data_dir": "data",
        "runner.model_save_path": str(tmp_path / "out0"), "hyper_parameters.input_size": input_size,
        "hyper_parameters.embedding_size": emb, "hyper_parameters.width": width, "hyper_parameters.depth": depth,
        "hyper_parameters.grad_c": 0.143})      # l1 after 6 steps: 0.143 * 6^0.8 = 0.60, the middle of mask + acc
    caplog.set_level(logging.INFO)
    s0, net0 = trainer.train(cfg, "autofis", device, kernels)
    said = [r.getMessage() for r in caplog.records if r.getMessage().startswith("autofis: stage 0 with 741")]
    assert len(said) == 1 and "SimpleGrda" in said[0] and "non-lazy" in said[0] and "gamma" in said[0]
    assert s0[0]["batches"] == 6 and s0[0]["samples"] == 12 and np.isfinite(s0[0]["loss"])
    assert 0.0 <= s0[0]["auc"] <= 1.0 and np.isfinite(s0[0]["log_loss"]) and s0[0]["log_loss"] > 0
    assert net0.step_count == 6 and net0.grda_iterations == 6 and int(net0.status.item()) == 0
    assert net0.lr == pytest.approx(0.001 * 0.7 ** 6)            # decay_steps = 6 // 5 = 1: every batch
    comb = np.load(d / "comb_mask.npy")
    kept = int(comb.sum())
    assert comb.shape == (741,) and 0 < kept < 741
    np.testing.assert_array_equal(comb, net0.comb_mask_of_mask())
    cfg1 = dict(cfg, stage="1", **{"runner.model_save_path": str(tmp_path / "out1"),
                                   "runner.infer_load_path": str(tmp_path / "out1")})
    s1, net1 = trainer.train(cfg1, "autofis", device, kernels)
    assert net1.stage == 1 and net1.num_pairs == kept and net1.grda_acc is None and s1[0]["batches"] == 6
    with open(os.path.join(s1[-1]["model_dir"], "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert sorted(sd) == param_keys(depth) and sd[AR.MASK].shape == (1, kept) and sd[AR.VEMB].shape == (input_size, emb)
    r = trainer.infer(cfg1, "autofis", device, kernels)
    assert [x["epoch"] for x in r] == [0] and r[0]["samples"] == 12 and 0.0 <= r[0]["auc"] <= 1.0
    assert np.isfinite(r[0]["log_loss"])
    fresh = trainer._dygraph_model("autofis").create_model(cfg1, device, **({"kernels": kernels} if kernels else {}))
    checkpoint.load_model(s1[-1]["model_dir"], fresh)
    for k, v in net1.state_dict().items():
        assert torch.equal(v.detach().cpu(), fresh.state_dict()[k].detach().cpu()), k
    return s0, s1, r


def test_stage0_comb_mask_stage1_infer_cpu_backend(tmp_path, caplog, monkeypatch):
    import autofis_cpu_kernels
    # a table of 1 178 909 rows is the reference's; the CPU stand-in's non-lazy Adam copies it, so keep it narrow
    run_trainer_loops(tmp_path, "cpu", autofis_cpu_kernels, caplog, monkeypatch, emb=2, width=4, depth=1)


def small_batch(rng, z, B):
    return rng.integers(0, z["N"], size=(B, z["S"]), dtype=np.int64), (rng.random(B) < 0.5).astype(np.int64)


def check_resume_is_bit_identical(tmp_path, device, kernels):
    """Save after step 2 of stage 0, reload into a fresh layer: its step 3 equals the uninterrupted run's step 3 bit for
    bit — parameters, running statistics, Adam moments and the GRDA accumulator and counters."""
    from paddlerec_amd import checkpoint
    _, z = golden()
    rng = np.random.default_rng(11)
    batches = [small_batch(rng, z, 9) for _ in range(3)]
    T = lambda a: torch.as_tensor(a).to(device)
    torch.manual_seed(1)
    a = make_layer(z, device, kernels, grad_c=0.25)
    for ids, label in batches[:2]:
        a.train_step(T(ids), T(label), lr=0.01)
    path = checkpoint.save_model(a, None, str(tmp_path / "ck"), 0, prefix="rec")
    with open(os.path.join(path, "rec.pdopt"), "rb") as f:
        assert {"grda.acc", "grda.iterations", "grda.l1_accumulation"} <= set(pickle.load(f))
    torch.manual_seed(2)                                                             # another initial draw
    b = make_layer(z, device, kernels, grad_c=0.25)
    assert not torch.equal(a.grda_acc.cpu(), b.grda_acc.cpu())
    checkpoint.load_model(path, b)
    assert b.step_count == 2 and b.grda_iterations == 2 and b.grda_l1 == a.grda_l1 > 0
    la, _ = a.train_step(T(batches[2][0]), T(batches[2][1]), lr=0.01)
    lb, _ = b.train_step(T(batches[2][0]), T(batches[2][1]), lr=0.01)
    assert torch.equal(la.cpu(), lb.cpu())
    for k, v in a.state_dict().items():
        assert torch.equal(v.cpu(), b.state_dict()[k].cpu()), k
    assert torch.equal(a.rec.cpu(), b.rec.cpu())                                     # w's moments ride the record
    assert torch.equal(a.sparse_state["mv"].cpu(), b.sparse_state["mv"].cpu())
    assert torch.equal(a.dense.m.cpu(), b.dense.m.cpu()) and torch.equal(a.grda_acc.cpu(), b.grda_acc.cpu())
    assert b.grda_iterations == 3 and b.grda_l1 == a.grda_l1
    assert not bool(a.dense.pm[AR.MASK].any())                                       # Adam never saw mask in stage 0
    assert bool((a.dense.p[AR.MASK] == 0).any())                                     # GRDA did


def test_checkpoint_resume_is_bit_identical_cpu_backend(tmp_path):
    import autofis_cpu_kernels
    check_resume_is_bit_identical(tmp_path, "cpu", autofis_cpu_kernels)


def test_dygraph_model_plugin_surface():
    import autofis_cpu_kernels
    from paddlerec_amd import trainer
    from paddlerec_amd.autofis import DygraphModel
    assert "autofis" in trainer.MODELS and "autofis" in trainer.__doc__
    assert trainer.guess_model("/x/models/rank/autofis/config.yaml") == "autofis"
    dm = trainer._dygraph_model("autofis")
    assert isinstance(dm, DygraphModel)
    g, z = golden()
    cfg = dict(reference_config(), **{"hyper_parameters.num_inputs": z["S"], "hyper_parameters.input_size": z["N"],
                                      "hyper_parameters.embedding_size": z["D"], "hyper_parameters.width": z["width"],
                                      "hyper_parameters.depth": z["depth"], "hyper_parameters.pairs": z["P"],
                                      "hyper_parameters.optimizer.learning_rate": 1e-12})
    net = dm.create_model(cfg, "cpu", kernels=autofis_cpu_kernels)
    assert net.stage == 0 and net.grad_c == 0.0005 and net.grad_mu == 0.8 and net.num_pairs == z["P"]
    net.set_dict(params(g, "a_", z["depth"]))
    metrics, names = dm.create_metrics("cpu")
    assert names == ["auc", "log_loss"]
    loss, metrics, printed = dm.train_forward(net, metrics, (g["ids"], g["label"]), cfg)     # the reference's (x, y)
    assert_close_scaled(float(loss), g["a_loss"], REL, "loss")
    assert sorted(printed) == ["loss"] and printed["loss"] is loss
    assert int(metrics[0][0].sum() + metrics[0][1].sum()) == z["B"]
    want = AR.log_loss(g["a_pred"].astype(np.float64), g["label"])
    assert_close_scaled(dm.metric_value("log_loss", metrics[1]), want, REL, "log_loss")
    net.set_dict(params(g, "d_", z["depth"]))
    metrics, _ = dm.create_metrics("cpu")
    dm.infer_forward(net, metrics, (torch.as_tensor(g["label"]).reshape(-1, 1), torch.as_tensor(g["ids"])), cfg)
    dm.infer_forward(net, metrics, (g["ids"], g["label"]), cfg)
    assert int(metrics[1][1].item()) == 2
    assert_close_scaled(dm.metric_value("log_loss", metrics[1]), AR.log_loss(g["d_pred"].astype(np.float64), g["label"]),
                        REL, "eval log_loss")


def check_bad_arguments(device, kernels):
    from paddlerec_amd._lib import REC_AUTOFIS_MAX_PAIRS, RecError
    _, z = golden()
    AP = kernels.AutofisPairs
    AP([0, 0], [1, 2], 3, device)
    for cols, rows, S in (([1], [1], 3), ([2], [1], 3), ([0], [3], 3), ([-1], [1], 3), ([0, 1], [1], 3), ([], [], 3),
                          ([0] * 4, [1] * 4, 3), ([0], [1], 65), ([0], [1], 1)):
        with pytest.raises(RecError):
            AP(cols, rows, S, device)
    many = [(a, b) for a in range(64) for b in range(a + 1, 64)]
    assert len(many) == REC_AUTOFIS_MAX_PAIRS
    AP([a for a, _ in many], [b for _, b in many], 64, device)
    with pytest.raises(RecError):                                                    # P over the limit
        AP([a for a, _ in many] + [0], [b for _, b in many] + [1], 64, device)
    with pytest.raises(ValueError, match="kept no interaction"):                     # P = 0
        make_layer(z, device, kernels, 1, np.zeros(z["P"], np.int64))
    with pytest.raises(ValueError, match="comb_mask has"):                           # a wrong comb_mask length
        make_layer(z, device, kernels, 1, np.ones(z["P"] - 1, np.int64))
    with pytest.raises(ValueError):
        make_layer(z, device, kernels, 1, None)
    with pytest.raises(ValueError):
        make_layer(dict(z, P=z["P"] - 1), device, kernels)
    with pytest.raises(NotImplementedError):
        make_layer(z, device, kernels, use_bn=False)


def test_bad_arguments_are_rejected_cpu_backend():
    import autofis_cpu_kernels
    check_bad_arguments("cpu", autofis_cpu_kernels)
