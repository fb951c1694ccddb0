"""PLE (models/multitask/ple) without a GPU: tests/mtl_ref.py (float64) against the goldens recorded from the reference's
net.py / dygraph_model.py, the layer on the CPU operator backend against them, the expert-indexing quirk, checkpoints and
the trainer.  Tolerances: mtl_checks.py."""
import numpy as np
import pytest
import torch

import mtl_checks as K
import mtl_cpu_kernels
import mtl_ref as R

FIXTURES = ("ple_init.npz", "ple_rand_l1.npz", "ple_rand_l2.npz")
UNUSED, TWICE = "lev_0.lev_0_exp_1_2", "lev_0.lev_0_exp_0_2"


@pytest.fixture(scope="module", params=FIXTURES)
def gold(request):
    return K.gold(request.param)


def test_goldens_hold_the_cases_they_are_meant_to():
    init, l1, l2 = (K.gold(n) for n in FIXTURES)
    assert init["steps"] == 3 and init["g"]["x_0"].shape == (2, 499) and len(init["plan"]["levels"]) == 1
    assert np.all(init["p"]["lev_0.lev_0_exp_1_1.weight"] == np.float32(1e-5))            # 10^-(1 + 1 * 3 + 1)
    assert np.all(init["p"]["lev_0.lev_0_exp_shared_1.weight"] == np.float32(1e-2))
    assert (len(l1["plan"]["levels"]), len(l2["plan"]["levels"])) == (1, 2)
    assert np.all(l2["p"]["lev_0.lev_0_gate_shared_.weight"] == l2["p"]["lev_0._param_gate_shared.weight"])
    assert "lev_1.lev_1_gate_shared_.weight" not in l2["p"] and l2["p"]["lev_1.lev_1_exp_0_0.weight"].shape == (6, 6)
    for G in (l1, l2):
        assert G["g"]["x_0"].shape == (7, 11) and G["g"]["label_0"].shape == (7, 2) and (G["g"]["x_0"] < 0).any()
        H = R.forward(G["p"], G["g"]["x_0"], G["g"]["label_0"], G["plan"])["tape"][0]["H"]
        assert 0.1 < (H == 0).mean() < 0.9
        # level 0 runs the twice-used expert on the same features: slots 2 and 3 hold the same columns
        assert np.array_equal(H[:, 12:18], H[:, 18:24])


def test_float64_reference_matches_every_array_of_the_golden(gold):
    K.check_golden(gold)


def test_layer_on_cpu_kernels_matches_the_reference(gold):
    K.check_layer(gold, K.layer_of(gold, "cpu", mtl_cpu_kernels), "cpu mirror")


def test_state_dict_and_initial_values_are_the_references():
    from paddlerec_amd.ple import QUIRKS, DygraphModel
    for name, levels in (("ple_init.npz", 1), ("ple_rand_l2.npz", 2)):
        G = K.gold(name)
        F, S = G["p"]["lev_0.lev_0_exp_0_0.weight"].shape
        cfg = {"hyper_parameters.feature_size": F, "hyper_parameters.task_num": 2, "hyper_parameters.exp_per_task": 3,
               "hyper_parameters.shared_num": 2, "hyper_parameters.expert_size": S,
               "hyper_parameters.tower_size": G["p"]["tower_0.weight"].shape[1], "hyper_parameters.level_number": levels}
        m = DygraphModel().create_model(cfg, device="cpu", kernels=mtl_cpu_kernels)
        sd = m.state_dict()
        assert sorted(sd) == sorted(G["p"])
        for k, v in sd.items():
            assert tuple(v.shape) == G["p"][k].shape, k
            if levels == 1:
                assert np.array_equal(v.numpy(), G["p"][k]), k                 # the reference's constants
        if levels == 2:
            assert sd["lev_0._param_gate_shared.weight"] is sd["lev_0.lev_0_gate_shared_.weight"]
            assert np.all(sd["lev_0.lev_0_gate_shared_.weight"].numpy() == np.float32(0.1))
            assert [len(lev["images"]) for lev in m.levels] == [1, 3]            # level 0: one image; level 1: one per input
    assert "i * task_num + j" in QUIRKS and "exp_1_2" in QUIRKS


def test_the_expert_indexing_quirk():
    G = K.gold("ple_rand_l1.npz")
    m = K.layer_of(G, "cpu", mtl_cpu_kernels)
    m.set_dict(G["p"])
    assert [n.split("_exp_")[1] for _, n, _ in m.slot_map(0)] == ["0_0", "0_1", "0_2", "0_2", "1_0", "1_1", "shared_0", "shared_1"]
    assert [i for _, _, i in m.slot_map(0)] == [0, 0, 0, 1, 1, 1, 2, 2] and m.unused() == [UNUSED]
    x, y = torch.as_tensor(G["g"]["x_0"]), torch.as_tensor(G["g"]["label_0"])
    m.train_step(x, y, G["lr"])
    g, sd = m.last_gradients(), m.state_dict()
    assert UNUSED + ".weight" not in g and "g_0_" + UNUSED + ".weight" not in G["g"]
    assert np.array_equal(sd[UNUSED + ".weight"].numpy(), G["p"][UNUSED + ".weight"])
    assert np.array_equal(G["g"]["n_0_" + UNUSED + ".bias"], G["p"][UNUSED + ".bias"])
    # the twice-used expert: its gradient is the sum of its two slots (columns 12:18 and 18:24 of dH), in slot order
    c = R.forward(G["p"], G["g"]["x_0"], G["g"]["label_0"], G["plan"])
    r64 = K.ref_step(G["p"], None, G["g"]["x_0"], G["g"]["label_0"], G["lr"], G["plan"])[0]
    tp = c["tape"][0]
    dtop = np.zeros((7, 12))
    for t in range(2):
        wo, a = G["p"]["tower_out_%d.weight" % t].astype(np.float64), c["acts"][t]
        da = np.where(a > 0, c["dz"][:, 2 * t + 1:2 * t + 2] * (wo[:, 1] - wo[:, 0])[None, :], 0)
        dtop[:, 6 * t:6 * t + 6] = da @ G["p"]["tower_%d.weight" % t].astype(np.float64).T
    dH, _ = R.mix_bwd(tp["H"], tp["prob"], dtop, 6, 8, [gt[2] for gt in G["plan"]["levels"][0]["gates"]])
    xs = G["g"]["x_0"].astype(np.float64)
    both = xs.T @ dH[:, 12:18] + xs.T @ dH[:, 18:24]
    assert R.relerr(both, r64["g"][TWICE + ".weight"]) < 1e-12 and np.abs(xs.T @ dH[:, 18:24]).max() > 0
    assert R.relerr(g[TWICE + ".weight"].numpy(), both) <= K.bound_of(K.gold("ple_rand_l1.npz")["r32"][0]["g"][TWICE + ".weight"], both)
    (im,) = m.levels[0]["images"]                                               # both copies of the expert moved alike
    (w2, b2), (w3, b3) = im["img"].part("p", 2), im["img"].part("p", 3)
    assert torch.equal(w2, w3) and torch.equal(b2, b3) and not np.array_equal(w2.numpy(), G["p"][TWICE + ".weight"])


def test_a_config_whose_expert_index_overruns_is_refused():
    from paddlerec_amd.ple import DygraphModel, ple_plan
    with pytest.raises(ValueError, match=r"i \* task_num \+ j.*IndexError"):
        ple_plan(11, 3, 1, 1, 6, 4, 1)                                          # index 2 * 3 + 0 = 6 of 4 experts
    cfg = {"hyper_parameters.feature_size": 11, "hyper_parameters.task_num": 4, "hyper_parameters.exp_per_task": 2,
           "hyper_parameters.shared_num": 1, "hyper_parameters.expert_size": 6, "hyper_parameters.tower_size": 4,
           "hyper_parameters.level_number": 1}
    with pytest.raises(ValueError, match="IndexError"):
        DygraphModel().create_model(cfg, device="cpu", kernels=mtl_cpu_kernels)
    with pytest.raises(ValueError, match="shared_num"):
        ple_plan(11, 2, 3, 0, 6, 4, 1)
    ple_plan(11, 2, 4, 1, 6, 4, 1)                                              # largest index 5 of 9: fine, two experts twice


def test_checkpoint_reproduces_the_next_step_bit_for_bit(tmp_path):
    from paddlerec_amd import checkpoint
    G = K.gold("ple_rand_l2.npz")
    x, y = torch.as_tensor(G["g"]["x_0"]), torch.as_tensor(G["g"]["label_0"])
    m = K.layer_of(G, "cpu", mtl_cpu_kernels)
    m.set_dict(G["p"])
    m.train_step(x, y, G["lr"])
    d = checkpoint.save_model(m, None, str(tmp_path), 0)
    m2 = K.layer_of(G, "cpu", mtl_cpu_kernels)
    checkpoint.load_model(d, m2)
    a, b = m.train_step(x, y, G["lr"]), m2.train_step(x, y, G["lr"])
    assert m2.step_count == 2 and torch.equal(a[0].value(), b[0].value()) and torch.equal(a[1], b[1])
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k


def test_trainer_knows_the_model_trains_and_resumes(tmp_path):
    from paddlerec_amd import checkpoint, trainer
    assert "ple" in trainer.MODELS and "ple" in trainer.__doc__
    assert trainer.guess_model("/x/models/multitask/ple/config.yaml") == "ple"
    assert type(trainer._dygraph_model("ple")).__module__ == "paddlerec_amd.ple"
    cfg = K.census_config(tmp_path, "ple")
    out, m = trainer.train(cfg, "ple", device="cpu", kernels=mtl_cpu_kernels)
    assert len(out) == 2 and out[1]["batches"] == 4 and np.isfinite(out[1]["loss"]) and m.step_count == 8
    assert 0.0 <= out[1]["auc_income"] <= 1.0 and 0.0 <= out[1]["auc_marital"] <= 1.0
    res = trainer.infer(cfg, "ple", device="cpu", kernels=mtl_cpu_kernels)
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 8
    m2 = trainer._dygraph_model("ple").create_model(cfg, "cpu", kernels=mtl_cpu_kernels)
    checkpoint.load_model(out[1]["model_dir"], m2)
    batch = next(iter(trainer.create_data_loader(cfg, "ple", "cpu")()))
    dm = trainer._dygraph_model("ple")
    la, _, _ = dm.train_forward(m, dm.create_metrics("cpu")[0], batch, cfg)
    lb, _, _ = dm.train_forward(m2, dm.create_metrics("cpu")[0], batch, cfg)
    assert m2.step_count == 9 and torch.equal(la.value(), lb.value())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
