"""MMoE (models/multitask/mmoe) without a GPU: tests/mtl_ref.py (float64) against the goldens recorded from the reference's
net.py / dygraph_model.py, the layer on the CPU operator backend against them, the census reader, checkpoints and the
trainer; the argument checks of the rec_mtl_* entry points (they return before any launch).  Tolerances: mtl_checks.py."""
import os

import numpy as np
import pytest
import torch

import mtl_checks as K
import mtl_cpu_kernels
import mtl_ref as R
from conftest import GOLDEN

FIXTURES = ("mmoe_init.npz", "mmoe_rand.npz")


@pytest.fixture(scope="module", params=FIXTURES)
def gold(request):
    return K.gold(request.param)


def test_goldens_hold_the_cases_they_are_meant_to():
    init, rand = K.gold("mmoe_init.npz"), K.gold("mmoe_rand.npz")
    assert init["steps"] == 3 and init["g"]["x_0"].shape == (2, 499) and init["p"]["expert_7.weight"].shape == (499, 16)
    assert np.all(init["p"]["expert_2.weight"] == np.float32(1e-3)) and np.all(init["p"]["gate_1.weight"] == np.float32(1e-2))
    assert np.all(init["p"]["tower_1.weight"] == np.float32(1e-2)) and np.all(init["p"]["tower_out_1.bias"] == np.float32(0.1))
    assert rand["steps"] == 1 and rand["g"]["x_0"].shape == (7, 11) and rand["g"]["label_0"].shape == (7, 3)
    assert len(rand["plan"]["levels"][0]["slots"]) == 5 and rand["plan"]["tasks"] == 3
    assert rand["p"]["expert_0.weight"].shape == (11, 6) and rand["p"]["tower_0.weight"].shape == (6, 4)
    w = rand["p"]["expert_3.weight"]
    assert len(np.unique(w)) == w.size and (rand["g"]["x_0"] < 0).any()         # no two columns alike; some ReLUs are off
    c = R.forward(rand["p"], rand["g"]["x_0"], rand["g"]["label_0"], rand["plan"])
    H = c["tape"][0]["H"]
    assert 0.1 < (H == 0).mean() < 0.9
    for t in range(3):
        assert set(rand["g"]["label_0"][:, t].tolist()) == {0.0, 1.0}


def test_float64_reference_matches_every_array_of_the_golden(gold):
    K.check_golden(gold)


def test_layer_on_cpu_kernels_matches_the_reference(gold):
    K.check_layer(gold, K.layer_of(gold, "cpu", mtl_cpu_kernels), "cpu mirror")


def test_state_dict_and_initial_values_are_the_references():
    from paddlerec_amd.mmoe import QUIRKS, DygraphModel
    G = K.gold("mmoe_init.npz")
    cfg = {"hyper_parameters.feature_size": 499, "hyper_parameters.expert_num": 8, "hyper_parameters.gate_num": 2,
           "hyper_parameters.expert_size": 16, "hyper_parameters.tower_size": 8}
    m = DygraphModel().create_model(cfg, device="cpu", kernels=mtl_cpu_kernels)
    sd = m.state_dict()
    assert sorted(sd) == sorted(G["p"]) and len(m.parameters()) == len(sd)
    for k, v in sd.items():
        assert tuple(v.shape) == G["p"][k].shape and np.array_equal(v.numpy(), G["p"][k]), k
    assert "GATE" in QUIRKS and "marital, income" in QUIRKS
    # all experts and gates are one image: [499, 8 * 16 + 2 * 8]
    (lev,) = m.levels
    (im,) = lev["images"]
    assert (im["img"].K, im["img"].N) == (499, 144) and sd["gate_1.weight"].data_ptr() == im["img"].view["p"]["W"][:, 136:].data_ptr()


def test_forward_is_one_gemm_for_all_experts_and_gates():
    G = K.gold("mmoe_rand.npz")
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(mtl_cpu_kernels, name)
            if name != "gemm":
                return fn
            return lambda A, B, *a, **kw: (calls.append((tuple(A.shape), tuple(B.shape))), fn(A, B, *a, **kw))[1]

    m = K.layer_of(G, "cpu", Counting())
    m.set_dict(G["p"])
    preds = m.forward(torch.as_tensor(G["g"]["x_0"]))
    assert calls[0] == ((7, 11), (11, 5 * 6 + 3 * 5)) and len(calls) == 1 + 2 * 3          # the image, then two per tower
    assert len(preds) == 3 and R.relerr(torch.cat(preds, 1).numpy(), G["r64"][0]["pred"]) <= K.bound_of(G["r32"][0]["pred"], G["r64"][0]["pred"])


def test_checkpoint_reproduces_the_next_step_bit_for_bit(tmp_path):
    from paddlerec_amd import checkpoint
    G = K.gold("mmoe_rand.npz")
    x, y = torch.as_tensor(G["g"]["x_0"]), torch.as_tensor(G["g"]["label_0"])
    m = K.layer_of(G, "cpu", mtl_cpu_kernels)
    m.set_dict(G["p"])
    m.train_step(x, y, G["lr"])
    d = checkpoint.save_model(m, None, str(tmp_path), 0)
    m2 = K.layer_of(G, "cpu", mtl_cpu_kernels)
    checkpoint.load_model(d, m2)
    assert m2.step_count == 1
    a, b = m.train_step(x, y, G["lr"]), m2.train_step(x, y, G["lr"])
    assert torch.equal(a[0].value(), b[0].value()) and torch.equal(a[1], b[1])
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k


# ------------------------------------------------------------------------------------------------ reader, trainer
def test_reader_reproduces_the_reference_readers_rows(tmp_path):
    from paddlerec_amd.reader import CensusReader
    want = np.load(os.path.join(GOLDEN, "census_reader.npz"))
    sample = os.path.join(GOLDEN, "census_sample.txt")
    bs = list(CensusReader([sample], 3, "cpu"))
    assert len(bs) == 2                                                        # drop_last: 8 lines, batches of 3
    for i, (x, inc, mar) in enumerate(bs):
        assert x.dtype == inc.dtype == mar.dtype == torch.float32 and tuple(inc.shape) == tuple(mar.shape) == (3, 1)
        assert np.array_equal(x.numpy(), want["features"][3 * i:3 * i + 3])
        assert np.array_equal(inc.numpy(), want["label_income"][3 * i:3 * i + 3].astype(np.float32))
        assert np.array_equal(mar.numpy(), want["label_marital"][3 * i:3 * i + 3].astype(np.float32))
    assert len(list(CensusReader([sample, sample], 3, "cpu"))) == 5             # drop_last over the concatenation
    assert want["label_income"].min() == 0 and want["label_marital"].max() == 1
    bad = tmp_path / "bad.txt"
    with open(sample) as f:
        lines = f.readlines()
    lines[1] = "0,2," + lines[1].split(",", 2)[2]
    bad.write_text("".join(lines))
    with pytest.raises(ValueError, match=r"bad\.txt:2: label_income"):
        list(CensusReader([str(bad)], 2, "cpu"))
    lines[1] = "0.5,1," + lines[1].split(",", 2)[2]                          # the reference's int() would make it 0
    bad.write_text("".join(lines))
    with pytest.raises(ValueError, match=r"bad\.txt:2: label_marital is 0\.5"):
        list(CensusReader([str(bad)], 2, "cpu"))


def test_trainer_knows_the_model_trains_and_resumes(tmp_path):
    from paddlerec_amd import checkpoint, trainer
    assert "mmoe" in trainer.MODELS and "mmoe" in trainer.__doc__
    assert trainer.guess_model("/x/models/multitask/mmoe/config.yaml") == "mmoe"
    assert type(trainer._dygraph_model("mmoe")).__module__ == "paddlerec_amd.mmoe"
    cfg = K.census_config(tmp_path, "mmoe")
    out, m = trainer.train(cfg, "mmoe", device="cpu", kernels=mtl_cpu_kernels)
    assert len(out) == 2 and out[1]["batches"] == 4 and np.isfinite(out[1]["loss"]) and m.step_count == 8
    assert 0.0 <= out[1]["auc_income"] <= 1.0 and 0.0 <= out[1]["auc_marital"] <= 1.0
    res = trainer.infer(cfg, "mmoe", device="cpu", kernels=mtl_cpu_kernels)
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 8 and "auc_marital" in res[1]
    m2 = trainer._dygraph_model("mmoe").create_model(cfg, "cpu", kernels=mtl_cpu_kernels)
    checkpoint.load_model(out[1]["model_dir"], m2)
    batch = next(iter(trainer.create_data_loader(cfg, "mmoe", "cpu")()))
    dm = trainer._dygraph_model("mmoe")
    la, _, _ = dm.train_forward(m, dm.create_metrics("cpu")[0], batch, cfg)
    lb, _, _ = dm.train_forward(m2, dm.create_metrics("cpu")[0], batch, cfg)
    assert m2.step_count == 9 and torch.equal(la.value(), lb.value())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k


# ------------------------------------------------------------------------------------------------ argument checks
def test_mtl_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    K.run_refusals(engine_lib)
    from paddlerec_amd import _lib
    names = [n for n in _lib.SIGNATURES if n.startswith("rec_mtl_")]
    assert sorted(names) == ["rec_mtl_head", "rec_mtl_mix_bwd", "rec_mtl_mix_fwd"] and not any(n.endswith("_bytes") for n in names)
