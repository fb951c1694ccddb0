"""ESCM2 (models/multitask/escm2) without a GPU: tests/esm_ref.py (float64) against the goldens recorded from the reference's
net.py / dygraph_model.py in the IPW and the DR mode, the layer on the CPU operator backend against them, the AliCCP reader,
checkpoints and the trainer.  Tolerances: esm_checks.py."""
import os

import numpy as np
import pytest
import torch

import esm_checks as K
import esm_cpu_kernels
import esm_ref as R
from conftest import GOLDEN


@pytest.fixture(scope="module", params=K.FIXTURES["escm2"])
def gold(request):
    return K.gold(request.param)


def test_goldens_hold_the_cases_they_are_meant_to():
    for name, mode, gates in (("escm2_ipw_rand.npz", "IPW", 2), ("escm2_dr_rand.npz", "DR", 3)):
        G = K.gold(name)
        g, p = G["g"], G["p"]
        assert G["steps"] == 2 and G["cfg"] == dict(mode=mode, global_w=0.5, counterfactual_w=0.3)
        assert p["embedding.weight"].shape == (61, 4) and not p["embedding.weight"][0].any()
        assert sum(1 for k in p if k.startswith("gate_") and k.endswith(".weight")) == gates
        assert p["expert_2.weight"].shape == (12, 6) and p["tower_out_1.weight"].shape == (4, 2) and "expert_3.weight" not in p
        for s in range(2):
            ids, click, buy = g["ids_%d" % s], g["click_%d" % s], g["buy_%d" % s]
            assert ids.shape == (7, 3, 3) and g["outs_%d" % s].shape == (7, 9 + (gates == 3))
            assert (ids == 0).any() and (ids == 0).all(2).any() and ids.max() < 61           # padding, an all-padding field
            assert ids[3, 0, 0] == ids[3, 0, 1] != 0 and np.array_equal(ids[4, 2], ids[0, 2])  # duplicates
            assert {(0, 0), (1, 0), (1, 1)} <= set(zip(click.tolist(), buy.tolist()))
            assert g["g_%d_embedding.weight" % s].shape == (61, 4) and not g["g_%d_embedding.weight" % s][0].any()


def test_float64_reference_matches_every_array_of_the_golden(gold):
    K.check_golden(gold)


def test_layer_on_cpu_kernels_matches_the_reference(gold):
    m = K.layer_of(gold, "cpu", esm_cpu_kernels)
    assert sorted(m.state_dict()) == sorted(gold["p"]) and len(m.parameters()) == len(gold["p"])
    K.check_layer(gold, m, "cpu mirror")
    assert m.step_count == 2


def test_forward_returns_the_references_out_list(gold):
    m = K.layer_of(gold, "cpu", esm_cpu_kernels)
    m.set_dict(gold["p"])
    outs = m.forward(torch.as_tensor(gold["g"]["ids_0"]))
    assert len(outs) == (7 if gold["cfg"]["mode"] == "DR" else 6) and [o.shape[1] for o in outs[:6]] == [2, 1, 2, 1, 2, 1]
    got = torch.cat(outs, 1).numpy()
    assert R.relerr(got, gold["r64"][0]["outs"]) <= K.bound_of(gold["r32"][0]["outs"], gold["r64"][0]["outs"])


def test_features_are_pooled_straight_into_one_gemm():
    G = K.gold("escm2_dr_rand.npz")
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(esm_cpu_kernels, name)
            if name not in ("gemm", "field_sumpool_fwd"):
                return fn
            return lambda *a, **kw: (calls.append((name, tuple(a[0].shape), tuple(a[1].shape))), fn(*a, **kw))[1]

    m = K.layer_of(G, "cpu", Counting())
    m.set_dict(G["p"])
    m.forward(torch.as_tensor(G["g"]["ids_0"]))
    assert calls[0] == ("field_sumpool_fwd", (7, 3, 3), (61, 4))
    assert calls[1] == ("gemm", (7, 12), (12, 3 * 6 + 3 * 3)) and len(calls) == 2 + 2 * 3     # the image, two per tower


def test_initial_values_quirks_and_refusals():
    from paddlerec_amd.escm2 import QUIRKS, DygraphModel, ESCMLayer
    base = {"hyper_parameters.sparse_feature_number": 50, "hyper_parameters.sparse_feature_dim": 4, "hyper_parameters.num_field": 3,
            "hyper_parameters.ctr_fc_sizes": [256, 64], "hyper_parameters.cvr_fc_sizes": [256, 64], "hyper_parameters.gate_num": 7,
            "hyper_parameters.feature_size": 12, "hyper_parameters.expert_num": 8, "hyper_parameters.expert_size": 16,
            "hyper_parameters.tower_size": 8, "hyper_parameters.global_w": 1.0, "hyper_parameters.counterfactual_w": 0.01}
    torch.manual_seed(3)
    for mode, gates in (("DR", 3), ("IPW", 2)):
        m = DygraphModel().create_model(dict(base, **{"runner.counterfact_mode": mode}), device="cpu", kernels=esm_cpu_kernels)
        sd = m.state_dict()
        assert m.gate_num == gates and "gate_%d.weight" % (gates - 1) in sd and "gate_%d.weight" % gates not in sd   # gate_num 7 ignored
        assert list(sd)[0] == "embedding.weight" and not sd["embedding.weight"][0].any() and sd["embedding.weight"][1:].abs().max() <= 1
        assert (m.global_w, m.counterfactual_w) == (1.0, 0.01) and m.emb.max_len == 3
        for k, v in sd.items():
            if k.endswith(".bias"):
                assert torch.all(v == np.float32(0.1)), k
            elif k != "embedding.weight":
                lim = np.sqrt(6.0 / sum(v.shape))
                assert v.abs().max() <= lim and v.abs().max() > 0.5 * lim and len(torch.unique(v)) > v.numel() // 2, k
        (lev,) = m.levels
        (im,) = lev["images"]
        assert (im["img"].K, im["img"].N) == (12, 8 * 16 + gates * 8)
    for word in ("ctr_fc_sizes", "cvr_fc_sizes", "gate_num", "infer_forward", "seven"):
        assert word in QUIRKS
    with pytest.raises(ValueError, match="feature_size is 13 .* 3 \\* 4 = 12"):
        ESCMLayer(50, 4, 3, None, None, 8, 16, 8, "DR", 13, device="cpu", kernels=esm_cpu_kernels)
    for bad in ("dr", None, "ESMM"):
        with pytest.raises(ValueError, match="unknown runner.counterfact_mode"):
            ESCMLayer(50, 4, 3, None, None, 8, 16, 8, bad, 12, device="cpu", kernels=esm_cpu_kernels)
    m = ESCMLayer(50, 4, 3, None, None, 2, 4, 4, "IPW", 12, device="cpu", kernels=esm_cpu_kernels)
    with pytest.raises(ValueError, match=r"ids int64 \[B, 3, 3\]"):
        m.forward(torch.zeros(2, 3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="click and buy"):
        m.train_step(torch.zeros(2, 3, 3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))


def test_checkpoint_keeps_the_moments_and_reproduces_the_next_step(tmp_path, gold):
    from paddlerec_amd import checkpoint
    m = K.layer_of(gold, "cpu", esm_cpu_kernels)
    m.set_dict(gold["p"])
    m.train_step(*K.feeds(gold, 0, "cpu"), gold["lr"])
    d = checkpoint.save_model(m, None, str(tmp_path), 0)
    m2 = K.layer_of(gold, "cpu", esm_cpu_kernels)
    checkpoint.load_model(d, m2)
    assert m2.step_count == 1 and m.emb.m.abs().max() > 0
    a, b = m.extra_optimizer_state(), m2.extra_optimizer_state()
    assert sorted(a) == sorted(b) and "mtl.v.embedding.weight" in a and "mtl.m.gate_1.bias" in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    x, y = m.train_step(*K.feeds(gold, 1, "cpu"), gold["lr"]), m2.train_step(*K.feeds(gold, 1, "cpu"), gold["lr"])
    assert torch.equal(x[0].value(), y[0].value()) and torch.equal(x[1], y[1])
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k


# ------------------------------------------------------------------------------------------------ reader, trainer
def test_reader_reproduces_the_reference_readers_rows():
    from paddlerec_amd.reader import AliCCPReader
    want = np.load(os.path.join(GOLDEN, "aliccp_reader.npz"))
    sample = os.path.join(GOLDEN, "aliccp_sample.txt")
    assert want["ids"].shape == (4, 23, 3) and (want["ids"] == 0).any() and want["click"].tolist() == [1, 0, 1, 0]
    bs = list(AliCCPReader([sample], 3, "cpu"))
    assert len(bs) == 1                                                        # drop_last: 4 lines, batches of 3
    ids, click, buy = bs[0]
    assert ids.dtype == click.dtype == buy.dtype == torch.int64 and tuple(click.shape) == tuple(buy.shape) == (3,)
    assert np.array_equal(ids.numpy(), want["ids"][:3]) and np.array_equal(click.numpy(), want["click"][:3])
    assert np.array_equal(buy.numpy(), want["buy"][:3])
    both = list(AliCCPReader([sample, sample], 3, "cpu"))                      # drop_last over the concatenation
    assert len(both) == 2 and np.array_equal(both[1][0].numpy(), want["ids"][[3, 0, 1]])
    with open(sample) as f:
        first = f.readline().strip().split(",")
    per_field = {}
    for elem in first[4:]:
        per_field.setdefault(elem.split(":")[0], []).append(int(elem.split(":")[1]))
    assert len(per_field["150_14"]) > 3 and "999" not in AliCCPReader.FIELDS                     # a field that is truncated
    (one,) = list(AliCCPReader([sample], 4, "cpu", max_len=5))
    f150 = AliCCPReader.FIELDS.index("150_14")
    assert one[0].shape == (4, 23, 5) and one[0][0, f150].tolist() == per_field["150_14"][:5]
    assert np.array_equal(one[0][:, :, :3].numpy()[want["ids"] != 0], want["ids"][want["ids"] != 0])


@pytest.mark.parametrize("mode", ["DR", "IPW"])
def test_trainer_knows_the_model_trains_infers_and_resumes(tmp_path, mode):
    from paddlerec_amd import checkpoint, trainer
    assert "escm2" in trainer.MODELS and "escm2" in trainer.__doc__
    assert trainer.guess_model("/x/models/multitask/escm2/config.yaml") == "escm2"
    assert type(trainer._dygraph_model("escm2")).__module__ == "paddlerec_amd.escm2"
    cfg = K.aliccp_config(tmp_path, "escm2", mode=mode)
    out, m = trainer.train(cfg, "escm2", device="cpu", kernels=esm_cpu_kernels)
    assert len(out) == 2 and out[1]["batches"] == 2 and np.isfinite(out[1]["loss"]) and m.step_count == 4
    assert m.n_tasks == (3 if mode == "DR" else 2)
    for n in ("auc_ctr", "auc_cvr", "auc_ctcvr"):
        assert 0.0 <= out[1][n] <= 1.0
    res = trainer.infer(cfg, "escm2", device="cpu", kernels=esm_cpu_kernels)           # both modes: QUIRKS
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 4 and "auc_ctcvr" in res[1]
    m2 = trainer._dygraph_model("escm2").create_model(cfg, "cpu", kernels=esm_cpu_kernels)
    checkpoint.load_model(out[1]["model_dir"], m2)
    batch = next(iter(trainer.create_data_loader(cfg, "escm2", "cpu")()))
    dm = trainer._dygraph_model("escm2")
    la, _, _ = dm.train_forward(m, dm.create_metrics("cpu")[0], batch, cfg)
    lb, _, _ = dm.train_forward(m2, dm.create_metrics("cpu")[0], batch, cfg)
    assert m2.step_count == 5 and torch.equal(la.value(), lb.value())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
