"""TiSASRec (recall/tisas) without a GPU: tests/tisas_ref.py against the recordings of the reference's own files, the host
logic of paddlerec_amd/tisas.py over the CPU stand-ins (tests/tisas_cpu_kernels.py) against the same recordings, the reader
against what the reference's movielens_reader.py yields, and the refusals.  Tolerances: tests/tisas_checks.py."""
import os

import numpy as np
import pytest
import torch

import tisas_checks as TC
import tisas_cpu_kernels
import tisas_ref as R
from conftest import GOLDEN


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_ref_matches_the_golden(name):
    TC.check_golden(TC.gold(name))


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_layer_on_cpu_kernels_matches_the_golden(name):
    G = TC.gold(name)
    m = TC.layer_of(G, kernels=tisas_cpu_kernels)
    TC.check_layer(G, m, "cpu " + name[6:8])
    TC.check_infer(G, m, "cpu " + name[6:8])


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_state_dict_names_and_shapes(name):
    G = TC.gold(name)
    m = TC.layer_of(G, kernels=tisas_cpu_kernels)
    sd = m.state_dict()
    assert sorted(sd) == sorted(G["p"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(G["p"][k].shape), k
    assert tuple(sd["forward_layers.1.conv2.weight"].shape) == (8, 8, 1)
    m.set_dict(G["p"])
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), G["p"][k]), k
    ex = m.extra_optimizer_state()
    assert sorted(ex) == sorted("mtl.%s.%s" % (s, k) for s in "mv" for k in G["p"])
    ex["mtl.m.forward_layers.0.conv1.weight"] = np.arange(64, dtype=np.float32).reshape(8, 8, 1)
    m.set_extra_optimizer_state(ex)
    assert np.array_equal(m.extra_optimizer_state()["mtl.m.forward_layers.0.conv1.weight"].reshape(8, 8),
                          np.arange(64, dtype=np.float32).reshape(8, 8))


def test_dropout_streams_name_every_site():
    G = TC.gold(TC.FIXTURES[0])
    m = TC.layer_of(G, kernels=tisas_cpu_kernels, dropout_rate=0.2)
    s1, s2 = m.dropout_streams(1), m.dropout_streams(2)
    sites = ["emb", "pos_k", "pos_v", "time_k", "time_v"] + ["%s%d" % (n, b) for b in range(2) for n in ("att", "ffn1_", "ffn2_")]
    assert sorted(s1) == sorted(sites)
    assert len(set(s1.values()) | set(s2.values())) == 2 * len(sites)          # no stream is used twice
    assert TC.layer_of(G, kernels=tisas_cpu_kernels).dropout_streams(1) == {}


def test_layer_with_dropout_on_cpu_kernels():
    """Every dropout site on: the layer over the stand-ins against tisas_ref fed the masks rebuilt from dropout_streams."""
    G = TC.gold(TC.FIXTURES[1])
    m = TC.layer_of(G, kernels=tisas_cpu_kernels, dropout_rate=0.2, dropout_seed=99)
    TC.check_layer(G, m, "cpu drop", masks_of=masks_of(tisas_cpu_kernels.keep_mask))


def masks_of(keep_mask):
    """-> masks_of(m, step, B, L) for tisas_checks.check_layer; keep_mask(shape, p, seed, stream) rebuilds one mask."""
    def f(m, step, B, L):
        D, H = m.hidden_units, m.num_heads
        shapes = dict(emb=(B * L, D), pos_k=(B * L, D), pos_v=(B * L, D), time_k=(B * L * L, D), time_v=(B * L * L, D))
        for n in range(m.num_blocks):
            shapes.update({"att%d" % n: (B * H * L, L), "ffn1_%d" % n: (B * L, D), "ffn2_%d" % n: (B * L, D)})
        return {s: keep_mask(shapes[s], m.dropout_rate, m.dropout_seed, st) for s, st in m.dropout_streams(step).items()}
    return f


def test_refusals():
    from paddlerec_amd.tisas import QUIRKS, TiSASRecLayer
    with pytest.raises(ValueError, match="multiple of num_heads"):
        TiSASRecLayer(5, 11, 8, 6, 4, 2, 3, device="cpu", kernels=tisas_cpu_kernels)
    with pytest.raises(ValueError, match="limits"):
        TiSASRecLayer(5, 11, 8, 500, 4, 2, 1, device="cpu", kernels=tisas_cpu_kernels)
    with pytest.raises(ValueError, match="limits"):
        TiSASRecLayer(5, 11, 130, 6, 4, 2, 1, device="cpu", kernels=tisas_cpu_kernels)
    m = TiSASRecLayer(5, 11, 8, 6, 4, 2, 2, device="cpu", kernels=tisas_cpu_kernels)
    with pytest.raises(ValueError, match="time_matrices"):
        m.forward(torch.zeros(2, 6, dtype=torch.int64), torch.zeros(2, 6, 5, dtype=torch.int64),
                  torch.ones(2, 3, dtype=torch.int64))
    for word in ("10 000 users", "uniformly", "padding_idx", "0.98", "set order"):
        assert word in QUIRKS, word


def test_reader_refuses_the_branch_the_reference_cannot_run(tmp_path):
    from paddlerec_amd.reader import TisasDataset
    path = tmp_path / "big.txt"
    with open(path, "w") as f:
        for u in range(1, 10002):
            for j in range(5):
                f.write("%d\t%d\t%d\n" % (u, j + 1, 1000 + 3 * j))
    with pytest.raises(ValueError, match="10000 users"):
        TisasDataset([str(path)], 4, 4, "test")
    assert len(TisasDataset([str(path)], 4, 4, "train")) == 10001             # the train mode has no such branch


@pytest.mark.parametrize("case,fname,draws", [("sample", "tisas_sample.txt", 4), ("synth", "tisas_synth.txt", 6)])
def test_reader_matches_the_reference(case, fname, draws):
    from paddlerec_amd.reader import TisasDataset
    z = np.load(os.path.join(GOLDEN, "tisas_reader.npz"))
    for mode, cols in (("train", ("seq", "tm", "pos", "neg")), ("test", ("seq", "tm", "items"))):
        key = "%s_%s_" % (case, mode)
        maxlen, span, usernum, itemnum, n = (int(v) for v in z[key + "shape"])
        ds = TisasDataset([os.path.join(GOLDEN, fname)], maxlen, span, mode)
        assert (ds.usernum, ds.itemnum, len(ds)) == (usernum, itemnum, n)
        failed = set(z[key + "failed"].tolist())
        rows = []
        for i in range(draws if mode == "train" else n):
            if i in failed:                               # a test user without a valid item: the reference fails there too
                with pytest.raises(IndexError):
                    ds[i]
                continue
            rows.append(ds[i])
        assert len(rows) == len(z[key + cols[0]])
        for c, col in enumerate(cols):
            got = np.stack([r[c] for r in rows])
            assert got.dtype == np.int64 and np.array_equal(got, z[key + col]), (case, mode, col)
    if case == "synth":
        tm = z["synth_train_tm"]
        assert tm.max() == 6 and tm.min() == 0 and len(set(z["synth_train_seq"][:, 0] != 0)) == 2   # the clip; short and full rows


def test_reader_batches_like_the_reference_loader():
    from paddlerec_amd.reader import TisasDataset, TisasReader
    path = os.path.join(GOLDEN, "tisas_synth.txt")
    rd = TisasReader([path], 4, "cpu", 8, 6, "train")
    assert len(rd) == 13 // 4
    ds = TisasDataset([path], 8, 6, "train")
    want = [ds[i] for i in range(24)]
    got = [b for _ in range(2) for b in rd]               # two epochs: the draws carry on
    assert len(got) == 6
    for bi, b in enumerate(got):
        assert [tuple(t.shape) for t in b] == [(4, 8), (4, 8, 8), (4, 8), (4, 8)] and all(t.dtype == torch.int64 for t in b)
        for c in range(4):
            assert np.array_equal(b[c].numpy(), np.stack([want[bi * 4 + j][c] for j in range(4)]))


def test_head_with_nothing_selected_is_nan_with_zero_gradients():
    h = R.head(np.ones((3, 4)), np.zeros(3, np.int64), np.ones(3, np.int64), np.ones((5, 4)))
    assert np.isnan(h["loss"]) and not h["d_feats"].any() and not h["coef_pos"].any()


def test_trainer_train_then_infer_on_cpu_kernels(tmp_path):
    from paddlerec_amd import trainer
    cfg = TC.tisas_config(tmp_path, epochs=2)
    summaries, m = trainer.train(cfg, "tisas", "cpu", tisas_cpu_kernels)
    assert len(summaries) == 2 and all(np.isfinite(s["loss"]) and s["batches"] == 1 for s in summaries)
    assert m.step_count == 2
    out = trainer.infer(cfg, "tisas", "cpu", tisas_cpu_kernels)
    assert len(out) == 1 and out[0]["batches"] == 2 and 0.0 <= out[0]["NDCG@10"] <= out[0]["HR@10"] <= 1.0
