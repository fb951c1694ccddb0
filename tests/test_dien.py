"""DIEN without a GPU: the float64 restatement (tests/dien_ref.py) against the golden recorded from the reference's own
net.py (tools/make_golden_dien.py), DIENLayer's host logic on a CPU stand-in backend (tests/dien_cpu_kernels.py), the
reader against the reference reader's recorded batches, and the argument checks of the new entry points.

Bounds.  The golden is a float32 torch run; the float64 restatement agrees with it to that run's own rounding.  The
error is max|got - ref| / max|ref| per tensor and the bound 2e-5 — about ten float32 roundings of a sum over a few
dozen terms; measured at most 1.4e-6 (gradients) and 2.5e-7 (logit).  The stand-in computes in float32, so DIENLayer's
step is held to the same bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dien_cpu_kernels
import dien_ref as R
from conftest import GOLDEN

FEEDS = ("hist_item_seq", "hist_cat_seq", "target_item", "target_cat", "label", "mask", "target_item_seq",
         "target_cat_seq", "neg_hist_item_seq", "neg_hist_cat_seq")
BOUND = 2e-5


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLDEN, "dien_D8.npz"))
    p = {k[2:]: g[k] for k in g.files if k.startswith("p_")}
    att = ([g["att_w%d" % i] for i in range(3)], [g["att_b%d" % i] for i in range(3)])
    feeds = [g[k] for k in FEEDS]
    fw = R.forward(p, att, feeds)
    return dict(g=g, p=p, att=att, feeds=feeds, fw=fw, grads=R.backward(p, att, feeds, fw))


def test_golden_holds_the_cases_it_is_meant_to(gold):
    g = gold["g"]
    assert tuple(g["sizes"]) == (4, 4, 5, 6, 31, 29) and 1 in g["lens"]
    for k in ("hist_item_seq", "hist_cat_seq"):                # id 0 at a valid position, duplicates
        valid = np.arange(6)[None, :] < g["lens"][:, None]
        assert (g[k][valid] == 0).any() and len(np.unique(g[k][valid])) < valid.sum()
    assert (g["target_item"] == 0).any() and (g["neg_hist_item_seq"] == 0).any()
    for k in ("linear_0.bias", "linear_2.bias", "item_b_attr.weight", "gru_net.bias_hh_l1", "gru_cell_attention.bias_ih"):
        assert np.abs(g["p_" + k]).min() > 0, k                # a dropped bias shows
    assert all(np.abs(g["att_b%d" % i]).min() > 0 for i in range(3))
    assert sorted(k[2:] for k in g.files if k.startswith("p_")) == sorted(
        [n + ".weight" for n in R.TABLES] + ["item_b_attr.weight"] +
        ["linear_%d.%s" % (i, s) for i in range(3) for s in ("weight", "bias")] +
        [pat % k for pat in R.GRUS for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])


def test_float64_reference_matches_every_array_of_the_golden(gold):
    g, fw, grads, p = gold["g"], gold["fw"], gold["grads"], gold["p"]
    for k in ("logit", "aux", "loss", "cost"):
        e = R.relerr(fw[k], g[k])
        print(k, e)
        assert e < BOUND, (k, e)
    new = R.sgd_step(p, grads, float(g["lr"][0]))
    for k in p:
        e, e2 = R.relerr(grads[k], g["g_" + k]), R.relerr(new[k], g["n_" + k])
        print(k, e, e2)
        assert e < BOUND and e2 < BOUND, (k, e, e2)
    for n in R.TABLES:                                          # the padding row gets no gradient
        assert not grads[n + ".weight"][0].any() and not g["g_" + n + ".weight"][0].any()


def _layer(gold, **kw):
    from paddlerec_amd.dien import DIENLayer
    m = DIENLayer(4, 4, "sigmoid", False, False, 31, 29, device="cpu", kernels=dien_cpu_kernels, **kw)
    m.set_dict(gold["p"])
    m.set_attention(*gold["att"])
    return m


def test_layer_forward_and_train_step_match_the_golden_on_the_stand_in(gold):
    g = gold["g"]
    m = _layer(gold)
    feeds = [torch.as_tensor(a) for a in gold["feeds"]]
    logit, aux = m.forward(*feeds)
    assert R.relerr(logit.numpy(), g["logit"]) < BOUND and R.relerr(aux.numpy(), g["aux"]) < BOUND
    att_before = [w.clone() for w in m.attention_w + m.attention_b]
    rows0 = {n: m.params[n + ".weight"][0].clone() for n in R.TABLES}
    cost, pred, aux = m.train_step(*feeds, base_lr=float(g["lr"][0]))
    assert R.relerr(cost.numpy(), g["cost"]) < BOUND and R.relerr(aux.numpy(), g["aux"]) < BOUND
    assert R.relerr(pred.numpy(), 1 / (1 + np.exp(-g["logit"].astype(np.float64)))) < BOUND
    for k, v in m.state_dict().items():
        e = R.relerr(v.numpy(), g["n_" + k])
        assert e < BOUND, (k, e)
    for n in R.TABLES:                                          # row 0 of every padded table: bit-unchanged
        assert torch.equal(m.params[n + ".weight"][0], rows0[n]), n
    assert not torch.equal(m.params["item_b_attr.weight"], torch.as_tensor(g["p_item_b_attr.weight"]))
    assert all(torch.equal(a, b) for a, b in zip(m.attention_w + m.attention_b, att_before))   # used, never trained
    assert not any("attention" in k and "gru" not in k for k in m.state_dict())
    assert sorted(m.state_dict()) == sorted(k[2:] for k in g.files if k.startswith("p_"))
    assert int(m.status.item()) == 0


def test_state_dict_round_trip_and_alias_keys(gold):
    m, m2 = _layer(gold), _layer(gold)
    sd = {k: v.numpy() + 0.25 for k, v in m.state_dict().items()}
    alias = {}
    for k, v in sd.items():
        if k.startswith("gru_net."):                            # gru_net.weight_ih_l1 -> gru_net.1.cell.weight_ih
            name, layer = k[len("gru_net."):].rsplit("_l", 1)
            k = "gru_net.%s.cell.%s" % (layer, name)
        alias[k] = v
    assert any(".cell." in k for k in alias)
    m.set_dict(sd)
    m2.set_dict(alias)
    for k in sd:
        assert np.array_equal(m.state_dict()[k].numpy(), sd[k]) and torch.equal(m.state_dict()[k], m2.state_dict()[k]), k
    for k in ("gru_net.weight_hh_l0", "gru_cell_attention.weight_hh"):        # read as float4 by the kernels
        assert m.params[k].data_ptr() % 16 == 0


def test_unequal_item_and_cat_sizes_are_refused():
    from paddlerec_amd.dien import DIENLayer
    with pytest.raises(ValueError, match="item_emb_size"):
        DIENLayer(4, 8, "sigmoid", False, False, 31, 29, device="cpu", kernels=dien_cpu_kernels)


def test_learning_rate_is_the_piecewise_decay():
    from paddlerec_amd.dien import DIENLayer
    assert DIENLayer.learning_rate(0, 0.85) == 0.85 and DIENLayer.learning_rate(409999, 0.85) == 0.85
    assert DIENLayer.learning_rate(410000, 0.85) == 0.2


# ------------------------------------------------------------------------------------------------ reader
def _batches(item_count, batch_size=4):
    from paddlerec_amd.reader import DienReader
    return list(DienReader([os.path.join(GOLDEN, "dien_sample.txt")], batch_size, "cpu", item_count=item_count))


@pytest.mark.parametrize("tag,item_count", [("a", 63001), ("f", 30000)])
def test_reader_reproduces_the_reference_readers_first_batches(tag, item_count):
    g = np.load(os.path.join(GOLDEN, "dien_reader.npz"))
    bs = _batches(item_count)
    assert 4 * len(bs) == int(g[tag + "_count"][0])
    for b in range(3):
        for j, name in enumerate(FEEDS):
            got, want = bs[b][j].numpy(), g["%s%d_%s" % (tag, b, name)]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (b, name)
    assert bs[0][5].dtype == torch.float32 and bs[0][5].shape[2] == 1


def test_reader_skips_short_batches_and_filters_by_count():
    lines = [ln for ln in open(os.path.join(GOLDEN, "dien_sample.txt")) if len(ln.strip().split(";")) == 5]
    lens = sorted(len(ln.split(";")[0].split()) for ln in lines)
    n = len(lines) - len(lines) % 4
    skipped = sum(1 for i in range(0, n, 4) if max(lens[i:i + 4]) < 2)
    assert skipped >= 1                                         # the fixture holds whole batches of length-1 histories
    bs = _batches(63001)
    assert len(bs) == n // 4 - skipped and all(b[0].shape[1] >= 2 for b in bs)
    kept = [ln for ln in lines if max(int(x) for x in ln.split(";")[0].split()) <= 30000]
    assert 0 < len(kept) < len(lines)
    assert sum(b[0].shape[0] for b in _batches(30000)) <= len(kept)
    assert all(int(b[0].max()) <= 30000 for b in _batches(30000))


# ------------------------------------------------------------------------------------------------ argument checks
def test_dien_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    L, p = engine_lib, C.c_void_p(4096)                         # never dereferenced: every call is refused first
    assert L.rec_gru_seq_fwd(4, 3, 10, p, p, p, p, None, None) == -2 and b"multiple of 4" in L.rec_last_error()
    assert L.rec_gru_seq_fwd(4, 3, 260, p, p, p, p, None, None) == -2
    assert L.rec_gru_seq_fwd(4, 0, 8, p, p, p, p, None, None) == -1
    assert L.rec_gru_seq_fwd(4, 3, 8, p, None, p, p, None, None) == -1
    assert L.rec_gru_seq_fwd(4, 3, 8, p, C.c_void_p(4100), p, p, None, None) == -1 and b"aligned" in L.rec_last_error()
    assert L.rec_gru_seq_fwd(0, 3, 8, None, None, None, None, None, None) == 0
    assert L.rec_gru_seq_bwd(4, 3, 8, p, p, None, None, p, p, None) == -1          # dGi is dGh
    assert L.rec_gru_seq_bwd(4, 3, 12, None, p, None, None, p, C.c_void_p(8192), None) == -1
    n = C.c_size_t(0)
    assert L.rec_dien_aux_workspace_bytes(5, 6, C.byref(n)) == 0 and n.value == 5 * 6 * 4
    assert L.rec_dien_aux_workspace_bytes(5, 0, C.byref(n)) == -1
    aux = lambda Ei, si, ws_bytes: L.rec_dien_aux_fwd(5, 6, Ei, 4, p, p, p, p, p, si, 31, p, 4, 29, 0, p, p, p,
                                                      C.c_size_t(ws_bytes), None)
    assert aux(4, 3, 1 << 20) == -1 and aux(0, 4, 1 << 20) == -1
    assert aux(4, 4, 8) == -3                                   # workspace too small
    assert L.rec_dien_aux_bwd(5, 6, 4, 4, p, p, p, p, p, 4, 31, p, 4, 29, 0, 1.0, p, p, 1, p, p, None) == -1   # aliases
    assert L.rec_dien_att_feat_fwd(3, 0, p, p, p, None) == -1 and L.rec_dien_att_feat_fwd(0, 8, None, None, None, None) == 0
    assert L.rec_dien_att_feat_bwd(3, 8, p, p, p, p, 1, p, None) == -1
    assert L.rec_dien_attention_seq_fwd(2, 0, 8, p, p, p, 1.0, p, p, None) == -1
    assert L.rec_dien_attention_seq_bwd(2, 3, 8, p, p, p, 1.0, p, p, 0, None) == -1  # d_hist is dx_att
