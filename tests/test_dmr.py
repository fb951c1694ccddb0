"""DMR without a GPU: the float64 restatement (tests/dmr_ref.py) against the golden recorded from the reference's own
net.py (tools/make_golden_dmr.py), DMRLayer's host logic on a CPU stand-in backend (tests/dmr_cpu_kernels.py), the reader
against the reference reader's record, and the argument checks of the new entry points.

Bounds.  The golden is a float32 torch run.  Per array, err = max|a - b| / max|b|, and the bound is the rule of
test_dien_gpu.py: max(8 x the error of dmr_ref run in float32 against dmr_ref in float64, 1e-6) — the restatement's own
float32 rounding is the yardstick of what a float32 evaluation of this net can agree on.  Both errors are printed.
Parameters after the Adam step go through helpers.assert_adam_weights_close with its own frac: the first Adam step is
sign-like where a gradient is near eps, and the golden's seed was chosen (and checked by the tool) so that dmr_ref in
float32 alone passes it.

One parameter is outside that statement, for a reason of the net's and not of the seed: att_layer3_layer.bias.  Adding a
constant to every u2i score leaves every softmax row unchanged (a padded entry has weight exactly 0, a row without a valid
entry is uniform and gated out), so its gradient is ZERO in exact arithmetic and rounding noise in float32 (about 1e-9
here).  The gradient is therefore asserted to be noise on both sides (at most B * T roundings of the largest score
gradient), and the moved distance only to be within what one Adam step can move — Adam divides the noise by its own
size, and no two float32 evaluations agree on the result."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmr_cpu_kernels
import dmr_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close

NOISE_GRAD = "att_layer3_layer.bias"


@pytest.fixture(scope="module")
def gold():
    g = R.load_golden(GOLDEN)
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    lr = float(g["lr"][0])
    c64, g64, n64, _ = R.train_step(p, g["sparse"], g["price"], lr)
    c32, g32, n32, _ = R.train_step(p, g["sparse"], g["price"], lr, dtype=np.float32)
    return dict(g=g, p=p, lr=lr, c64=c64, g64=g64, n64=n64, c32=c32, g32=g32, n32=n32)


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def _check_adam(got, gold, key, lr):
    """The Adam-weights statement of the module docstring for one key."""
    if key == NOISE_GRAD:
        assert np.abs(np.asarray(got, np.float64) - gold["g"]["n_" + key]).max() <= 2.0 * lr * 3.17
        return
    assert_adam_weights_close(got, gold["g"]["n_" + key], lr, 1, err_msg=key)


def test_golden_holds_the_cases_it_is_meant_to(gold):
    g = gold["g"]
    T, E, O, B = (int(x) for x in g["sizes"][:4])
    assert (T, E, O, B) == (50, 4, 2, 6)
    f = R.split_feeds(g["sparse"], T)
    valid = (f["mask"] == 1).sum(1)
    assert sorted(valid.tolist()) == [0, 1, 2, 28, 34, 50]
    assert f["mask"][1, T - 1] == 1 and f["mask"][1, T - 2] == 0              # row T-2 of sample 1 has no valid entry
    hole = f["mask"][4]
    assert hole[5] == 1 and hole[25] == 0 and hole[40] == 1
    assert set(f["match_mask"][:, T - 2].tolist()) == {0, 1} and f["match_mask"][1, T - 2] == 1
    assert len(np.unique(f["cate_his"][0])) < T and (f["cate_his"] == f["cate_id"][0]).any()     # duplicates
    assert f["cate_id"][3] == f["cate_id"][0] and f["cate_his"][1, -1] == f["cate_his"][4, -1]
    for k in g:
        if k.startswith("p_") and (k.endswith(".bias") or k.endswith("._weight")):
            if not k.startswith("p_logits_layer"):
                assert np.abs(g[k]).min() > 0 and not np.allclose(g[k], 0.1), k        # no default left
    assert not np.allclose(g["p_inp_layer._mean"], 0) and not np.allclose(g["p_inp_layer._variance"], 1)
    assert sorted(k[2:] for k in g if k.startswith("p_")) == sorted(R.param_keys())
    assert not g["g_logits_layer.weight"].any() and (g["n_logits_layer.weight"] == g["p_logits_layer.weight"]).all()
    assert float(g["price"].min()) > 0 and g["price"].dtype == np.float32


def test_float64_reference_matches_every_array_of_the_golden(gold):
    g, c64, c32 = gold["g"], gold["c64"], gold["c32"]
    for k in ("y_hat", "aux", "ctr", "loss"):
        e, b = R.relerr(c64[k], g[k]), bound_of(c32[k], c64[k])
        print("%-44s err %.3g  float32-ref err %.3g" % (k, e, b / 8))
        assert e <= b, (k, e, b)
    for k in gold["p"]:
        e, b = R.relerr(gold["g64"][k], g["g_" + k]), bound_of(gold["g32"][k], gold["g64"][k])
        print("%-44s err %.3g  float32-ref err %.3g" % ("g_" + k, e, b / 8))
        assert e <= b, (k, e, b)
    for k in ("inp_layer._mean", "inp_layer._variance"):
        e, b = R.relerr(gold["n64"][k], g["n_" + k]), bound_of(gold["n32"][k], gold["n64"][k])
        assert e <= b, (k, e, b)
    # the structurally zero gradient: it is the sum of the B * T score gradients, so float32 noise is at most
    # B * T roundings (2^-23 each) of the largest of them — on both sides; float64 sits 2^29 below that
    noise = gold["c64"]["ds1"].size * 2.0 ** -23 * np.abs(gold["c64"]["ds1"]).max()
    print("%s: golden %.3g, float32 ref %.3g, float64 ref %.3g, noise bound %.3g" % (
        NOISE_GRAD, g["g_" + NOISE_GRAD][0], gold["g32"][NOISE_GRAD][0], gold["g64"][NOISE_GRAD][0], noise))
    assert np.abs(g["g_" + NOISE_GRAD]).max() <= noise and np.abs(gold["g32"][NOISE_GRAD]).max() <= noise
    assert np.abs(gold["g64"][NOISE_GRAD]).max() <= noise * 2.0 ** -29


def test_parameters_after_adam(gold):
    for k in gold["p"]:
        if k in R.NO_GRAD:
            continue
        _check_adam(gold["n32"][k], gold, k, gold["lr"])                       # float32 alone passes: the seed's property
        _check_adam(gold["n64"][k], gold, k, gold["lr"])
    assert (gold["n64"]["logits_layer.weight"] == gold["p"]["logits_layer.weight"]).all()


def _layer(gold, **kw):
    from paddlerec_amd.dmr import DMRLayer
    g = gold["g"]
    sizes = [int(x) for x in g["sizes"][4:]]
    m = DMRLayer(*sizes, 4, 2, device="cpu", kernels=dmr_cpu_kernels, **kw)
    m.set_dict(gold["p"])
    return m


def test_layer_train_step_matches_the_golden_on_the_stand_in(gold):
    g, lr = gold["g"], gold["lr"]
    m = _layer(gold)
    feeds = [torch.as_tensor(g["sparse"]), torch.as_tensor(g["price"])]
    unused = m.params["logits_layer.weight"].clone()
    loss, y_hat, aux, ctr = m.train_step(feeds, lr=lr)
    for k, got in (("y_hat", y_hat), ("aux", aux), ("ctr", ctr), ("loss", loss)):
        e, b = R.relerr(got.numpy(), gold["c64"][k]), bound_of(gold["c32"][k], gold["c64"][k])
        assert e <= b, (k, e, b)
    grads = m.last_gradients()
    for k in gold["p"]:
        if k in R.NO_GRAD:
            assert k not in grads
            continue
        e, b = R.relerr(grads[k].numpy(), gold["g64"][k]), bound_of(gold["g32"][k], gold["g64"][k])
        assert e <= b, (k, e, b)
    sd = m.state_dict()
    assert sorted(sd) == sorted(R.param_keys())
    for k in gold["p"]:
        if k in R.NO_GRAD:
            continue
        _check_adam(sd[k].numpy(), gold, k, lr)
    for k in ("inp_layer._mean", "inp_layer._variance"):
        assert R.relerr(sd[k].numpy(), g["n_" + k]) <= 1e-6, k
    assert torch.equal(sd["logits_layer.weight"], unused) and "logits_layer.bias" in sd       # declared, never stepped
    assert "dm_item_biases" not in sd and int(m.status.item()) == 0


def test_two_row_shortcut_equals_the_full_tile(gold):
    """The layer pools rows T-2 and T-1 only; the restatement builds all T rows.  Same vectors, same score gradient."""
    c = gold["c64"]
    T = c["T"]
    out, w, _ = R.prefix_pool_fwd(c["s1"], c["f"]["mask"], c["hist"], (T - 2, T - 1))
    assert R.relerr(out, c["pooled"][:, T - 2:]) < 1e-14 and R.relerr(w, c["W1"][:, T - 2:]) < 1e-14
    assert np.array_equal(w[1, 0], np.full(T, 1.0 / T))                        # sample 1, row T-2: uniform over ALL T
    assert np.array_equal(w[3], np.full((2, T), 1.0 / T))                      # the fully masked sample
    # gradient: rows T-2, T-1 of d pooled are the only non-zero ones in the full backward
    P = c["P"]
    dd1p = np.zeros_like(c["d1p"])
    rng = np.random.default_rng(3)
    dd1p[:, T - 2:] = rng.standard_normal(dd1p[:, T - 2:].shape)
    dpool = dd1p @ P["dnn_layer1_layer.weight"].T
    W1, hist = c["W1"], c["hist"]
    dW1 = dpool @ np.swapaxes(hist, 1, 2)
    dM = W1 * (dW1 - (W1 * dW1).sum(-1, keepdims=True))
    full_ds = np.where(c["valid"], np.where(np.tril(np.ones((T, T), bool))[None], dM, 0).sum(1), 0)
    full_dh = np.swapaxes(W1, 1, 2) @ dpool
    ds, dh = R.prefix_pool_bwd(c["f"]["mask"], hist, (T - 2, T - 1), w, dpool[:, T - 2:])
    assert R.relerr(ds, full_ds) < 1e-13 and R.relerr(dh, full_dh) < 1e-13
    assert not ds[1, :T - 1].any() and not ds[3].any()                         # padded entries: no gradient


def test_infer_uses_running_statistics_and_skips_the_aux_branch(gold):
    g = gold["g"]
    m = _layer(gold)
    m.eval()
    feeds = [torch.as_tensor(g["sparse"]), torch.as_tensor(g["price"])]
    y_hat, one = m(feeds, 1)
    c = R.forward(gold["p"], g["sparse"], g["price"], train=False)
    assert R.relerr(y_hat.numpy(), c["y_hat"]) < 1e-5 and float(one) == 1.0 and "aux" not in c
    assert torch.equal(m.params["inp_layer._mean"], torch.as_tensor(g["p_inp_layer._mean"]))


def test_state_dict_round_trip_and_checkpoint(gold, tmp_path):
    from paddlerec_amd import checkpoint
    m, m2 = _layer(gold), _layer(gold)
    feeds = [torch.as_tensor(gold["g"]["sparse"]), torch.as_tensor(gold["g"]["price"])]
    m.train_step(feeds, lr=gold["lr"])
    sd = {k: v.numpy().copy() for k, v in m.state_dict().items()}
    m2.set_dict(sd)
    for k in sd:
        assert np.array_equal(m2.state_dict()[k].numpy(), sd[k]), k
    d = checkpoint.save_model(m, None, str(tmp_path), 0)
    m3 = _layer(gold)
    checkpoint.load_model(d, m3)
    assert m3.step_count == 1
    for k in sd:
        assert np.array_equal(m3.state_dict()[k].numpy(), sd[k]), k
    assert torch.equal(m3._dense_m, m._dense_m) and torch.equal(m3._tv["cat_embeddings_var"], m._tv["cat_embeddings_var"])
    assert m._dense_m.abs().max() > 0
    l1 = m.train_step(feeds, lr=gold["lr"])[0]
    l3 = m3.train_step(feeds, lr=gold["lr"])[0]
    assert torch.equal(l1, l3)


def test_constructor_refuses_what_the_kernels_cannot_take():
    from paddlerec_amd.dmr import DMRLayer
    sizes = [5] * 16
    with pytest.raises(ValueError, match="main_embedding_size"):
        DMRLayer(*sizes, 6, 2, device="cpu", kernels=dmr_cpu_kernels)
    with pytest.raises(ValueError, match="history_length"):
        DMRLayer(*sizes, 4, 2, history_length=1, device="cpu", kernels=dmr_cpu_kernels)
    m = DMRLayer(*sizes, 32, 8, device="cpu", kernels=dmr_cpu_kernels)
    assert m.inp_length == 459                                               # net.py:373-377 at the config's sizes


# ------------------------------------------------------------------------------------------------ reader
def test_reader_reproduces_the_reference_readers_rows():
    from paddlerec_amd.reader import AlimamaReader
    want = np.load(os.path.join(GOLDEN, "dmr_reader.npz"))["rows"]
    bs = list(AlimamaReader([os.path.join(GOLDEN, "dmr_sample.txt")], 16, "cpu"))
    assert len(bs) == len(want) // 16 == 2                                    # drop_last
    for i, (sparse, price) in enumerate(bs):
        w = want[16 * i:16 * i + 16]
        assert sparse.dtype == torch.int64 and tuple(sparse.shape) == (16, 267)
        assert price.dtype == torch.float32 and tuple(price.shape) == (16, 1)
        assert np.array_equal(sparse.numpy(), w.astype(np.int64)) and np.array_equal(price.numpy()[:, 0], w[:, 264])
    valid = (bs[0][0][:, 150:200] == 1).sum(1).tolist()
    assert {1, 2, 28, 48} <= set(valid)


def test_reader_reads_empty_and_null_as_zero_and_refuses_short_lines(tmp_path):
    from paddlerec_amd.reader import AlimamaReader
    row = ["7"] * 267
    row[3], row[4], row[5], row[264] = "", "NULL", "null", "12.5"
    p = tmp_path / "a.txt"
    p.write_text(",".join(row) + "\n\n" + ",".join(row) + "\n")
    (sparse, price), = list(AlimamaReader([str(p)], 2, "cpu"))
    assert sparse[0, 3] == 0 and sparse[0, 4] == 0 and sparse[0, 5] == 0 and sparse[0, 6] == 7
    assert sparse[0, 264] == 12 and float(price[0, 0]) == 12.5
    p.write_text(",".join(row[:-1]) + "\n")
    with pytest.raises(ValueError, match="266 fields"):
        list(AlimamaReader([str(p)], 1, "cpu"))


def test_trainer_knows_the_model():
    from paddlerec_amd import trainer
    assert "dmr" in trainer.MODELS and trainer.guess_model("/x/models/rank/dmr/config.yaml") == "dmr"
    assert type(trainer._dygraph_model("dmr")).__module__ == "paddlerec_amd.dmr"


# ------------------------------------------------------------------------------------------------ argument checks
def test_dmr_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    L, p = engine_lib, C.c_void_p(4096)                         # never dereferenced: every call is refused first
    rows = (C.c_int32 * 2)(48, 49)
    pool = lambda T, R, r: L.rec_dmr_prefix_pool_fwd(4, T, 8, p, p, T, p, 8, R, r, p, 16, None, 0, p, None)
    assert pool(49, 2, rows) == -1 and b"outside" in L.rec_last_error()
    assert pool(50, 0, rows) == -1 and pool(50, 9, rows) == -1 and pool(50, 2, None) == -1
    assert L.rec_dmr_prefix_pool_fwd(4, 50, 8, p, p, 49, p, 8, 2, rows, p, 16, None, 0, p, None) == -1     # ld_mask < T
    assert L.rec_dmr_prefix_pool_fwd(0, 50, 8, None, None, 50, None, 8, 2, rows, None, 16, None, 0, None, None) == 0
    bwd = lambda T, dh: L.rec_dmr_prefix_pool_bwd(4, T, 8, p, T, p, 8, 1, (C.c_int32 * 1)(0), p, C.c_void_p(8192), 8, None,
                                                  0, C.c_void_p(12288), dh, 8, 0, None)
    assert bwd(5000, C.c_void_p(16384)) == -2 and bwd(50, p) == -1          # steps > 4096; d_hist is hist
    a = C.c_void_p(4096)
    assert L.rec_prelu_fwd(4, 8, p, 8, a, 7, 0, 0, 0, p, 8, None) == -1 and b"num_alpha" in L.rec_last_error()
    assert L.rec_prelu_fwd(4, 8, p, 8, a, 50, 1, 2, 49, p, 8, None) == -1   # base + period > num_alpha
    assert L.rec_prelu_fwd(4, 8, p, 7, a, 8, 0, 0, 0, p, 8, None) == -1     # ldx < n
    assert L.rec_prelu_fwd(0, 8, None, 8, None, 8, 0, 0, 0, None, 8, None) == 0
    n = C.c_size_t(0)
    assert L.rec_prelu_workspace_bytes(100, 8, 0, 0, C.byref(n)) == 0 and n.value == 7 * 8 * 4
    assert L.rec_prelu_workspace_bytes(100, 8, 1, 50, C.byref(n)) == 0 and n.value == 1 * 400 * 4
    assert L.rec_prelu_bwd(4, 8, p, 8, p, 8, a, 8, 0, 0, 0, C.c_void_p(8192), 8, a, p, C.c_size_t(4), None) == -3
    assert L.rec_prelu_bwd(4, 8, p, 8, p, 8, a, 8, 0, 0, 0, p, 8, a, p, C.c_size_t(1 << 20), None) == -1   # dX is X
    fb, bb = C.c_size_t(0), C.c_size_t(0)
    assert L.rec_dmr_match_loss_workspace_bytes(100, 12978, 32, C.byref(fb), C.byref(bb)) == 0
    assert fb.value == 100 * 130 * 4 and bb.value == 16 * 12978 * 32 * 4    # fixed chunk counts: nothing of size B x C
    big = C.c_size_t(1 << 30)
    ml = lambda k, ldu, U: L.rec_dmr_match_loss_fwd(8, 37, k, U, ldu, p, k, None, p, 1, p, p, p, p, big, None)
    assert ml(6, 6, p) == -2 and b"multiple of 4" in L.rec_last_error()
    assert ml(68, 68, p) == -2 and ml(8, 6, p) == -1 and ml(8, 8, C.c_void_p(4100)) == -1
    assert L.rec_dmr_match_loss_fwd(8, 37, 8, p, 8, p, 8, None, p, 1, p, p, p, p, C.c_size_t(16), None) == -3
    assert L.rec_dmr_match_loss_bwd(8, 37, 8, p, 8, p, 8, None, p, 1, p, 0.1, C.c_void_p(8192), 8, p, 8, 0, p, big,
                                    None) == -1                              # dV is V
    assert L.rec_dmr_tail_fwd(4, 50, 7, p, 7, p, 7, p, p, 1, p, 4, 37, p, p, 7, p, 7, p, 1, p, p, None) == -1   # odd dim
    assert L.rec_dmr_tail_fwd(0, 50, 8, None, 8, None, 8, None, None, 1, None, 4, 37, None, None, 8, None, 8, None, 1,
                              None, None, None) == 0
    assert L.rec_dmr_tail_bwd_match(4, 4, None, None, 1, p, p, 1, p, 4, 37, p, p, p, 4, None) == -1
    assert L.rec_dmr_tail_bwd_hist(4, 50, 8, None, None, p, 8, p, 8, p, 8, p, 8, p, 8, p, 7, p, 8, p, 8, None) == -1
