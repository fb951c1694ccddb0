"""BST without a GPU: tests/bst_ref.py (float64) against the two goldens recorded from the reference's net.py, the layer on
the CPU operator backend against both, the wrong-key quirk, checkpoints, the reader and the trainer.

Tolerance, the project's rule: err = max|got - ref64| / max|ref64| per tensor; the bound is 8 x the same error of bst_ref.py
evaluated in float32 on the same inputs, floor 1e-6.

Parameters after Adagrad.  One step from accumulator 0 moves a weight by lr g / (|g| + eps): the full lr for every |g| >>
eps = 1e-6, whatever the size of g, and sign-like where |g| is near eps.  A relative error on the parameter tensor would
therefore say nothing.  The step's sensitivity to the gradient is lr eps / (|g| + eps)^2 (bst_ref.step_bound has the form for a non-zero accumulator), so each ELEMENT is bound by that
sensitivity times the absolute gradient bound of its tensor (the rule above times max|g64|), capped at lr (the step cannot be
larger), plus 4 float32 roundings of the parameter itself (it is stored in float32; at |g| >> eps the sensitivity term is far
below one rounding).  bst.k_liner.bias (bst_ref.STRUCTURAL_ZERO) has a gradient that is zero in exact arithmetic — a constant
added to every key shifts each score row by a constant and softmax is shift invariant — and rounding noise in float32, which
Adagrad turns into a step of up to lr in either direction: no two float32 evaluations agree on it.  It is held to a noise bound
on the gradient, 32 float32 epsilons times the scale of the terms that cancel (bst_ref.kbias_noise_scale: sum P (|dP| + |D|) |q|
— 32 covers the exp, the two dot products of at most 64 terms and the sums over i and j), and to the lr cap on the parameter.
In the "n" variant nothing else is of this kind elementwise: the rows that feed q_liner / k_liner / v_liner are layer-norm
outputs and sum to zero, so the sums over the input axis of those three weight gradients vanish — a linear combination of
elements, not an element — and every element is held to the ordinary bound."""
import os

import numpy as np
import pytest
import torch

import bst_cpu_kernels
import bst_ref as R
from conftest import GOLDEN

F32_EPS = float(np.finfo(np.float32).eps)
FIXTURES = ("bst_da.npz", "bst_n.npz")


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def param_bounds(res64, res32, p, lr=R.LR, acc=None):
    """{name: elementwise bound on the parameter after one step} from two bst_ref.train_step results (acc: the accumulators
    the step started from, None = 0)."""
    out = {}
    for k in p:
        g64 = res64[2][k].reshape(np.shape(p[k]))
        gb = bound_of(res32[2][k], res64[2][k]) * np.abs(g64).max()
        a = 0.0 if acc is None else np.asarray(acc[k], np.float64).reshape(g64.shape)
        out[k] = R.step_bound(g64, a, res64[3][k], gb, lr)
    return out


@pytest.fixture(scope="module", params=FIXTURES)
def gold(request):
    g, p, feeds, cfg = R.load_golden(os.path.join(GOLDEN, request.param))
    r64 = R.train_step(p, None, feeds, cfg, None, R.LR)
    r32 = R.train_step(p, None, feeds, cfg, None, R.LR, dtype=np.float32)
    c64 = R.forward_backward(p, feeds, cfg)[3]
    B, T = feeds["hist_item"].shape
    noise = 32 * F32_EPS * R.kbias_noise_scale(c64, B, T + 1, cfg["n_head"])
    return dict(name=request.param, g=g, p=p, feeds=feeds, cfg=cfg, r64=r64, r32=r32, pb=param_bounds(r64, r32, p), noise=noise)


def _check_params(got, gold, what):
    for k in gold["p"]:
        diff = np.abs(np.asarray(got[k], np.float64).reshape(gold["p"][k].shape) - gold["r64"][3][k])
        if k in R.STRUCTURAL_ZERO:
            assert diff.max() <= R.LR * (1 + 1e-3), (what, k, diff.max())
            continue
        over = diff - gold["pb"][k]
        assert (over <= 0).all(), (what, k, float(over.max()), float(diff.max()))


def _check_grads(got, gold, what):
    for k in gold["p"]:
        a = np.asarray(got[k], np.float64).reshape(gold["p"][k].shape)
        if k in R.STRUCTURAL_ZERO:
            print("%-40s |g| %.3g  noise bound %.3g" % (k, np.abs(a).max(), gold["noise"]))
            assert np.abs(a).max() <= gold["noise"], (what, k)
            continue
        e, b = R.relerr(a, gold["r64"][2][k]), bound_of(gold["r32"][2][k], gold["r64"][2][k])
        print("%-40s err %.3g  float32-ref err %.3g" % ("g_" + k, e, b / 8))
        assert e <= b, (what, k, e, b)


def test_golden_holds_the_cases_it_is_meant_to(gold):
    g, f = gold["g"], gold["feeds"]
    assert (str(g["pre"]), str(g["post"])) == (("da", "da") if gold["name"] == "bst_da.npz" else ("n", "da"))
    assert f["hist_item"].shape == (5, 7) and [int(x) for x in g["heads"]] == [3, 4, 4]
    assert not f["hist_item"][3].any() and not f["hist_cat"][3].any() and not f["hist_position"][3].any()
    assert len(np.unique(f["hist_item"][0])) < 6 and f["hist_item"][2, 1] == f["hist_item"][0, 0]
    assert f["target_item"][1, 0] == f["hist_item"][0, 0] and f["target_item"][4, 0] == f["target_item"][1, 0]
    for k in gold["p"]:
        if k.endswith("bias"):
            assert np.abs(gold["p"][k]).min() > 0, k
    names = ["bst.%s.weight" % t for t in R.TABLES] + ["bias"]
    for n in ("q_liner", "k_liner", "v_liner", "po_liner", "hid_l", "hid2_l", "dnn_linear_0", "dnn_linear_1", "dnn_linear_2"):
        names += ["bst.%s.weight" % n, "bst.%s.bias" % n]
    assert sorted(gold["p"]) == sorted(names)
    assert g["p_bst.hist_item_emb_attr.weight"].shape == g["p_bst.target_item_emb_attr.weight"].shape == (40, 4)
    # id 0 is a live, trained row: the padded positions of the all-zero history move it
    assert np.abs(g["g_bst.hist_item_emb_attr.weight"][0]).max() > 0
    assert (g["n_bst.hist_item_emb_attr.weight"][0] != g["p_bst.hist_item_emb_attr.weight"][0]).all()


def test_float64_reference_matches_every_array_of_the_golden(gold):
    g, (pred64, loss64, g64, _, _), (pred32, loss32, g32, _, _) = gold["g"], gold["r64"], gold["r32"]
    for k, a64, a32 in (("pred", pred64, pred32), ("loss", loss64, loss32)):
        e, b = R.relerr(a64, g[k]), bound_of(a32, a64)
        print("%-40s err %.3g  float32-ref err %.3g" % (k, e, b / 8))
        assert e <= b, (k, e, b)
    _check_grads({k: g["g_" + k] for k in gold["p"]}, gold, "golden")
    assert np.abs(g64[R.STRUCTURAL_ZERO[0]]).max() <= gold["noise"] * 2.0 ** -29       # float64 sits 2^29 below


def test_parameters_after_adagrad(gold):
    _check_params({k: gold["g"]["n_" + k] for k in gold["p"]}, gold, "golden")
    _check_params(gold["r32"][3], gold, "float32 restatement")                        # the seed's property
    k = "bst.dnn_linear_0.weight"
    moved = np.abs(gold["g"]["n_" + k] - gold["p"][k])
    assert moved.max() <= R.LR * (1 + 1e-3) and np.median(moved) > 0.9 * R.LR            # sign-like steps of lr


def _layer(gold, **kw):
    from paddlerec_amd.bst import BSTLayer
    p, cfg = gold["p"], gold["cfg"]
    tab = lambda n: p["bst.%s.weight" % n].shape
    fc = [p["bst.dnn_linear_%d.weight" % i].shape[1] for i in range(R.num_dnn(p) - 1)]
    args = dict(dropout_rate=0.0, prepostprocess_dropout=0.0)
    args.update(kw)
    m = BSTLayer(tab("userid_attr")[0], tab("hist_item_emb_attr")[1], tab("hist_cat_emb_attr")[1],
                 tab("hist_position_emb_attr")[1], "relu", True, True, tab("hist_item_emb_attr")[0], tab("hist_cat_emb_attr")[0],
                 tab("hist_position_emb_attr")[0], 1, tab("userid_attr")[1], cfg["d_key"], cfg["d_value"], cfg["n_head"],
                 args["dropout_rate"], cfg["post"], cfg["pre"], args["prepostprocess_dropout"], p["bst.hid_l.weight"].shape[1],
                 0.0, fc, device="cpu", kernels=bst_cpu_kernels)
    m.set_dict(p)
    return m


def _feeds(gold):
    f = gold["feeds"]
    return [torch.as_tensor(f[k]) for k in ("userid", "hist_item", "hist_cat", "hist_position", "target_item", "target_cat",
                                            "target_position")], torch.as_tensor(f["label"])


def test_layer_train_step_matches_the_golden_on_the_stand_in(gold):
    m = _layer(gold)
    feeds, label = _feeds(gold)
    assert sorted(m.state_dict()) == sorted(gold["p"])
    loss, pred = m.train_step(feeds, label)
    for k, got, i in (("pred", pred, 0), ("loss", loss, 1)):
        e, b = R.relerr(got.numpy(), gold["r64"][i]), bound_of(gold["r32"][i], gold["r64"][i])
        assert e <= b and R.relerr(got.numpy(), gold["g"][k]) <= 2 * b, (k, e, b)
    _check_grads({k: v.numpy() for k, v in m.last_gradients().items()}, gold, "layer")
    _check_params({k: v.numpy() for k, v in m.state_dict().items()}, gold, "layer")
    assert int(m.status.item()) == 0


def test_eval_forward_and_dropout_masks_on_the_stand_in(gold):
    feeds, label = _feeds(gold)
    m = _layer(gold, dropout_rate=0.2, prepostprocess_dropout=0.2)
    m.eval()
    pred = m(*feeds)
    assert R.relerr(pred.numpy(), gold["r64"][0]) <= bound_of(gold["r32"][0], gold["r64"][0])       # eval: no dropout
    m.train()
    streams = m.dropout_streams(1)
    B, T = gold["feeds"]["hist_item"].shape
    L, H = T + 1, gold["cfg"]["n_head"]
    assert sorted(streams) == sorted(R.dropout_sites(gold["cfg"]) + ["att", "ffn"])
    assert len(set(streams.values())) == len(streams) and not set(streams.values()) & set(m.dropout_streams(2).values())
    from oracle.dcn_v2_ref import dropout_keep
    masks = {s: dropout_keep((B * H * L, L) if s == "att" else (B * L, m.d_model), 0.2, m.dropout_seed, st) / 0.8
             for s, st in streams.items()}
    pred64, loss64, g64, _ = R.forward_backward(gold["p"], gold["feeds"], gold["cfg"], masks)
    pred32, loss32, g32, _ = R.forward_backward(gold["p"], gold["feeds"], gold["cfg"], masks, dtype=np.float32)
    loss, pred = m.train_step(feeds, label)
    assert R.relerr(pred.numpy(), pred64) <= bound_of(pred32, pred64) and R.relerr(loss.numpy(), loss64) <= bound_of(loss32, loss64)
    assert R.relerr(pred64, gold["r64"][0]) > 1e-4                                                  # the masks did something
    got = m.last_gradients()
    for k in gold["p"]:
        if k not in R.STRUCTURAL_ZERO:
            e, b = R.relerr(got[k].numpy(), g64[k]), bound_of(g32[k], g64[k])
            assert e <= b, (k, e, b)


def test_create_model_reads_preprocess_cmd_from_the_wrong_key():
    from paddlerec_amd.bst import QUIRKS, DygraphModel
    cfg = {"hyper_parameters.item_emb_size": 4, "hyper_parameters.cat_emb_size": 4, "hyper_parameters.position_emb_size": 4,
           "hyper_parameters.item_count": 9, "hyper_parameters.user_count": 7, "hyper_parameters.cat_count": 5,
           "hyper_parameters.position_count": 5, "hyper_parameters.d_model": 12, "hyper_parameters.d_key": 4,
           "hyper_parameters.d_value": 4, "hyper_parameters.n_head": 3, "hyper_parameters.dropout_rate": 0.2,
           "hyper_parameters.postprocess_cmd": "da", "hyper_parameters.preprocess_cmd": "n",
           "hyper_parameters.prepostprocess_dropout": 0.2, "hyper_parameters.d_inner_hid": 8, "hyper_parameters.fc_sizes": [8]}
    m = DygraphModel().create_model(cfg, device="cpu", kernels=bst_cpu_kernels)
    assert (m.preprocess_cmd, m.postprocess_cmd) == ("da", "da")                # the shipped YAMLs: no layer norm at all
    assert m.num_pp_sites == 4 and m.streams_per_step == 6
    del cfg["hyper_parameters.postprocess_cmd"]
    m = DygraphModel().create_model(cfg, device="cpu", kernels=bst_cpu_kernels)
    assert (m.preprocess_cmd, m.postprocess_cmd) == ("n", "da")                 # the default applies when the key is absent
    assert "postprocess_cmd" in QUIRKS and "k_liner.bias" in QUIRKS


def test_constructor_refuses_what_the_kernels_cannot_take():
    from paddlerec_amd.bst import BSTLayer
    mk = lambda dm, dk, dv, H, w=4: BSTLayer(7, w, 4, 4, "relu", True, True, 9, 5, 5, 1, dm, dk, dv, H, 0.0, "da", "da", 0.0, 8, 0.0,
                                             [8], device="cpu", kernels=bst_cpu_kernels)
    with pytest.raises(ValueError, match="d_model"):
        mk(16, 4, 4, 4)
    with pytest.raises(ValueError, match="n_head"):
        mk(12, 4, 4, 2)
    with pytest.raises(ValueError, match="multiples of 4"):
        mk(12, 6, 4, 3)
    with pytest.raises(ValueError, match="multiples of 4"):
        mk(144, 4, 72, 2, w=136)


def test_state_dict_round_trip_and_checkpoint(gold, tmp_path):
    from paddlerec_amd import checkpoint
    m, m2 = _layer(gold), _layer(gold)
    feeds, label = _feeds(gold)
    m.train_step(feeds, label)
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
    for k in ("bst.k_liner.weight", "bst.hist_cat_emb_attr.weight", "bias"):       # the accumulators, per parameter
        assert torch.equal(m3._acc[k], m._acc[k]) and m._acc[k].abs().max() > 0, k
    assert torch.equal(m.train_step(feeds, label)[0], m3.train_step(feeds, label)[0])


# ------------------------------------------------------------------------------------------------ reader, trainer
def test_reader_reproduces_the_reference_readers_rows():
    from paddlerec_amd.reader import AmazonBSTReader
    want = np.load(os.path.join(GOLDEN, "bst_reader.npz"))
    rd = AmazonBSTReader([os.path.join(GOLDEN, "bst_sample.txt")], 4, "cpu")
    bs = list(rd)
    n, T = want["hist_item"].shape
    assert len(bs) == n // 4 == 3 and rd.max_len() == T
    names = ("label", "userid", "hist_item", "hist_cat", "hist_position", "target_item", "target_cat", "target_position")
    for i, b in enumerate(bs):
        assert len(b) == 8
        for t, name in zip(b, names):
            assert t.dtype == torch.int64 and np.array_equal(t.numpy(), want[name][4 * i:4 * i + 4]), name
    lens = (want["hist_item"] != 0).sum(1)
    assert lens.max() == T and 2 in lens.tolist()


def test_reader_pads_to_the_longest_history_of_the_whole_file_list(tmp_path):
    from paddlerec_amd.reader import AmazonBSTReader
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_text("userid:3 history:5 history:6 cate:1 cate:2 position:9 position:0 target:7 target_cate:2 "
                 "target_position:0 label:1 \nuserid:4 target:8 other:9 label:0\n")
    b.write_text("userid:5 history:1 history:2 history:3 history:4 cate:1 cate:1 cate:1 cate:1 position:3 position:2 "
                 "position:1 position:0 target:7 target_cate:2 target_position:0 label:0\n")
    first, = list(AmazonBSTReader([str(a), str(b)], 2, "cpu"))                 # drop_last: the third line is left over
    label, uid, hist, cate, pos, tgt, tcate, tpos = first
    assert tuple(hist.shape) == (2, 4)                                         # the SECOND file's history sets the length
    assert hist.tolist() == [[5, 6, 0, 0], [0, 0, 0, 0]] and cate.tolist() == [[1, 2, 0, 0], [0, 0, 0, 0]]
    assert pos.tolist() == [[9, 0, 0, 0], [0, 0, 0, 0]] and uid.tolist() == [[3], [4]] and label.tolist() == [[1], [0]]
    assert tgt.tolist() == [[7], [8]] and tcate.tolist() == [[2], [0]] and tpos.tolist() == [[0], [0]]   # missing slot: [0]
    assert tuple(list(AmazonBSTReader([str(a)], 2, "cpu"))[0][2].shape) == (2, 2)


def test_trainer_knows_the_model_and_trains_on_the_stand_in(tmp_path):
    from paddlerec_amd import trainer
    assert "bst" in trainer.MODELS and trainer.guess_model("/x/models/rank/bst/config.yaml") == "bst"
    assert type(trainer._dygraph_model("bst")).__module__ == "paddlerec_amd.bst"
    data = tmp_path / "data"
    data.mkdir()
    with open(os.path.join(GOLDEN, "bst_sample.txt")) as f:
        (data / "part-0").write_text(f.read())
    cfg = {"runner.train_data_dir": str(data), "runner.train_batch_size": 4, "runner.epochs": 1, "runner.print_interval": 1,
           "runner.model_save_path": str(tmp_path / "out"), "runner.use_gpu": False,
           "hyper_parameters.item_emb_size": 4, "hyper_parameters.cat_emb_size": 4, "hyper_parameters.position_emb_size": 4,
           "hyper_parameters.item_count": 63001, "hyper_parameters.user_count": 192403, "hyper_parameters.cat_count": 801,
           "hyper_parameters.position_count": 5001, "hyper_parameters.d_model": 12, "hyper_parameters.d_key": 4,
           "hyper_parameters.d_value": 4, "hyper_parameters.n_head": 3, "hyper_parameters.dropout_rate": 0.2,
           "hyper_parameters.postprocess_cmd": "da", "hyper_parameters.prepostprocess_dropout": 0.2,
           "hyper_parameters.d_inner_hid": 8, "hyper_parameters.fc_sizes": [8, 4]}
    out, _ = trainer.train(cfg, "bst", device="cpu", kernels=bst_cpu_kernels)
    assert len(out) == 1 and out[0]["batches"] == 3 and np.isfinite(out[0]["loss"]) and 0.0 <= out[0]["auc"] <= 1.0


# ------------------------------------------------------------------------------------------------ argument checks
def test_bst_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    import ctypes as C
    L, p, q = engine_lib, C.c_void_p(4096), C.c_void_p(8192)
    mha = lambda Ln, dk, ld, ptr=p: L.rec_mha_fwd(2, Ln, 3, dk, dk, ptr, ld, ptr, ld, ptr, ld, 1.0, 0.0, 0, 0, q, 3 * dk,
                                                  C.c_void_p(12288), None)
    assert mha(8193, 4, 12) == -2 and b"8192" in L.rec_last_error()                       # the stated limit on L
    assert mha(8, 6, 18) == -2 and mha(8, 68, 204) == -2 and mha(0, 4, 12) == -1            # d_k: multiple of 4, <= 64
    assert mha(8, 4, 8) == -1 and mha(8, 4, 14) == -1 and mha(8, 4, 12, C.c_void_p(4100)) == -1   # stride, alignment
    assert L.rec_mha_fwd(2, 8, 3, 4, 4, p, 12, p, 12, p, 12, 1.0, 1.0, 0, 0, q, 12, q, None) == -1   # p = 1
    assert L.rec_mha_fwd(0, 8, 3, 4, 4, None, 12, None, 12, None, 12, 1.0, 0.0, 0, 0, None, 12, None, None) == 0
    assert L.rec_mha_bwd(2, 8, 3, 4, 4, p, 12, p, 12, p, 12, 1.0, 0.0, 0, 0, q, 12, q, 12, q, q, p, 12, C.c_void_p(12288), 12,
                         C.c_void_p(16384), 12, None) == -1 and b"alias" in L.rec_last_error()     # dq is q
    assert L.rec_add_layer_norm_fwd(4, 8, p, 7, None, 0, 1e-5, q, 8, 0, 0, p, p, None) == -1        # ldx < n
    assert L.rec_add_layer_norm_fwd(4, 8, p, 8, None, 0, 1e-5, q, 8, 2, 15, p, p, None) == -1       # group stride too small
    assert L.rec_add_layer_norm_fwd(0, 8, None, 8, None, 0, 1e-5, None, 8, 0, 0, None, None, None) == 0
    assert L.rec_add_layer_norm_bwd(4, 8, q, 8, 0, 0, p, p, 8, q, 8, None) == -1                    # dx is y
    assert L.rec_leaky_relu_fwd(4, 8, p, 8, -0.1, q, 8, None) == -1 and L.rec_leaky_relu_bwd(4, 8, q, 8, p, 8, 0.01, q, 8, None) == -1
    assert L.rec_bst_add(4, 8, p, 8, None, 0, q, 7, None) == -1
    assert L.rec_bst_possum_fwd(4, 0, p, p, q, None) == -1 and L.rec_bst_possum_bwd(4, 3, p, p, q, None) == -1   # dz is dy
    assert L.rec_bst_embed_fwd(4, 7, None, None, None, None, None, p, 12, q, 12, p, None) == -1
