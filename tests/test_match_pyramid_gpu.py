"""MatchPyramid on the GPU: the three entry points of csrc/match_pyramid_ops.hip against tests/match_pyramid_ref.py in float64,
and the layer (paddlerec_amd/match_pyramid.py) against the goldens recorded from the reference's own net.py.

Kernel cases: every output is NaN-poisoned (argmax: -7) before the call and every leading dimension is padded, so a missing
write shows as a NaN inside and a stray one as a number outside.  Tolerance: tests/match_pyramid_checks.py (8 x the float32
error of the restatement, floor 1e-6; dL / dR row by row; argmax exact)."""
import ast
import os

import numpy as np
import pytest
import torch

import match_pyramid_checks as K
import match_pyramid_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _shape(Ll, Lr, E, Kc, filt, pool, stride, relu=True):
    from paddlerec_amd import ops
    return ops.MpyrShape(Ll, Lr, E, Kc, filt[0], filt[1], pool[0], pool[1], stride[0], stride[1], int(relu))


def _cfg(s, pad):
    return dict(pad=pad, filter=(s.filter_h, s.filter_w), pool=(s.pool_h, s.pool_w), stride=(s.stride_h, s.stride_w),
                relu=bool(s.relu), pairs=1)


def _problem(s, B, V, seed, pad_frac=0.1, integer=False):
    """table [V, E] (row V - 1 is the padding row), ids with paddings, conv weights and a gradient of the pooled values."""
    rng = np.random.default_rng(seed)
    N = s.channels * ((s.left_len - s.pool_h) // s.stride_h + 1) * ((s.right_len - s.pool_w) // s.stride_w + 1)
    if integer:
        draw = lambda *sh: rng.integers(-2, 3, sh).astype(np.float32)
    else:
        draw = lambda *sh: (0.5 * rng.standard_normal(sh)).astype(np.float32)
    table, w, b, dp = draw(V, s.emb_dim), draw(s.channels, 1, s.filter_h, s.filter_w), draw(s.channels), draw(B, N)
    left, right = rng.integers(0, V - 1, (B, s.left_len)), rng.integers(0, V - 1, (B, s.right_len))
    left[rng.random(left.shape) < pad_frac] = V - 1
    right[rng.random(right.shape) < pad_frac] = V - 1
    return dict(table=table, w=w, b=b, dp=dp, left=left.astype(np.int64), right=right.astype(np.int64), pad=V - 1, N=N)


def _poisoned(rows, cols, extra, dtype=torch.float32, fill=float("nan")):
    buf = torch.full((rows, cols + extra), fill, dtype=dtype, device=DEV)
    return buf, buf[:, :cols]


def _run(s, pr):
    """Both kernels on the problem -> dict of numpy outputs; asserts that nothing was written outside the views and that every
    element inside was."""
    from paddlerec_amd import ops
    t = lambda a: torch.as_tensor(a).to(DEV)
    B, N, E = pr["left"].shape[0], pr["N"], s.emb_dim
    V = pr["table"].shape[0]
    tab_buf = torch.full((V, E + 3), 7.0, dtype=torch.float32, device=DEV)             # a row stride that is not E
    tab_buf[:, :E] = t(pr["table"])
    table = tab_buf[:, :E]
    left, right, w, b = t(pr["left"]), t(pr["right"]), t(pr["w"]), t(pr["b"])
    status = ops.new_status(DEV)
    pbuf, pooled = _poisoned(B, N, 5)
    abuf, argmax = _poisoned(B, N, 3, torch.int32, -7)
    ops.mpyr_fwd(s, left, right, table, w, b, pr["pad"], status, out=(pooled, argmax))
    dpbuf, dp = _poisoned(B, N, 2)
    dp.copy_(t(pr["dp"]))
    lbuf, dL = _poisoned(B * s.left_len, E, 2)
    rbuf, dR = _poisoned(B * s.right_len, E, 6)
    dw = torch.full((s.channels * s.filter_h * s.filter_w,), float("nan"), device=DEV)
    db = torch.full((s.channels,), float("nan"), device=DEV)
    ops.mpyr_bwd(s, left, right, table, w, b, dp, argmax, dL, dR, dw, db, pr["pad"])
    torch.cuda.synchronize()
    for buf, width in ((pbuf, N), (lbuf, E), (rbuf, E)):
        assert bool(torch.isnan(buf[:, width:]).all()) and not bool(torch.isnan(buf[:, :width]).any())
    assert bool((abuf[:, N:] == -7).all()) and bool((abuf[:, :N] >= 0).all())
    assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any())
    n = lambda x: x.cpu().numpy()
    return dict(pooled=n(pooled), argmax=n(argmax), dL=n(dL), dR=n(dR), d_w=n(dw), d_b=n(db), status=int(status.item()))


def _refs(s, pr):
    cfg = _cfg(s, pr["pad"])
    out = []
    for dt in (np.float64, np.float32):
        f = R.interaction_fwd(pr["table"], pr["left"], pr["right"], pr["w"], pr["b"], cfg, dt)
        bw = R.interaction_bwd(f, pr["dp"], cfg, dt)
        out.append(dict(pooled=f["pooled"], argmax=f["argmax"], pre=f["pre"], xp=f["xp"], **bw))
    return out


def _check(s, pr, what, exact=False):
    got = _run(s, pr)
    r64, r32 = _refs(s, pr)
    assert np.array_equal(r32["argmax"], r64["argmax"])                 # the case itself has no near-tie
    assert np.array_equal(got["argmax"], r64["argmax"]), what
    for k in ("pooled", "d_w", "d_b"):
        if exact:
            assert np.array_equal(got[k].reshape(r64[k].shape), r64[k]), (what, k)
        else:
            K.check_tensor(what, k, got[k], r64[k], r32[k])
    for k in ("dL", "dR"):
        if exact:
            assert np.array_equal(got[k].reshape(r64[k].shape), r64[k]), (what, k)
        else:
            K.check_rows(what, k, got[k], r64[k], r32[k])
    return got, r64


# name -> (shape, B, V): a the shipped shape (rows 18 and 19 are unpooled, E is no multiple of 4); b minimal, an odd filter; c an
# even filter on both axes and leftovers on both; d1 overlapping windows (a cell may win two), d2 gapped windows; f more
# blocks than one wave of the chip holds, and one sample
CASES = {
    "a_shipped": (lambda: _shape(20, 500, 50, 8, (2, 10), (6, 50), (6, 50)), 3, 600),
    "b_minimal": (lambda: _shape(4, 6, 1, 1, (3, 3), (2, 2), (2, 2)), 2, 9),
    "c_even_leftover": (lambda: _shape(7, 23, 6, 3, (2, 4), (3, 5), (3, 5)), 5, 50),
    "c_no_relu": (lambda: _shape(7, 23, 6, 3, (2, 4), (3, 5), (3, 5), relu=False), 5, 50),
    "d_overlap": (lambda: _shape(7, 23, 6, 3, (2, 4), (3, 4), (2, 3)), 5, 50),
    "d_gapped": (lambda: _shape(7, 23, 6, 3, (2, 4), (2, 2), (3, 4)), 5, 50),
    "f_one": (lambda: _shape(7, 23, 6, 3, (2, 4), (3, 5), (3, 5)), 1, 50),
    "f_many": (lambda: _shape(7, 23, 6, 3, (2, 4), (3, 5), (3, 5)), 300, 50),
    "wide_tile": (lambda: _shape(9, 300, 20, 11, (3, 2), (4, 30), (2, 25)), 2, 80),        # two column tiles, K over one chunk
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_interaction_kernels_against_float64(name):
    make, B, V = CASES[name]
    s = make()
    pr = _problem(s, B, V, seed=sorted(CASES).index(name) + 1)
    got, r64 = _check(s, pr, name)
    assert got["status"] == 0
    if name == "a_shipped":
        assert (got["argmax"] // 500).max() <= 17                      # rows 18 and 19 are never pooled
    if name == "d_overlap":
        am = got["argmax"].reshape(B, 3, -1)
        assert any(len(set(ch.tolist())) < ch.size for smp in am for ch in smp)          # a cell that won two windows


def test_integer_case_ties_dead_windows_padding_and_an_id_out_of_range():
    """Case e: small integers, so float32 is exact and every output is compared bit for bit."""
    from paddlerec_amd import _lib
    s = _shape(7, 23, 6, 3, (2, 4), (3, 5), (3, 5))
    V = 12
    pr = _problem(s, 6, V, seed=5, integer=True)
    pr["w"][0], pr["b"][0] = 0.0, -1.0                                  # channel 0: every window is all <= 0 before ReLU
    pr["left"][1] = V - 1                                               # a fully padded left sentence
    pr["right"][2, 14:] = V - 1                                         # a fully padded right tail
    pr["left"][3, 2], pr["right"][3, 5] = V, V                          # an id equal to V
    got, r64 = _check(s, pr, "e_integer", exact=True)
    assert got["status"] & _lib.REC_FLAG_INDEX_OOB
    N1 = pr["N"] // 3
    assert not got["pooled"][:, :N1].any()                              # the dead channel: pooled 0 ...
    zero_dp = dict(pr, dp=pr["dp"] * np.repeat([0, 1, 1], N1)[None, :].astype(np.float32))
    again = _run(s, zero_dp)
    for k in ("dL", "dR", "d_w", "d_b"):                                # ... and its gradient changes nothing
        assert np.array_equal(again[k], got[k]), k
    assert not got["d_w"].reshape(3, -1)[0].any() and got["d_b"][0] == 0
    assert not got["dL"].reshape(6, 7, 6)[1].any() and not got["dR"].reshape(6, 23, 6)[2, 14:].any()
    assert not got["dL"].reshape(6, 7, 6)[3, 2].any() and not got["dR"].reshape(6, 23, 6)[3, 5].any()
    # an exact positive tie between two cells of one window whose tap footprints differ: the first in row-major order won
    cfg, act, xp = _cfg(s, pr["pad"]), np.maximum(r64["pre"], 0), r64["xp"]
    found = 0
    for b in range(6):
        for k in range(1, 3):
            for p in range(2):
                for q in range(4):
                    win = act[b, k, 3 * p:3 * p + 3, 5 * q:5 * q + 5].reshape(-1)
                    top = np.flatnonzero(win == win.max())
                    if win.max() > 0 and len(top) > 1:
                        cells = [(3 * p + c // 5, 5 * q + c % 5) for c in top[:2]]
                        if not np.array_equal(*[xp[b, i:i + 2, j:j + 4] for i, j in cells]):
                            found += 1
                            assert got["argmax"][b, k * 8 + p * 4 + q] == cells[0][0] * 23 + cells[0][1]
    assert found > 0


def test_channel_group_split_writes_the_same_bits(tmp_path):
    """REC_MPYR_SPLIT=channel, the alternative grid tools/match_pyramid_bench.py measures: the library reads the variable once, so
    a child process runs the forward (11 channels: three groups, the last one short) and this one compares."""
    import subprocess
    import sys
    make, B, V = CASES["wide_tile"]
    want = _run(make(), _problem(make(), B, V, seed=9))
    code = ("import sys, numpy as np; sys.path[:0] = %r; import test_match_pyramid_gpu as T; make, B, V = T.CASES['wide_tile']; "
            "got = T._run(make(), T._problem(make(), B, V, seed=9)); np.savez(%r, pooled=got['pooled'], argmax=got['argmax'])"
            % ([os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))],
               str(tmp_path / "child.npz")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, REC_MPYR_SPLIT="channel"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "child.npz")
    assert np.array_equal(got["argmax"], want["argmax"]) and np.array_equal(got["pooled"], want["pooled"])


def test_a_left_id_out_of_range_in_an_unpooled_row_is_flagged():
    """Image row 7 of 8 lies below the last pool window and its filter's reach (pool and stride 3, filter height 2: rows 0 to 6
    are read) and belongs to no block's band: an id outside the table there changes no output and still sets the status bit."""
    from paddlerec_amd import _lib
    s = _shape(8, 23, 6, 3, (2, 4), (3, 5), (3, 5))
    pr = _problem(s, 4, 30, seed=21)
    clean = _run(s, pr)
    assert clean["status"] == 0
    pr["left"][2, 7] = 30
    got = _run(s, pr)
    assert got["status"] & _lib.REC_FLAG_INDEX_OOB
    assert np.array_equal(got["pooled"], clean["pooled"]) and np.array_equal(got["argmax"], clean["argmax"])
    assert not got["dL"].reshape(4, 8, 6)[2, 7].any()


@pytest.mark.parametrize("B, pairs", [(128, 64), (130, 64), (2, 1), (600, 300)])
def test_hinge_against_float64(B, pairs):
    from paddlerec_amd import ops
    rng = np.random.default_rng(B)
    pred = rng.standard_normal((B, 1)).astype(np.float32)
    loss = torch.full((1,), float("nan"), device=DEV)
    dbuf = torch.full((B + 4,), float("nan"), device=DEV)
    ops.mpyr_hinge(torch.as_tensor(pred).to(DEV), pairs, out=(loss, dbuf[:B]))
    (l64, d64, _), (l32, d32, _) = R.hinge(pred, pairs, np.float64), R.hinge(pred, pairs, np.float32)
    K.check_tensor("hinge", "loss B %d" % B, loss.cpu().numpy(), np.asarray([l64]), np.asarray([l32]))
    d = dbuf.cpu().numpy()
    assert np.isnan(d[B:]).all() and np.array_equal(d[:B], d64.astype(np.float32))       # +-1 / pairs or 0, exactly
    assert not d[2 * pairs:B].any()


def test_hinge_pinned_at_exactly_zero_passes_the_gradient():
    from paddlerec_amd import ops
    pred = torch.tensor([[1.5], [3.0], [0.25], [0.5], [0.0], [-0.75]], device=DEV)         # terms 0, -2, 0: exact in float32
    loss, d = ops.mpyr_hinge(pred, 3)
    assert float(loss) == 0.0 and d.cpu().tolist() == [-1 / np.float32(3), 0, -1 / np.float32(3), 1 / np.float32(3), 0,
                                                       1 / np.float32(3)]


# ------------------------------------------------------------------------------------------------ the layer
@pytest.mark.parametrize("name", K.GOLDENS)
def test_layer_two_steps_and_infer_against_the_golden(name):
    G = K.gold(name)
    m = K.layer_of(G, DEV)
    K.check_layer(G, m, name)
    K.check_infer(G, m, name)


def test_layer_step_is_bit_identical_from_run_to_run_and_survives_a_checkpoint(tmp_path):
    from paddlerec_amd import checkpoint
    G = K.gold(K.GOLDENS[0])
    runs = []
    for _ in range(2):
        m = K.layer_of(G, DEV)
        m.set_dict(K.full_state(G, G["p"]))
        loss = m.train_step(K.feeds_of(G, "*_0", DEV), lr=G["lr"])
        grads = {k: v.clone() for k, v in m.store.view["g"].items()}
        grads["emb.weight"] = m._last["rows"].clone()          # dL | dR as the kernel wrote them (last_gradients scatters with torch)
        runs.append((loss.clone(), {k: v.clone() for k, v in m.state_dict().items()}, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]) and torch.equal(runs[0][2][k], runs[1][2][k]), k
    # state_dict, moments and the step count through checkpoint.py: the next step is the same bits
    checkpoint.save_model(m, None, str(tmp_path), 0)
    m2 = K.layer_of(G, DEV)
    checkpoint.load_model(os.path.join(str(tmp_path), "0"), m2)
    for a, b in zip((m.state_dict(),) + m.moments(), (m2.state_dict(),) + m2.moments()):
        assert all(torch.equal(a[k], b[k]) for k in a)
    m2.step_count = m.step_count
    l1, l2 = (x.train_step(K.feeds_of(G, "*_1", DEV), lr=G["lr"]) for x in (m, m2))
    assert torch.equal(l1, l2) and all(torch.equal(m.state_dict()[k], m2.state_dict()[k]) for k in m.state_dict())


def test_trainer_trains_two_steps_on_the_sample(tmp_path, capsys):
    """--model by the directory name `match-pyramid`: two epochs of one batch of 128 on the reference's whole 128-line train
    sample at the shipped sentence sizes, filter and pool, emb_size 6, from a checkpoint of known parameters
    (runner.model_init_path).  The first epoch's loss is the restatement's loss on those lines from those parameters, and the
    second differs: the step moved the parameters."""
    from paddlerec_amd import checkpoint, trainer
    from paddlerec_amd.match_pyramid import MatchPyramidLayer
    from paddlerec_amd.reader import letor_parse
    root = tmp_path / "match-pyramid"
    (root / "data" / "train").mkdir(parents=True)
    path = K.sample_train(root / "data" / "train")
    torch.manual_seed(1234)
    m = MatchPyramidLayer("none.npy", 193368, 6, 8, [2, 10], "relu", 20, 1, [6, 50], [6, 50], "VALID", "max", "relu", 20, 500,
                          device=DEV)
    table = m.state_dict()["emb.weight"]
    table.copy_(0.5 * torch.randn_like(table))                  # XavierNormal over 193 368 rows leaves every prediction near 0
    table[K.PAD].zero_()
    init = checkpoint.save_model(m, None, str(tmp_path / "init"), 0)
    (root / "config.yaml").write_text(
        "runner:\n  train_data_dir: data/train\n  train_batch_size: 128\n  epochs: 2\n  print_interval: 1\n  model_save_path: %s\n"
        "  model_init_path: %s\n"
        "hyper_parameters:\n  optimizer:\n    class: adam\n    learning_rate: 0.001\n  emb_path: none.npy\n"
        "  sentence_left_size: 20\n  sentence_right_size: 500\n  vocab_size: 193368\n  emb_size: 6\n  kernel_num: 8\n"
        "  hidden_size: 20\n  hidden_act: relu\n  out_size: 1\n  channels: 1\n  conv_filter: [2, 10]\n  conv_act: relu\n"
        "  pool_size: [6, 50]\n  pool_stride: [6, 50]\n  pool_type: max\n  pool_padding: VALID\n" % (tmp_path / "out", init))
    assert trainer.guess_model(str(root / "config.yaml")) == "match-pyramid"
    trainer.main(["-m", str(root / "config.yaml"), "--device", DEV])
    epochs = [ast.literal_eval(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [(e["batches"], e["samples"]) for e in epochs] == [(1, 128), (1, 128)]
    assert all(np.isfinite(e["loss"]) and e["loss"] > 0 for e in epochs)
    assert epochs[0]["loss"] != epochs[1]["loss"] and epochs[0]["loss"] != 1.0
    assert os.path.exists(os.path.join(str(tmp_path / "out"), "1", "rec.pdparams"))
    # the restatement on the rows the 128 lines name, from the parameters the trainer started from
    left, right = letor_parse([path])
    rows = np.unique(np.concatenate([left.reshape(-1), right.reshape(-1), [K.PAD]]))
    p = {k: v.cpu().numpy() for k, v in m.state_dict().items() if k != "emb.weight"}
    p["emb.weight"] = table[torch.as_tensor(rows).to(DEV)].cpu().numpy()
    cfg = dict(pad=len(rows) - 1, filter=(2, 10), pool=(6, 50), stride=(6, 50), relu=True, pairs=64)
    want = [R.loss_and_grads(p, R.compact_ids(rows, left), R.compact_ids(rows, right), cfg, dt)["loss"] for dt in (np.float64,
                                                                                                                  np.float32)]
    print("trainer epoch losses", [e["loss"] for e in epochs], "restatement", want)
    K.check_tensor("trainer", "epoch 0 loss", np.asarray([epochs[0]["loss"]]), want[0], want[1])
