"""DMR on the GPU: the new kernels of csrc/dmr_ops.hip against tests/dmr_ref.py in float64, whole train steps against
the golden and the restatement, inference, and the trainer.

Tolerance, everywhere: err = max|got - ref64| / max|ref64| per tensor against dmr_ref.py in float64; the bound is 8 x the
same error of dmr_ref.py evaluated in float32 on the same inputs, floor 1e-6 (the factor 8: a different summation order).
Both errors are printed.  Parameters after Adam go through helpers.assert_adam_weights_close (test_dmr.py says why, and
why att_layer3_layer.bias is only held to what Adam can move).

Tiles, and the sizes one past them:
  * prefix pool: one 256-thread block per sample; the softmax walks T in strides of 256 (T 257 = one more), the pooling
    walks R * D items in strides of 256 (R 2 x D 68 = 136, D 64 x 2 = 128; R * D > 256 does not occur below 8 x 33), the
    backward's dots are one wave per position with lanes over D (D 64 = exactly a wave, 68 = one more) and 4 waves over
    T; B 1, 5, 65 = one block, a few, more than one block per XCD slot;
  * PReLU: 256 columns x 16 rows per block: n 1, 128, 130; virtual widths 400 (period 50 x n 8: two column blocks) and 8;
    m 37 / 150 / 74 (no multiples of 16); a row stride wider than n;
  * match loss: a thread per batch row, 256 per block (B 1, 17, 100); at most 64 class chunks — C 1, 7, 64 (one class
    per chunk), 65 (two per chunk, 33 chunks), 1031 (17 per chunk, 61 chunks); 16 batch chunks in dV (B 17: two rows per
    chunk, 9 chunks; B 100: 7 per chunk, 15 chunks); K 4, 32 (register arrays of exactly K / 4), 36 (9 float4 in an
    array of 12)."""
import os
import shutil

import numpy as np
import pytest
import torch

import dmr_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NOISE_GRAD = "att_layer3_layer.bias"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _close(name, got, ref64, ref32):
    e, e32 = R.relerr(_n(got) if isinstance(got, torch.Tensor) else got, ref64), R.relerr(ref32, ref64)
    print("%-40s err %.3g  float32-ref err %.3g" % (name, e, e32))
    assert e <= max(8 * e32, 1e-6), (name, e, e32)
    return e


@pytest.fixture(scope="module")
def ops(engine_lib):
    from paddlerec_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ prefix pool
def _mask(kind, T):
    m = np.zeros(T, np.int64)
    if kind == 0:
        m[:] = 1
    elif kind == 1:
        m[T - 1:] = 1
    elif kind == 2:
        m[max(T - 2, 0):] = 1
    elif kind == 4:
        m[:] = 1
        m[T // 3:max(T // 3 + 1, 2 * T // 3)] = 0
    return m


@pytest.mark.parametrize("T", [2, 3, 50, 65, 257])
def test_prefix_pool_against_float64(ops, T):
    rng = np.random.default_rng(100 + T)
    configs = [(1, [k]) for k in range(5)] + [(5, list(range(5))), (65, [b % 5 for b in range(65)])]
    for B, kinds in configs:
        mask = np.stack([_mask(k, T) for k in kinds])
        mask[mask == 0] = rng.integers(-1, 3, mask.shape)[mask == 0] * 2          # "not 1" is any other value (0, +-2, 4)
        for D in (4, 8, 64, 68):
            score = rng.standard_normal((B, T)).astype(F32) * 2
            wide = rng.standard_normal((B, T, D + 4)).astype(F32)                # hist as a strided view
            hist = wide[:, :, :D]
            feed = np.concatenate([rng.integers(0, 9, (B, 3)), mask, rng.integers(0, 9, (B, 2))], 1)   # mask as a view
            t_feed, t_wide, t_score = _t(feed), _t(wide), _t(score)
            t_mask, t_hist = t_feed[:, 3:3 + T], t_wide[:, :, :D]
            for rows, with_rel in (((max(T - 2, 0), T - 1), False), ((T - 1,), True), ((0,), False)):
                Rn = len(rows)
                tag = "B%d T%d D%d rows%s" % (B, T, D, rows)
                o64, w64, r64 = R.prefix_pool_fwd(score, mask, hist, rows)
                o32, w32, r32 = R.prefix_pool_fwd(score, mask, hist, rows, dtype=F32)
                frame = torch.full((B, Rn * D + 3), 7.0, device=DEV)             # out / rel as column ranges of a wider row
                out_v, rel_v = frame[:, :Rn * D], frame[:, Rn * D + 1:Rn * D + 2]
                out, w = ops.dmr_prefix_pool_fwd(t_score, t_mask, t_hist, rows, out=out_v, rel=rel_v if with_rel else None)
                _close(tag + " out", out, o64.reshape(B, -1), o32.reshape(B, -1))
                _close(tag + " w", w, w64, w32)
                assert (frame[:, Rn * D] == 7).all() and (frame[:, Rn * D + 2] == 7).all()
                if with_rel:
                    _close(tag + " rel", rel_v, r64.reshape(B, 1), r32.reshape(B, 1))
                else:
                    assert (rel_v == 7).all()
                uniform = np.stack([~((mask[:, :r + 1] == 1).any(1)) for r in rows], 1)          # [B, R]
                wn = _n(w)
                assert np.array_equal(wn[uniform], np.broadcast_to(F32(1) / F32(T), (int(uniform.sum()), T)))
                out2, w2 = ops.dmr_prefix_pool_fwd(t_score, t_mask, t_hist, rows)
                assert torch.equal(w2, w) and torch.equal(out2, out_v)           # bit-identical rerun
                # backward, overwrite and accumulate
                d_out = rng.standard_normal((B, Rn * D)).astype(F32)
                d_rel = rng.standard_normal((B, 1)).astype(F32) if with_rel else None
                ds64, dh64 = R.prefix_pool_bwd(mask, hist, rows, w64, d_out.reshape(B, Rn, D), d_rel)
                ds32, dh32 = R.prefix_pool_bwd(mask, hist, rows, w32, d_out.reshape(B, Rn, D), d_rel, dtype=F32)
                gframe = _t(np.concatenate([d_out, np.zeros((B, 1), F32), d_rel if with_rel else np.zeros((B, 1), F32)], 1))
                g_out, g_rel = gframe[:, :Rn * D], (gframe[:, Rn * D + 1:] if with_rel else None)
                dh_wide = torch.full((B, T, D + 2), 3.0, device=DEV)
                dh = dh_wide[:, :, :D]
                ds = ops.dmr_prefix_pool_bwd(t_mask, t_hist, rows, w, g_out, dh, d_rel=g_rel, accumulate=False)
                _close(tag + " dscore", ds, ds64, ds32)
                _close(tag + " d_hist", dh, dh64, dh32)
                assert (dh_wide[:, :, D:] == 3).all()
                dsn = _n(ds)
                gate = np.zeros((B, T), bool)
                for r in rows:
                    gate[:, :r + 1] |= mask[:, :r + 1] == 1
                if with_rel:
                    gate |= mask == 1
                assert not dsn[~gate].any()                                      # a padded entry: no gradient, even at w = 1/T
                first = dh.clone()
                ds2 = ops.dmr_prefix_pool_bwd(t_mask, t_hist, rows, w, g_out, dh, d_rel=g_rel, accumulate=True)
                assert torch.equal(ds2, ds)
                _close(tag + " d_hist +=", dh, 2 * dh64, 2 * dh32)
                dh3 = torch.empty(B, T, D, device=DEV)
                ops.dmr_prefix_pool_bwd(t_mask, t_hist, rows, w, g_out, dh3, d_rel=g_rel, accumulate=False)
                assert torch.equal(dh3, first)


# ------------------------------------------------------------------------------------------------ PReLU
@pytest.mark.parametrize("m,n,period,base,num_alpha", [(37, 1, 0, 0, 1), (37, 128, 0, 0, 128), (37, 130, 0, 0, 130),
                                                       (150, 8, 50, 0, 50), (74, 4, 2, 48, 50), (75, 4, 2, 48, 50)])
def test_prelu_against_float64(ops, m, n, period, base, num_alpha):
    rng = np.random.default_rng(7 * m + n)
    x = rng.standard_normal((m, n + 3)).astype(F32)
    x[rng.random(x.shape) < 0.15] = 0.0                                          # exact zeros (and negatives)
    dy = rng.standard_normal((m, n)).astype(F32)
    alpha = rng.uniform(0.05, 0.5, num_alpha).astype(F32)
    xv = x[:, :n]
    assert (xv == 0).any() and (xv < 0).any()
    tx = _t(x)[:, :n]                                                            # a row stride wider than n
    ws = ops.Workspace(DEV)
    y = ops.prelu_fwd(tx, _t(alpha), period=period, base=base)
    _close("prelu y", y, R.prelu_fwd(xv, alpha, period, base), R.prelu_fwd(xv, alpha, period, base, dtype=F32))
    dx, da = ops.prelu_bwd(tx, _t(dy), _t(alpha), ws, period=period, base=base)
    dx64, da64 = R.prelu_bwd(xv, dy, alpha, period, base)
    dx32, da32 = R.prelu_bwd(xv, dy, alpha, period, base, dtype=F32)
    _close("prelu dx", dx, dx64, dx32)
    _close("prelu dalpha", da, da64, da32)
    if period:
        untouched = np.ones(num_alpha, bool)
        untouched[base:base + period] = False
        assert not _n(da)[untouched].any()                                       # every entry written: 0 where unreached
    dx2, da2 = ops.prelu_bwd(tx, _t(dy), _t(alpha), ws, period=period, base=base, dalpha=torch.full_like(da, 9.0))
    assert torch.equal(dx2, dx) and torch.equal(da2, da)


# ------------------------------------------------------------------------------------------------ match loss
@pytest.mark.parametrize("K", [4, 32, 36])
def test_match_loss_against_float64(ops, K):
    rng = np.random.default_rng(K)
    ws = ops.Workspace(DEV)
    for B in (1, 17, 100):
        for Cn in (1, 7, 64, 65, 1031):
            U = rng.standard_normal((B, K)).astype(F32)
            V = (rng.standard_normal((Cn, K)) * 0.7).astype(F32)
            bias = (rng.standard_normal(Cn) * 0.5).astype(F32) if (B + Cn) % 2 else None
            label = rng.integers(0, Cn, B)
            label[0] = Cn - 1
            if B > 2:
                U[1] = 0.0                                                        # an all-zero row
                label[1], label[2], label[B - 1] = 0, Cn - 1, label[3]            # 0, C-1 and duplicate labels
            tag = "B%d C%d K%d" % (B, Cn, K)
            tU, tV, tb, tl = _t(U), _t(V), (None if bias is None else _t(bias)), _t(label)
            l64, lse64 = R.match_loss_fwd(U, V, bias, label)
            l32, lse32 = R.match_loss_fwd(U, V, bias, label, dtype=F32)
            loss, lse, status = ops.dmr_match_loss_fwd(tU, tV, tb, tl, ws)
            _close(tag + " loss", loss, [l64], [l32])
            _close(tag + " lse", lse, lse64, lse32)
            assert int(status.item()) == 0
            if B > 2 and bias is None:
                assert abs(float(lse[1]) - np.log(Cn)) <= 1e-6 * max(np.log(Cn), 1)          # zero row: log C
            dU64, dV64 = R.match_loss_bwd(U, V, bias, label, 0.1)
            dU32, dV32 = R.match_loss_bwd(U, V, bias, label, 0.1, dtype=F32)
            dV = torch.full((Cn, K), 5.0, device=DEV)
            dU = ops.dmr_match_loss_bwd(tU, tV, tb, tl, lse, 0.1, dV, ws, accumulate=False)
            _close(tag + " dU", dU, dU64, dU32)
            _close(tag + " dV", dV, dV64, dV32)
            if B > 2 and bias is None:                                           # zero row: the scaled mean row of V - its label's row
                want = 0.1 / B * (V.astype(np.float64).mean(0) - V[label[1]].astype(np.float64))
                assert R.relerr(_n(dU)[1], want) <= 1e-5
            first = dV.clone()
            dU2 = ops.dmr_match_loss_bwd(tU, tV, tb, tl, lse, 0.1, dV, ws, accumulate=True)
            _close(tag + " dV +=", dV, 2 * dV64, 2 * dV32)
            assert torch.equal(dU2, dU)
            loss2, lse2, _ = ops.dmr_match_loss_fwd(tU, tV, tb, tl, ws)
            dV3 = torch.empty(Cn, K, device=DEV)
            ops.dmr_match_loss_bwd(tU, tV, tb, tl, lse2, 0.1, dV3, ws, accumulate=False)
            assert torch.equal(loss2, loss) and torch.equal(lse2, lse) and torch.equal(dV3, first)   # bit-identical reruns


def test_match_loss_large_logits_strided_label_and_bad_label(ops):
    rng = np.random.default_rng(5)
    B, Cn, K = 17, 65, 32
    ws = ops.Workspace(DEV)
    U = rng.standard_normal((B, K)).astype(F32)
    V = rng.standard_normal((Cn, K)).astype(F32)
    U[0], V[3], V[4] = 3.0, 1.05, -1.05                                          # logits of about +100 and -100
    z = U.astype(np.float64) @ V.astype(np.float64).T
    assert z.max() > 100 and z.min() < -100                                      # exp overflows without the running maximum
    ids = rng.integers(0, Cn, (B, 5))
    t_ids = _t(ids)
    label = ids[:, 4]
    l64, lse64 = R.match_loss_fwd(U, V, None, label)
    l32, lse32 = R.match_loss_fwd(U, V, None, label, dtype=F32)
    loss, lse, status = ops.dmr_match_loss_fwd(_t(U), _t(V), None, t_ids[:, 4], ws)          # label as a strided column
    assert torch.isfinite(lse).all()
    _close("large loss", loss, [l64], [l32])
    _close("large lse", lse, lse64, lse32)
    dU64, dV64 = R.match_loss_bwd(U, V, None, label, 1.0)
    dU32, dV32 = R.match_loss_bwd(U, V, None, label, 1.0, dtype=F32)
    dV = torch.empty(Cn, K, device=DEV)
    dU = ops.dmr_match_loss_bwd(_t(U), _t(V), None, t_ids[:, 4], lse, 1.0, dV, ws)
    _close("large dU", dU, dU64, dU32)
    _close("large dV", dV, dV64, dV32)
    assert int(status.item()) == 0
    # a label outside [0, C): the flag, no fault, and the row contributes its lse alone
    bad = label.copy()
    bad[2], bad[5] = Cn, -1
    l64, _ = R.match_loss_fwd(U, V, None, bad)
    l32, _ = R.match_loss_fwd(U, V, None, bad, dtype=F32)
    loss, lse, status = ops.dmr_match_loss_fwd(_t(U), _t(V), None, _t(bad), ws)
    from paddlerec_amd import _lib
    assert int(status.item()) & _lib.REC_FLAG_INDEX_OOB
    _close("bad-label loss", loss, [l64], [l32])
    dU64, dV64 = R.match_loss_bwd(U, V, None, bad, 1.0)
    dU32, dV32 = R.match_loss_bwd(U, V, None, bad, 1.0, dtype=F32)
    dU = ops.dmr_match_loss_bwd(_t(U), _t(V), None, _t(bad), lse, 1.0, dV, ws)
    _close("bad-label dU", dU, dU64, dU32)
    _close("bad-label dV", dV, dV64, dV32)


# ------------------------------------------------------------------------------------------------ layer and trainer
@pytest.fixture(scope="module")
def gold():
    g = R.load_golden(GOLDEN)
    p = {k[2:]: g[k] for k in g if k.startswith("p_")}
    return dict(g=g, p=p, lr=float(g["lr"][0]))


def _layer(gold):
    from paddlerec_amd.dmr import DMRLayer
    m = DMRLayer(*[int(x) for x in gold["g"]["sizes"][4:]], 4, 2, device=DEV)
    m.set_dict(gold["p"])
    return m


def _adam_check(got, want, key, lr, steps):
    if key == NOISE_GRAD:
        assert np.abs(np.asarray(got, np.float64) - want).max() <= 2.0 * steps * lr * 3.17
        return
    assert_adam_weights_close(got, want, lr, steps, err_msg=key)


def test_layer_three_train_steps_and_infer(engine_lib, gold):
    g, p, lr = gold["g"], gold["p"], gold["lr"]
    m = _layer(gold)
    feeds = [_t(g["sparse"]), _t(g["price"])]
    p64, p32, st64, st32 = p, p, None, None
    for step in range(3):
        c64, g64, p64, st64 = R.train_step(p64, g["sparse"], g["price"], lr, st64)
        c32, g32, p32, st32 = R.train_step(p32, g["sparse"], g["price"], lr, st32, dtype=F32)
        loss, y_hat, aux, ctr = m.train_step(feeds, lr=lr)
        for k, got in (("y_hat", y_hat), ("aux", aux), ("ctr", ctr), ("loss", loss)):
            _close("step %d %s" % (step, k), got, c64[k], c32[k])
        if step == 0:
            grads = m.last_gradients()
            for k in p:
                if k not in R.NO_GRAD:
                    _close("g_" + k, grads[k], g64[k], g32[k])
            for k, got in (("y_hat", y_hat), ("aux", aux), ("ctr", ctr), ("loss", loss)):     # the golden itself
                assert R.relerr(_n(got), g[k]) <= max(8 * R.relerr(c32[k], c64[k]), 1e-6) + R.relerr(c64[k], g[k]), k
            sd = m.state_dict()
            for k in p:
                if k not in R.NO_GRAD:
                    _adam_check(_n(sd[k]), g["n_" + k], k, lr, 1)
            for k in ("inp_layer._mean", "inp_layer._variance"):
                _close(k, sd[k], p64[k], p32[k])
            assert np.array_equal(_n(sd["logits_layer.weight"]), g["p_logits_layer.weight"])
    sd = m.state_dict()
    for k in p:
        if k not in R.NO_GRAD:
            _adam_check(_n(sd[k]), p64[k], k, lr, 3)
    assert int(m.status.item()) == 0
    m.eval()
    y_hat, one = m(feeds, 1)
    now = {k: _n(v) for k, v in sd.items()}
    c64 = R.forward(now, g["sparse"], g["price"], train=False)
    c32 = R.forward(now, g["sparse"], g["price"], train=False, dtype=F32)
    _close("infer y_hat", y_hat, c64["y_hat"], c32["y_hat"])
    assert float(one) == 1.0


def test_trainer_model_dmr_train_save_load_infer(engine_lib, tmp_path, monkeypatch):
    """--model dmr on the sample lines: one epoch of one batch (32 of the 36 lines: drop_last), checkpoint, infer; the
    epoch's loss is dmr_ref's on that batch from the same initial parameters."""
    import pickle
    from paddlerec_amd import trainer
    from paddlerec_amd.dmr import DMRLayer
    rows = np.load(os.path.join(GOLDEN, "dmr_reader.npz"))["rows"]
    sparse = rows.astype(np.int64)
    T = 50
    col = lambda i: int(sparse[:, 5 * T + i].max()) + 1
    sizes = dict(user_size=col(0), cms_segid_size=col(1), cms_group_id_size=col(2), final_gender_code_size=col(3),
                 age_level_size=col(4), pvalue_level_size=col(5), shopping_level_size=col(6), occupation_size=col(7),
                 new_user_class_level_size=col(8), adgroup_id_size=col(9),
                 cate_size=max(col(10), int(sparse[:, T:2 * T].max()) + 1), campaign_id_size=col(11), customer_size=col(12),
                 brand_size=max(col(13), int(sparse[:, 2 * T:3 * T].max()) + 1), btag_size=int(sparse[:, :T].max()) + 1,
                 pid_size=col(15))
    d = tmp_path / "dmr"
    (d / "data").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "dmr_sample.txt"), d / "data" / "sample.txt")
    monkeypatch.chdir(d)
    out = str(tmp_path / "out")
    (d / "config.yaml").write_text(
        "runner:\n  train_data_dir: data\n  test_data_dir: data\n  train_batch_size: 32\n  epochs: 1\n  print_interval: 1\n"
        "  use_auc: True\n  model_save_path: %s\n  infer_batch_size: 16\n  infer_load_path: %s\n  infer_start_epoch: 0\n"
        "  infer_end_epoch: 1\nhyper_parameters:\n  optimizer:\n    class: Adam\n    learning_rate: 0.008\n%s"
        "  main_embedding_size: 4\n  other_embedding_size: 2\n" % (out, out, "".join("  %s: %d\n" % kv for kv in sizes.items())))
    config = trainer.load_yaml(str(d / "config.yaml"))
    assert trainer.guess_model(str(d / "config.yaml")) == "dmr"
    summaries, model = trainer.train(config, "dmr")
    assert len(summaries) == 1 and summaries[0]["batches"] == 1 and summaries[0]["samples"] == 32
    torch.manual_seed(config.get("runner.seed", 12345))                          # trainer.train's seed: the same start
    order = ("user_size", "cms_segid_size", "cms_group_id_size", "final_gender_code_size", "age_level_size",
             "pvalue_level_size", "shopping_level_size", "occupation_size", "new_user_class_level_size", "adgroup_id_size",
             "cate_size", "campaign_id_size", "customer_size", "brand_size", "btag_size", "pid_size")
    start = {k: _n(v) for k, v in DMRLayer(*[sizes[k] for k in order], 4, 2, device=DEV).state_dict().items()}
    price = rows[:32, 264:265]
    c64 = R.forward(start, sparse[:32], price)
    c32 = R.forward(start, sparse[:32], price, dtype=F32)
    _close("trainer loss", np.asarray([summaries[0]["loss"]]), c64["loss"], c32["loss"])
    with open(os.path.join(out, "0", "rec.pdparams"), "rb") as f:
        sd = pickle.load(f)
    assert sorted(sd) == sorted(R.param_keys()) and all(np.isfinite(v).all() for v in sd.values())
    assert np.array_equal(sd["logits_layer.weight"], start["logits_layer.weight"])
    res = trainer.infer(config, "dmr")
    assert len(res) == 1 and res[0]["batches"] == 2 and 0.0 <= res[0]["auc"] <= 1.0
