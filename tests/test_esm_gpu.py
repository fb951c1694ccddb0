"""The entire-space kernels (csrc/esm_ops.hip) and nets (paddlerec_amd/esmm.py, escm2.py) on the GPU against tests/esm_ref.py.

Pool: the output is compared BIT FOR BIT with a NumPy loop that adds the rows in l order in float32 (the kernel's chain:
one add per kept id, from +0).  Shapes: B below / across a block's pairs (a block holds 256 >> k pairs, k from D / VEC),
L 1 / 3 / 5, D 4 and 12 on the float4 path (1 and 3 chunks a pair), D 9 and a row stride of `out` that is no multiple of 4
on the scalar path, and D 260 (float4) / 70 (scalar): more column chunks than the 64 lanes of a pair, i.e. two column passes.
Head: err = max|got - ref64| / max|ref64| per output, bound max(8 x the float32 restatement's error on the same inputs,
1e-6) (esm_checks.py); B 1, 5 and 1025 (five blocks of the head, five passes of the one-block click count)."""
import numpy as np
import pytest
import torch

import esm_checks as K
import esm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
N_ROWS, FIELDS = 50, 3

# name: (B, L, D, guard columns behind every row of out, extra floats behind every row of W)
POOL_CASES = {
    "b1_l1_d4": (1, 1, 4, 4, 0),
    "b7_l3_d12_strided_table": (7, 3, 12, 4, 4),
    "b65_l5_d4": (65, 5, 4, 8, 0),
    "b65_l3_d12_packed": (65, 3, 12, 0, 0),
    "b7_l5_d9_scalar": (7, 5, 9, 0, 0),
    "b65_l3_d9_scalar_strided": (65, 3, 9, 5, 3),
    "b7_l3_d12_misaligned_ld_out": (7, 3, 12, 3, 0),
    "b65_l1_d12_misaligned_ld_out": (65, 1, 12, 1, 0),
    "b3_l3_d260_two_passes": (3, 3, 260, 4, 0),
    "b3_l3_d70_scalar_two_passes": (3, 3, 70, 2, 0),
}


def _pool_loop(W, ids, padding_idx):
    """The kernel's chain in NumPy float32: per (b, f) from +0, one add per kept id in l order."""
    B, F, L = ids.shape
    out = np.zeros((B, F, W.shape[1]), np.float32)
    for b in range(B):
        for f in range(F):
            acc = np.zeros(W.shape[1], np.float32)
            for l in range(L):
                i = ids[b, f, l]
                if i != padding_idx and 0 <= i < W.shape[0]:
                    acc = acc + W[i]
            out[b, f] = acc
    return out.reshape(B, -1)


@pytest.mark.parametrize("name", sorted(POOL_CASES))
def test_field_sumpool(engine_lib, name):
    from paddlerec_amd import ops
    B, L, D, pad, wpad = POOL_CASES[name]
    rng = np.random.default_rng(sorted(POOL_CASES).index(name))
    W = rng.standard_normal((N_ROWS, D)).astype(np.float32)
    W[3] = -0.0                                                  # -0 + +0 = +0: the sum starts from +0
    Wbuf = torch.full((N_ROWS, D + wpad), NAN, dtype=torch.float32, device=DEV)
    Wbuf[:, :D] = torch.as_tensor(W).to(DEV)
    Wv = Wbuf[:, :D]
    ids = rng.integers(1, N_ROWS, (B, FIELDS, L)).astype(np.int64)
    ids[rng.random(ids.shape) < 0.3] = 0                         # padding
    ids[0, 1, :] = 0                                             # an all-padding field
    ids[0, 2, 0] = 3
    clean = ids.copy()
    ids[0, 0, 0], ids[B - 1, 2, L - 1] = -1, N_ROWS              # out of range on both sides
    if B > 1:
        ids[1, 0, :] = 2 ** 40                                   # a whole field out of range, far out
    for case, want_flag in ((ids, 1), (clean, 0)):
        outs = []
        for _ in range(2):
            buf = torch.full((B, FIELDS * D + pad), NAN, dtype=torch.float32, device=DEV)
            out = buf[:, :FIELDS * D]
            got, status = ops.field_sumpool_fwd(torch.as_tensor(case).to(DEV), Wv, 0, out=out)
            assert got.data_ptr() == out.data_ptr() and int(status.item()) == want_flag
            assert pad == 0 or bool(torch.isnan(buf[:, FIELDS * D:]).all())          # the guard columns stay NaN
            outs.append(out.clone())
        assert torch.equal(outs[0], outs[1])
        want = _pool_loop(W, case, 0)
        assert np.array_equal(outs[0].cpu().numpy().view(np.uint32), want.view(np.uint32)), name   # bit-equal, signs of zero too
    assert not outs[0][0, D:2 * D].any()
    if B > 1:                                                    # the out-of-range rows contributed zero
        flagged = ops.field_sumpool_fwd(torch.as_tensor(ids).to(DEV), Wv, 0)[0]
        assert not flagged[1, :D].any() and not torch.isnan(flagged).any()
    # padding_idx None: id 0 is a row like any other
    got, status = ops.field_sumpool_fwd(torch.as_tensor(clean).to(DEV), Wv, None)
    assert int(status.item()) == 0 and np.array_equal(got.cpu().numpy().view(np.uint32), _pool_loop(W, clean, -1).view(np.uint32))
    assert got.is_contiguous() and tuple(got.shape) == (B, FIELDS * D)


def test_field_sumpool_unaligned_out_takes_the_scalar_form(engine_lib):
    """D and the row stride are multiples of 4 but `out` starts 4 bytes past a 16-byte boundary: float4 stores would be
    misaligned, the entry point must pick the scalar kernel — the same chains, bit-identical to the aligned run."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(5)
    B, L, D = 9, 3, 12
    W = torch.as_tensor(rng.standard_normal((N_ROWS, D)).astype(np.float32)).to(DEV)
    ids = torch.as_tensor(rng.integers(0, N_ROWS, (B, FIELDS, L)).astype(np.int64)).to(DEV)
    buf = torch.full((B, FIELDS * D + 4), NAN, dtype=torch.float32, device=DEV)
    out = buf[:, 1:1 + FIELDS * D]
    assert out.data_ptr() % 16 == 4 and out.stride(0) % 4 == 0
    ops.field_sumpool_fwd(ids, W, 0, out=out)
    assert bool(torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, -3:]).all())
    assert torch.equal(out, ops.field_sumpool_fwd(ids, W, 0)[0])


def _close(got, ref64, ref32, what):
    e, b = R.relerr(got.cpu().numpy(), ref64), K.bound_of(ref32, ref64)
    print("%-40s err %.3g  float32-ref err %.3g" % (what, e, b / 8))
    assert e <= b, (what, e, b)


@pytest.mark.parametrize("clicks", ["mixed", "none"])
@pytest.mark.parametrize("mode", ["ESMM", "IPW", "DR"])
@pytest.mark.parametrize("B,pad", [(1, 0), (5, 0), (1025, 0), (5, 3)])
def test_esm_head(engine_lib, B, pad, mode, clicks):
    from paddlerec_amd import ops
    G = 3 if mode == "DR" else 2
    gw, cw = (1.0, 0.0) if mode == "ESMM" else (0.5, 0.3)
    rng = np.random.default_rng(B + G)
    logits = (3 * rng.standard_normal((B, 2 * G))).astype(np.float32)
    click = rng.integers(0, 2, B).astype(np.int64)
    logits[0, :2] = (40.0, -40.0)              # pCTR below 1e-15: clipped (no gradient), the 1e-6 floors, IPS at its +15 clip
    click[0] = 1
    if B > 1:
        logits[1, :2] = (-40.0, 40.0)          # pCTR = 1 in float32: the clip's upper bound, the gradient passes
        logits[2, 2:4] = (40.0, -40.0)         # pCVR clipped
        logits[3, 2:4] = (-40.0, 40.0)
        click[1:4] = (0, 1, 1)
        if G == 3:
            logits[4, 4:6], logits[2, 4:6] = (40.0, -40.0), (-40.0, 40.0)
    if clicks == "none":
        click[:] = 0                           # N_click = 0: the IPW propensity sits on its floor for every sample
    buy = (click & rng.integers(0, 2, B)).astype(np.int64)
    if B > 1 and clicks == "mixed":
        buy[2:4] = (1, 0)
    buf = torch.full((B, 2 * G + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :2 * G] = torch.as_tensor(logits).to(DEV)
    Lv, cl, bu = buf[:, :2 * G], torch.as_tensor(click).to(DEV), torch.as_tensor(buy).to(DEV)
    for scale in (1.0, 1.0 / B):
        ref = {dt: R.head(logits, click, buy, mode, gw, cw, scale, dtype=dt) for dt in (np.float64, np.float32)}
        count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        a = ops.esm_head(Lv, cl, bu, mode, gw, cw, scale, click_count=count)
        b = ops.esm_head(Lv, cl, bu, mode, gw, cw, scale)
        assert int(count.item()) == int(click.sum())
        for x, y in zip(a, b):
            assert torch.equal(x, y)                                           # a second run is bit-identical
        assert tuple(a[0].shape) == (B, 2 * G + 2) and tuple(a[1].shape) == (B, 3) and tuple(a[2].shape) == (B, 2 * G)
        for i, what in enumerate(("pred", "cost", "dlogits")):
            _close(a[i], ref[np.float64][i], ref[np.float32][i], "head %s B%d %s %s" % (mode, B, clicks, what))
        assert torch.equal(a[2][:, 0::2], -a[2][:, 1::2])                       # d z0 = -d z1 exactly, every task
        assert not torch.isnan(torch.cat(a, 1)).any()
        if mode == "ESMM":
            assert not a[1][:, 1].any() and float(a[0][0, 1]) < 1e-30           # no counterfactual term, no clip
        else:
            assert float(a[0][0, 1]) == float(np.float32(1e-15)) and not a[2][0, :2].any()    # clipped: no gradient
            if B > 1:
                assert float(a[0][1, 1]) == 1.0 and not a[2][2, 2:4].any()
        if mode == "IPW" and clicks == "none":
            assert not a[1][:, 1].any()                                        # o = 0 everywhere
    pred, cost, none = ops.esm_head(Lv, cl, bu, mode, gw, cw, 1.0 / B, want_grad=False)         # dlogits = NULL
    assert none is None and torch.equal(pred, a[0]) and torch.equal(cost, a[1])


def test_refusals_return_before_any_launch(engine_lib):
    import test_esm_abi as A
    A.test_field_sumpool_refusals_without_gpu(engine_lib)
    A.test_esm_head_refusals_without_gpu(engine_lib)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", K.FIXTURES["esmm"] + K.FIXTURES["escm2"])
def test_both_recorded_steps_on_every_golden(engine_lib, name):
    G = K.gold(name)
    m = K.layer_of(G, DEV, None)
    K.check_layer(G, m, "gpu " + name)
    # bit-identical on a rerun from the same state
    m2 = K.layer_of(G, DEV, None)
    m2.set_dict(G["p"])
    for s in range(G["steps"]):
        m2.train_step(*K.feeds(G, s, DEV), G["lr"])
    for key, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[key]), key


@pytest.mark.parametrize("model,mode", [("esmm", None), ("escm2", "DR"), ("escm2", "IPW")])
def test_one_train_step_at_the_shipped_config_sizes(engine_lib, tmp_path, model, mode):
    """esmm/config.yaml and escm2/config.yaml: 737946 x 12 table, 23 fields, max_len 3, towers [256, 64] / 8 experts of 16."""
    from paddlerec_amd import trainer
    torch.manual_seed(1)
    cfg = K.aliccp_config(tmp_path, model, mode=mode or "DR", sparse_feature_number=737946)
    dm = trainer._dygraph_model(model)
    m = dm.create_model(cfg, DEV)
    N, B = 737946, 64
    assert tuple(m.emb.weight.shape) == (N, 12)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(1, N, (B, 23, 3), generator=g)
    ids[torch.rand(B, 23, 3, generator=g) < 0.5] = 0
    click = torch.randint(0, 2, (B,), generator=g)
    buy = click & torch.randint(0, 2, (B,), generator=g)
    before = m.emb.weight.clone()
    metrics, names = dm.create_metrics(DEV)
    loss, metrics, _ = dm.train_forward(m, metrics, (ids, click, buy), cfg)
    assert names == (["auc_ctr", "auc_ctcvr"] if model == "esmm" else ["auc_ctr", "auc_cvr", "auc_ctcvr"])
    assert np.isfinite(loss.item()) and int(m.status.item()) == 0
    touched = torch.unique(ids[ids > 0]).to(DEV)
    assert not torch.equal(before, m.emb.weight) and (before[touched] != m.emb.weight[touched]).any(1).float().mean() > 0.9
    assert not m.emb.weight[0].any() and not torch.isnan(m.emb.weight).any()
    for mt in metrics:
        assert int(mt[0].sum() + mt[1].sum()) == B


@pytest.mark.parametrize("model", ["esmm", "escm2"])
def test_trainer_trains_and_infers_on_the_sample(engine_lib, tmp_path, model):
    from paddlerec_amd import trainer
    cfg = K.aliccp_config(tmp_path, model)
    out, m = trainer.train(cfg, model, device=DEV)
    res = trainer.infer(cfg, model, device=DEV)
    assert len(out) == 2 and out[1]["batches"] == 2 and np.isfinite(out[1]["loss"]) and m.step_count == 4
    assert [r["epoch"] for r in res] == [0, 1] and res[1]["samples"] == 4
    for n in (["auc_ctr", "auc_ctcvr"] if model == "esmm" else ["auc_ctr", "auc_cvr", "auc_ctcvr"]):
        assert 0.0 <= out[1][n] <= 1.0 and 0.0 <= res[1][n] <= 1.0
