"""FAT-DeepFFM on the HIP kernels (csrc/fatffm_ops.hip): the four operators directly against the float64 restatement
(tests/fat_deepffm_ref.py), then the layer, the Adam trajectory and the trainer loops of tests/test_fat_deepffm.py on the
GPU, then one step at the reference's config.yaml sizes.

Tolerances.  Every error is taken relative to the reference tensor's own max-abs.  The yardstick is what float32
arithmetic itself costs the reference:
  * direct operator tests (no GEMM): the restatement is run a second time in float32 NumPy next to the float64 one, and
    the kernel may be off by OP_MULT = 8 times the error of that float32 run, per tensor and per case.  The margin is for
    the summation order (a thread's strided partial sums, a wave butterfly, per-block partials folded in block order
    against NumPy's pairwise sums) and for fused multiply-adds; both runs round every product to float32.
  * the layer against the fixture: the fixture IS the reference's float32 CPU execution; its error against the float64
    restatement, measured per tensor on the CPU (REF_ERR below; 8.6e-8 for pred up to 7.4e-7 for dnn.linear_1.bias), times
    LAYER_MULT = 16: the factor 8 above and 2 for the bf16 x 3 GEMMs, whose error is 2.3e-7 of sum |a||b| where an exact
    float32 GEMM has 1.1e-7.  The largest bound is 1.2e-5 of a tensor's scale, the smallest 8e-7.
"""
import numpy as np
import pytest
import torch

import fat_deepffm_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP_MULT = 8.0
LAYER_MULT = 16.0
# max |fixture - float64 restatement| / max |float64 restatement| per tensor, measured on the CPU
REF_ERR = {"pred": 8.61e-08, "loss": 5.02e-08, "bias": 5.88e-07, "cen.dense_w": 3.73e-07, "cen.embedding.weight": 2.50e-07,
           "cen.fc.AdditionLinear.bias": 1.70e-07, "cen.fc.AdditionLinear.weight": 3.25e-07,
           "cen.fc.ReductionLinear.bias": 2.58e-07, "cen.fc.ReductionLinear.weight": 2.86e-07,
           "dnn.linear_0.bias": 5.31e-07, "dnn.linear_0.weight": 3.90e-07, "dnn.linear_1.bias": 7.39e-07,
           "dnn.linear_1.weight": 5.92e-07, "dnn.linear_2.bias": 5.88e-07, "dnn.linear_2.weight": 4.97e-07}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _ru4(x):
    return (x + 3) // 4 * 4


def _problem(S, Dn, D, B, seed, N=40, stride=None):
    """Inputs of order 1 (H and d_a are products of four of them).  The pad columns of a padded table hold NaN: the
    kernels may load them, they may not use them."""
    rng = np.random.default_rng(seed)
    F = S + Dn
    R, F2, PD = F * D, F * F, F * (F - 1) // 2 * D
    stride = stride or _ru4(R)
    W = np.full((N, stride), np.nan, np.float32)
    W[:, :R] = rng.normal(0, 1, (N, R))
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    if B:
        ids[0, 0] = 0
    return dict(S=S, Dn=Dn, D=D, B=B, F=F, R=R, F2=F2, PD=PD, W=W, ids=ids,
                dense=rng.uniform(-1, 1, (B, Dn)).astype(np.float32),
                dense_w=rng.normal(0, 1, (Dn, R)).astype(np.float32),
                a=np.maximum(rng.normal(0, 1, (B, F2)), 0).astype(np.float32),          # a ReLU's output: half zeros
                dH=rng.normal(0, 1, (B, PD)).astype(np.float32), dz=rng.normal(0, 1, B).astype(np.float32),
                d_pooled=rng.normal(0, 1, (B, F2)).astype(np.float32))


def _mat(B, cols, ld, values=None):
    """A [B, cols] view of a NaN-filled [B, ld] buffer (+ the buffer)."""
    buf = torch.full((B, ld), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[:, :cols]
    if values is not None:
        view.copy_(_t(values))
    return view, buf


def _run(q, pad_ld, grad_stride=None, status=None):
    """The four operators -> numpy outputs; with pad_ld the matrices have leading dimensions rounded up to 4, and what
    lies between the rows must come back untouched."""
    from paddlerec_amd import ops
    B, F2, PD, D = q["B"], q["F2"], q["PD"], q["D"]
    lda, ldh = (_ru4(F2), _ru4(PD)) if pad_ld else (F2, PD)
    ids, dense, W, dw = _t(q["ids"]), _t(q["dense"]), _t(q["W"]), _t(q["dense_w"])
    st = status if status is not None else ops.new_status(DEV)
    pooled, pooled_b = _mat(B, F2, lda)
    a, _ = _mat(B, F2, lda, q["a"])
    H, H_b = _mat(B, PD, ldh)
    dH, _ = _mat(B, PD, ldh, q["dH"])
    d_a, d_a_b = _mat(B, F2, lda)
    d_pooled, _ = _mat(B, F2, lda, q["d_pooled"])
    dz = _t(q["dz"])
    ops.fatffm_pool_fwd(ids, dense, W, dw, D, st, out=pooled)
    _, y1, _ = ops.fatffm_inter_fwd(ids, dense, W, dw, a, D, st, out=(H, None))
    ops.fatffm_attn_bwd(ids, dense, W, dw, a, dH, dz, D, st, out=d_a)
    rg, ddw, _ = ops.fatffm_bwd(ids, dense, W, dw, a, dH, dz, d_pooled, D, ops.Workspace(DEV), status=st,
                                grad_stride=grad_stride)
    torch.cuda.synchronize()
    for view, buf in ((pooled, pooled_b), (H, H_b), (d_a, d_a_b)):
        assert bool(torch.isnan(buf[:, view.shape[1]:]).all()), "floats between the rows were written"
    out = dict(pooled=pooled, H=H, y1=y1, d_a=d_a, row_grad=rg, d_dense_w=ddw)
    return {k: v.cpu().numpy() for k, v in out.items()}, int(st.item())


def _expect(q, dtype, grad_stride=None):
    E = FR.cube(q["ids"], q["dense"], q["W"][:, :q["R"]], q["dense_w"], q["D"], dtype)
    H, y1 = FR.inter(E, q["a"])
    rg, ddw = FR.rows_grads(FR.cube_bwd(E, q["a"], q["dH"], q["dz"], q["d_pooled"]), q["dense"], q["S"],
                            grad_stride or _ru4(q["R"]))
    return dict(pooled=FR.pool(E)[0], H=H, y1=y1.reshape(-1, 1), d_a=FR.attn_bwd(E, q["a"], q["dH"], q["dz"]), row_grad=rg,
                d_dense_w=ddw)


def _close(got, want64, want32, mult, name):
    """|got - want64| <= mult x the error of the float32 run of the reference, both relative to max |want64|."""
    want64 = np.asarray(want64, np.float64)
    got = np.asarray(got, np.float64).reshape(want64.shape)
    if want64.size == 0:
        return
    scale = float(np.abs(want64).max())
    floor = float(np.abs(np.asarray(want32, np.float64).reshape(want64.shape) - want64).max())
    err = float(np.abs(got - want64).max())
    print("%-12s err %.3e  float32 reference %.3e  (of scale %.3e: %.2e / %.2e)" % (
        name, err, floor, scale, err / max(scale, 1e-300), floor / max(scale, 1e-300)))
    assert err <= mult * floor, "%s: max err %.3e > %g x the float32 reference's %.3e (scale %.3e)" % (
        name, err, mult, floor, scale)


def _check(q, pad_ld, grad_stride=None):
    got, st = _run(q, pad_ld, grad_stride)
    assert st == 0
    w64, w32 = _expect(q, np.float64, grad_stride), _expect(q, np.float32, grad_stride)
    for k in ("pooled", "H", "y1", "d_a", "row_grad", "d_dense_w"):
        _close(got[k], w64[k], w32[k], OP_MULT, k)
    assert not got["row_grad"][:, q["R"]:].any(), "pad columns of row_grad must be written 0"
    return got


SHAPES = [  # S, Dn, D, B, table stride
    (1, 1, 1, 1, None),         # F 2, one pair
    (3, 0, 4, 5, None),         # no dense fields
    (6, 3, 9, 10, 81),          # R 81 at table stride 81: scalar staging
    (6, 3, 9, 10, 84),          # the same at stride 84: float4 staging
    (3, 2, 4, 1000, None),      # more samples than blocks, uneven chunks
    (26, 13, 10, 3, None),      # the reference shape, LDS path
    (26, 13, 16, 2, None),      # 97 KB cube: the table path
    (40, 24, 2, 2, None),       # F 64
]


@pytest.mark.parametrize("pad_ld", [False, True])
@pytest.mark.parametrize("S,Dn,D,B,stride", SHAPES)
def test_fatffm_ops_match_restatement(engine_lib, S, Dn, D, B, stride, pad_ld):
    _check(_problem(S, Dn, D, B, seed=S * 1000 + D * 10 + B, stride=stride), pad_ld)


def test_fatffm_empty_batch(engine_lib):
    got, st = _run(_problem(6, 3, 9, 0, seed=1), False)
    assert st == 0 and got["pooled"].shape == (0, 81) and got["H"].size == 0 and got["row_grad"].shape == (0, 84)


def test_fatffm_ties_go_to_the_first_index(engine_lib):
    """A constant dense_w row (every slice of that field ties, whatever the dense value's sign), a dense value of 0 (a row
    of +0 / -0) and a table row with two equal maxima planted in one slice: with a = 0, dz = 0 and dH = 0 the cube's
    gradient is d_pooled on the argmax alone, so row_grad and d_dense_w show where it was put."""
    q = _problem(2, 2, 4, 2, seed=5, N=5)
    F, D, S = 4, 4, 2
    q["ids"][:] = [[1, 2], [2, 1]]
    q["W"][1, 4:8] = [0.3, 0.9, 0.9, 0.1]                    # slice (i, 1) of the field that holds row 1: maxima at d 1, 2
    q["W"][2, 0:4] = -1.0                                    # four equal negative values
    q["dense_w"][0, :] = 1.0
    q["dense"][:] = [[0.7, 0.0], [-0.5, 0.3]]
    only_pool = dict(q, a=np.zeros_like(q["a"]), dz=np.zeros_like(q["dz"]), dH=np.zeros_like(q["dH"]))
    got, st = _run(only_pool, False)
    assert st == 0
    E = FR.cube(q["ids"], q["dense"], q["W"][:, :16], q["dense_w"], D, np.float32)
    am = E.argmax(axis=3)                                    # first index among equal maxima
    assert am[0, 0, 1] == 1 and (am[:, 2] == 0).all() and (am[0, 3] == 0).all() and am[1, 0, 0] == 0
    assert ((E == E.max(axis=3, keepdims=True)).sum(axis=3) > 1).sum() >= 14
    dE = np.zeros((2, F, F, D), np.float32)
    np.put_along_axis(dE, am[..., None], q["d_pooled"].reshape(2, F, F, 1), 3)
    assert np.array_equal(got["row_grad"], dE[:, :S].reshape(2 * S, F * D))
    want_dw = np.einsum("bk,bkc->kc", q["dense"].astype(np.float64), dE[:, S:].reshape(2, 2, F * D).astype(np.float64))
    assert np.array_equal(got["d_dense_w"] != 0, want_dw != 0)
    assert not got["d_dense_w"].reshape(2, F, D)[:, :, 1:][:1].any()         # the constant row: index 0 only
    _check(q, True)                                          # and with everything switched on


def test_fatffm_ids_and_pad_columns(engine_lib):
    """Id 0 is a live row; an id outside [0, N) sets the flag and reads as a zero row; row_grad's pad columns are 0 at a
    grad_stride that is no multiple of 4 (scalar stores) and at one that is."""
    q = _problem(6, 3, 9, 12, seed=9, N=7)
    q["ids"][:, 2] = 0
    got = _check(q, True, grad_stride=88)
    assert got["row_grad"].shape == (72, 88) and got["row_grad"][2, :81].any()
    _check(q, False, grad_stride=87)
    bad = dict(q, ids=q["ids"].copy())
    bad["ids"][1, 0], bad["ids"][5, 5], bad["ids"][7, 3] = -1, 7, 10 ** 12
    got, st = _run(bad, True)
    assert st & 1
    w64, w32 = _expect(bad, np.float64), _expect(bad, np.float32)      # FR.cube reads an id outside [0, N) as zeros
    for k in ("pooled", "H", "y1", "d_a", "row_grad", "d_dense_w"):
        _close(got[k], w64[k], w32[k], OP_MULT, k)
    assert not got["pooled"][1, :9].any() and not got["pooled"][5, 45:54].any()


def test_fatffm_reruns_are_bit_identical(engine_lib):
    q = _problem(6, 3, 9, 1500, seed=3)
    a, _ = _run(q, True)
    b, _ = _run(q, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(a["d_dense_w"]).max() > 0


def test_fatffm_argument_checks_on_the_device_build(engine_lib):
    import test_fat_deepffm
    test_fat_deepffm.check_entry_points_reject_bad_arguments(engine_lib)
    from paddlerec_amd import _lib, ops
    q = _problem(6, 3, 9, 4, seed=2)
    ids, dense, W, dw = _t(q["ids"]), _t(q["dense"]), _t(q["W"]), _t(q["dense_w"])
    with pytest.raises(_lib.RecError, match="share one leading dimension"):
        ops.fatffm_attn_bwd(ids, dense, W, dw, _t(q["a"]), _t(q["dH"]), _t(q["dz"]), 9, out=_mat(4, 81, 84)[0])
    with pytest.raises(_lib.RecError, match="a must be a float32 device matrix"):
        ops.fatffm_inter_fwd(ids, dense, W, dw, _t(q["a"][:, :80]), 9)
    with pytest.raises(_lib.RecError, match="rc=-2"):
        ops.fatffm_pool_fwd(_t(np.zeros((2, 52), np.int64)), _t(np.zeros((2, 13), np.float32)),
                            torch.zeros(3, 68, device=DEV), torch.zeros(13, 65, device=DEV), 1)


# ------------------------------------------------------------------ the layer and the loops
def test_layer_matches_fixture_gpu(engine_lib):
    import test_fat_deepffm
    test_fat_deepffm.check_layer_on_fixture(DEV, None, {k: LAYER_MULT * v for k, v in REF_ERR.items()})


@pytest.mark.parametrize("lazy", [False, True])
def test_adam_trajectory_gpu(engine_lib, lazy):
    """rel: LAYER_MULT x the largest per-tensor error of the reference's float32 execution (7.39e-7) = 1.2e-5."""
    import test_fat_deepffm
    test_fat_deepffm.check_adam_trajectory(DEV, None, lazy, LAYER_MULT * max(REF_ERR.values()))


def test_dropout_streams_and_l2_gpu(engine_lib):
    import test_fat_deepffm
    test_fat_deepffm.check_dropout_streams(DEV, None, LAYER_MULT * max(REF_ERR.values()))


@pytest.mark.parametrize("lazy", [True, False])
def test_fat_deepffm_trainer_loops_gpu(engine_lib, tmp_path, lazy):
    import test_fat_deepffm
    test_fat_deepffm.run_trainer_loops(tmp_path, "cuda", None, lazy)


# ------------------------------------------------------------------ the reference's own sizes
TABLE_SCALE, DENSE_W_SCALE = 2.0, 0.02


def test_full_size_step(engine_lib):
    """One step at fat_deepffm/config.yaml's sizes (1 000 001 rows x 390, F 39, D 10, tower 7410-1600-1600-1), B 512.

    First with the untouched initialisers: the logit saturates (the 13 dense rows are dense_k * 1.0 over 390 columns and a
    is of order 1), every predict is exactly 1.0 in float32, dz is exactly 0 and the step moves no parameter, as in the
    reference.  Then the table is scaled by TABLE_SCALE = 2 and cen.dense_w by DENSE_W_SCALE = 0.02: with those factors
    the NumPy restatement on the CPU gave logits of 0.08 .. 2.34 (predict 0.52 .. 0.91) over three draws of the
    initialisers and of a batch of 512 (the untouched ones: 85 .. 473; table x 1, dense_w x 0.05: predict up to 0.92;
    table x 3, dense_w x 0.02: up to 0.98), so every predict lies in (0.05, 0.95) with room to spare and the gradients
    are live.  The step is compared with the float64 restatement over the rows the batch touches; the bound is
    LAYER_MULT x the error of the restatement's own float32 run, per tensor."""
    from paddlerec_amd.fat_deepffm import FAT_DeepFFMLayer
    N, S, Dn, D, B = 1000001, 26, 13, 10, 512
    R = (S + Dn) * D
    torch.manual_seed(5)
    m = FAT_DeepFFMLayer(N, D, Dn, S, [1600, 1600], device=DEV)
    assert m.emb_table.shape == (N, 392) and m.input_size == 7410
    rng = np.random.default_rng(4)
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    ids[:, 0] = N - 1                                        # the last row: byte offsets past 2^31
    ids[0, 1] = 0
    dense = rng.random((B, Dn), dtype=np.float32)
    label = (rng.random((B, 1)) < 0.4).astype(np.int64)
    rows = np.unique(ids)
    before = m.dense.data.clone()
    rows_before = m.emb_table[_t(rows)].clone()
    loss, pred = m.train_step(_t(ids), _t(dense), _t(label), lr=1e-4)
    assert bool((pred == 1.0).all()) and int(m.status.item()) == 0
    assert torch.equal(m.dense.data, before) and torch.equal(m.emb_table[_t(rows)], rows_before)
    assert not m.dense.grad.any() and not m._last["row_grad"].any()
    assert not m.sparse_state["m"][_t(rows)].any() and not m.dense.m.any()
    # the scaled net
    m.emb_table.mul_(TABLE_SCALE)
    m.dense.p["cen.dense_w"].mul_(DENSE_W_SCALE)
    local = np.searchsorted(rows, ids)
    p = {k: v.detach().cpu().numpy() for k, v in m.dense.p.items()}
    p[FR.EMB] = m.emb_table[_t(rows)].cpu().numpy()[:, :R]
    loss, pred = m.train_step(_t(ids), _t(dense), _t(label), lr=1e-9)
    pred = pred.cpu().numpy()
    assert 0.05 < pred.min() and pred.max() < 0.95, (pred.min(), pred.max())
    o64 = FR.loss_and_grads(local, dense, label, p, D)
    o32 = FR.loss_and_grads(local, dense, label, p, D, dtype=np.float32)
    _close(pred, o64["pred"], o32["pred"], LAYER_MULT, "pred")
    _close(loss.cpu().numpy(), o64["loss"], o32["loss"], LAYER_MULT, "loss")
    gd = m.grad_dict()
    for k in sorted(gd):
        _close(gd[k].cpu().numpy(), o64["g"][k], o32["g"][k], LAYER_MULT, "g " + k)
    rg = m._last["row_grad"].cpu().numpy()
    assert not rg[:, R:].any()
    _close(rg[:, :R], o64["row_grad"], o32["row_grad"], LAYER_MULT, "row_grad")
