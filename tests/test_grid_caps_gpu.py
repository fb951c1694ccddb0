"""Every launch site of paddlerec_amd/csrc that clamps its grid, run past the clamp against float64.

Beyond the clamp a kernel depends on its grid-stride loop: the loop's index arithmetic, its ragged last pass and the fold of its
per-block partials only execute when the problem is larger than cap x work-per-block.  kNumCU = 256, kBlock = 256, kWave = 64.

Every site that `grid > `, `grid = ... ? ... :`, `min(` beside kNumCU, kLossBlocks, kSumsqBlocks, kCtrHeadMaxBlocks, kMaxBlocks and
resident_blocks find in paddlerec_amd/csrc — file:line, function <- exported entry points | work per block x cap | smallest problem with
a second pass | the test that crosses it (no file name: this file; "also": an existing direct kernel test that crosses it too):

  aitm_ops.hip:391       rec_auc_histogram_wide | 256 samples x 2048 blocks | batch > 524 288 | test_auc_histogram_wide_past_cap (N8)
  autofis_ops.hip:430    af_fwd_grid <- rec_autofis_fwd (training) | a chunk of sb <= 4 samples x 2048 | batch > 8192 at sb = 4 |
                         test_autofis_past_cap (8197)
  autofis_ops.hip:555    rec_autofis_fwd (eval) | the same | the same | test_autofis_past_cap
  autofis_ops.hip:637    rec_autofis_bwd (rows kernel) | sb <= 4 samples x 1536 (kAfBwdMaxBlocks) | batch > 6144 | test_autofis_past_cap
  bst_ops.hip:512        stream_grid <- rec_leaky_relu_fwd, rec_leaky_relu_bwd, rec_bst_add, rec_bst_possum_bwd | 256 elements x 4096 |
                         m n > 1 048 576 | test_bst_stream_glue_past_cap (4099 x 257)
  cin_ops.hip:261        rec_cin_outer_fwd, wave kernel (F, S <= 64, S % 4 != 0) | 4 rows x 16384 | B D > 65 536 |
                         test_cin_outer_past_cap[5-2-wave] (B D = 65 556)
  cin_ops.hip:270        rec_cin_outer_fwd, block kernels (float4 / scalar columns) | 1 row x 65536 | B D > 65 536 |
                         test_cin_outer_past_cap[8-4-float4], [8-1-scalar]
  cin_ops.hip:294        rec_cin_outer_bwd, wave kernel (F, S <= 64) | 4 rows x resident blocks (<= 2048) | B D > 8192 |
                         test_cin_outer_past_cap (all three cases: B D = 65 556)
  cin_ops.hip:305        rec_cin_outer_bwd, block kernel | 1 row x resident blocks (<= 2048) | B D > 2048 |
                         test_cin_outer_bwd_block_kernel_past_resident_grid (2053)
  cin_ops.hip:344, 362   rec_cin_contract_fwd, rec_cin_contract_bwd | 4 rows x 8192 | B D > 32 768 | test_cin_contract_past_cap (65 556)
  cross_ops.hip:151, 199 rec_softmax_rows, rec_softmax_rows_bwd | 256 rows x 2048 | m > 524 288 | test_softmax_rows_past_cap (N8; n = 2, 3)
  cross_ops.hip:169      rec_cross_bwd_prep | 256 float4 (or 256 floats) x 2048 | m n / 4 (or m n) > 524 288 |
                         test_cross_bwd_prep_past_cap; also test_cross_layers_gpu.py::test_cross_bwd_prep_grid_stride_loop (4096 x 1560,
                         4099 x 351)
  cross_ops.hip:186      rec_moe_bwd_prep | 4 rows x 2048 | m > 8192 | test_moe_bwd_prep_past_cap (8197 x 5); also
                         test_cross_layers_gpu.py::test_moe_bwd_prep_more_rows_than_one_sweep
  cross_ops.hip:361      rec_dropout | 256 elements x 4096 | rows cols > 1 048 576 | test_dropout_past_cap (4099 x 257)
  cross_ops.hip:372      rec_l2_decay_grad | 256 elements x 4096 | n > 1 048 576 | test_l2_decay_grad_past_cap (N16)
  crossnet_layers.hip:24 add_into <- rec_crossnet_mix_layer_bwd (gbias: n = d; g_gate_w: n = d E; g_gate_b: n = E — parameter sizes,
                         never B d) | 256 elements x 2048 | d > 524 288 | test_crossnet_mix_add_into_past_cap (d = N8, E = 2)
  deepfm_fm.hip:536      fm_fwd_tile_kernel <- rec_deepfm_fm_fwd (emb_dim <= 12, not a multiple of 4) | a tile of 16 samples x resident
                         blocks (<= 2048) | batch > 32 768 | test_deepfm_fm_past_max_blocks[32773-5-tile]
  deepfm_fm.hip:563-566  fm_fwd_kernel <- rec_deepfm_fm_fwd | 4 waves x SPW samples x min(resident, kMaxBlocks = 2048) | batch > 8192
                         at SPW = 1 (emb_dim 64) | test_deepfm_fm_past_max_blocks[8197-64-row-group]
  deepfm_fm.hip:663-665  fm_bwd_tile_kernel <- rec_deepfm_fm_bwd | 16 samples x min(resident, kMaxBlocks) | batch > 32 768 | [32773-5-tile]
  deepfm_fm.hip:695-698  fm_bwd_kernel <- rec_deepfm_fm_bwd, _bwd_sorted | 4 SPW samples x min(resident, kMaxBlocks) | batch > 8192 |
                         [8197-64-row-group]
  din_attention.hip:1609, 1645, 1736, 1752   rec_din_attention_pool_fwd, _bwd (both kernel pairs) | 1 sample (item) x resident blocks
                         (<= 2048) | batch > 2048 | test_din_attention_pool_past_resident_grid (4099)
  dlrm_ops.hip:363, 379  rec_dot_interact_fwd, rec_dot_interact_bwd | 4 samples x 4096 | batch > 16 384 | test_dot_interact_past_cap (16 389)
  fefm_ops.hip:489       fefm_sym <- rec_fefm_fwd, rec_fefm_bwd | 256 elements x 1024 | P D D > 262 144 | test_fefm_sym_past_cap (66 x 64 x 64)
  flen_ops.hip:402       rec_adagrad_dense | 256 elements x 2048 | n > 524 288 | test_adagrad_dense_past_cap (N8)
  gemm_f32.hip:783       launch_glds_cfg <- rec_gemm_f32 (route glds) | 1 tile x 2 blocks per CU (512) | tiles > 512 |
                         test_gemm_gpu.py::test_gemm_glds_kernel[66560-432-400-True] (520 x 3 tiles of 128 x 144; the route is asserted)
  gemm_f32.hip:868       launch_reduce <- rec_gemm_f32 with a K split, rec_gemm_f32_pair | 256 elements x 2048 | M N > 524 288 |
                         test_gemm_splitk_reduce_past_cap (1030 x 510, split_k 2; route asserted).  test_gemm_routes_gpu.py's splitk_*
                         routes stop at 130 x 90.
  gemm_f32.hip:1093      gemv_rows_kernel <- rec_gemm_f32, N <= 4 (route skinny_rows) | 4 rows x 2048 | M > 8192 |
                         test_gemm_routes_gpu.py route skinny_grid_stride (M = 9000; route asserted)
  gemm_f32.hip:1255      rec_mlp_head_bwd | ceil(B / grid) >= 32 consecutive rows x 2048 (no stride loop: the rows per block grow) |
                         batch > 65 536 | test_mlp_head_bwd_at_and_past_cap (65 569: 33 rows a block).  test_gemm_gpu.py stops AT 65 536.
  head_ops.hip:271       rec_sigmoid_logloss | 256 samples x 1024 (kLossBlocks) | batch > 262 144 | test_sigmoid_logloss_at_and_past_cap
  head_ops.hip:284       ctr_head_grid <- rec_ctr_head_fwd_bwd (and the step's head) | 16 samples x 1024 (kCtrHeadMaxBlocks) above batch
                         4096 | batch > 16 384 | test_ctr_head_at_and_past_cap (16 389); also test_ctr_head_gpu.py (65 536 x 400)
  head_ops.hip:351       rec_bce_with_logits | 256 samples x 1024 | batch > 262 144 | test_glue_kernels_gpu.py::test_bce_with_logits[262657]
  head_ops.hip:369       rec_auc_histogram | 16 x 256 samples x 512 | batch > 2 097 152 | test_auc_histogram_at_and_past_cap
  (head_ops.hip:499      rec_fill_uniform: a fixed grid of 2048 blocks | n > 524 288 | test_glue_kernels_gpu.py::test_fill_uniform[524801])
  ps_accessor.hip:466    ps_push_rows_narrow_kernel <- rec_ps_push_rows (no float4 groups, embedx_dim <= 16) | 256 features x 8192 |
                         more than 2 097 152 touched features | test_ps_push_rows_narrow_past_cap
  shard_ops.hip:138      route_keys_kernel <- rec_shard_route | 256 ids x 2048 | n > 524 288 | test_shard_route_past_cap (N8)
  sparse_update.hip:1808 sparse_adam_rows_narrow_kernel <- rec_sparse_adam_rows, _l2 (emb_dim <= 16, no float4 groups) | 256 rows x 8192 |
                         more than 2 097 152 unique rows | test_sparse_adam_rows_narrow_past_cap
  sparse_update.hip:2028 rec_sumsq | 8 x 256 elements x 1024 (kSumsqBlocks) | n > 2 097 152 | test_sumsq_at_and_past_cap; also
                         test_cross_layers_gpu.py::test_sumsq (2^21 + 1, 5 000 003)
  sparse_update.hip:2053 rec_sparse_rows_sumsq | 256 / LANES rows x 1024 | more than 262 144 unique rows at emb_dim 1 |
                         test_sparse_rows_sumsq_at_and_past_cap
  sparse_update.hip:2078 rec_adam_dense | 256 elements x 2048 | n > 524 288 | test_adam_dense_past_cap (N8)
  sparse_update.hip:2315 rec_sgd_dense | 256 elements x 2048 | n > 524 288 | test_glue_kernels_gpu.py::test_sgd_dense[524801-*]
  tisas_ops.hip:647      ts_grid <- rec_tisas_embed_fwd, _bwd (n dim elements) | 256 elements x 2048 | n dim > 524 288 |
                         test_tisas_embed_past_cap; <- rec_tisas_attn_bwd: ts_pos_grad_kernel (seq_len hidden) and ts_time_fold_kernel
                         (2 time_rows hidden) | the same | only with many heads (seq_len <= 128) |
                         test_tisas_attn_bwd_table_gradients_past_cap (128 x 4125, 2 x 64 x 4125)
  w2v_ops.hip:579        w2v_update_short_kernel <- rec_w2v_target_update | 4 unique rows x 2048 | more than 8192 unique target rows |
                         test_w2v_target_update_past_caps (which also passes :582, the long kernel's scan: 1024 rows x 1024 blocks)

Clamps of the same kind that those patterns do NOT find, with no test here: fefm_ops.hip:445 (kFefmGrid), gate_ops.hip:226
(kGateBwdMaxBlocks), flen_ops.hip:280 (kFlenBwdMaxBlocks), the 128 row blocks of the batch-norm column sums (dlrm_ops.hip:227,
autofis_ops.hip:435) and sparse_update.hip:2177 (the dense rider of the small-merge launch).

With them, from the same reading of the first-generation code: test_adam_dense_past_cap is also the SENSITIVE Adam test (non-zero
moments, a device grad_scale, hyper-parameters off their defaults, steps 1 / 2 / 1000 / 100 000, p, m and v);
test_batchnorm_two_pass_variance forces the two-pass variance of rec_batchnorm_fwd / _bwd and the _relu_ pair (x = 1000 + N(0, 1));
rec_transpose_f32, rec_cast_f32_i64 and rec_copy_2d_async, which no test called, are checked bit for bit through _lib.lib().

Tolerance, the project's rule (tests/test_glue_kernels_gpu.py), per tensor: err = max|got - ref64| / max|ref64|, bound
max(8 x the float32 restatement's error on the same inputs, 1e-6); both errors are printed.  A copy, an integer count or ONE
float32 operation must match bit for bit.  Besides the whole tensor the error is taken over the index range the first pass owns,
[0, cap x work), and over [cap x work, n) — a failure says which pass broke; a reduction to one value runs at exactly cap x work
and at n instead.  Inputs are N(0, 1) plus a slow ramp over the flat index (grid_caps_ref.ramped), integer inputs differ between
the two ranges.  Every call runs twice on fresh outputs, bit-identical; every output with a leading dimension is a view of a
NaN-filled wider buffer whose padding must still be NaN afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grid_caps_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32, F64 = np.float32, np.float64
CAP8, CAP16 = 2048 * 256, 4096 * 256              # kNumCU * 8 and kNumCU * 16 blocks of 256 threads, one element each
N8, N16 = CAP8 + 513, CAP16 + 513                 # two full blocks and one ragged thread into the second pass
MAT16 = (4099, 257)                               # rows x cols = 1 053 443 > CAP16 elements, both odd


def _t(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def _close(got, ref64, ref32, what):
    e, r = G.relerr(np.reshape(_n(got), np.shape(ref64)), ref64), G.relerr(ref32, ref64)
    print("%-60s err %.3g  float32-ref err %.3g" % (what, e, r))
    assert e <= max(8 * r, 1e-6), (what, e, r)


def _ranges(first, flat):
    cut = (lambda a: np.reshape(a, -1)) if flat else (lambda a: a)
    return ((" all", lambda a: a), (" pass 1", lambda a: cut(a)[:first]), (" later passes", lambda a: cut(a)[first:]))


def _close_split(got, ref64, ref32, first, what, flat=False):
    """The rule over the whole tensor, over what the first pass of the grid owns and over the rest: rows [0, first) and
    [first, m) of the leading dimension, or (flat) of the flat row-major index."""
    got = np.reshape(_n(got), np.shape(ref64))
    assert 0 < first < (got.size if flat else got.shape[0]), "the shape does not cross the cap"
    for name, f in _ranges(first, flat):
        _close(f(got), f(np.asarray(ref64)), f(np.asarray(ref32)), what + name)


def _exact_split(got, want, first, what, flat=False):
    got = np.reshape(_n(got), np.shape(want))
    assert 0 < first < (got.size if flat else got.shape[0]), "the shape does not cross the cap"
    for name, f in _ranges(first, flat):
        assert np.array_equal(_bits(f(got)), _bits(f(np.asarray(want, got.dtype)))), what + name


def _flat(a):
    """a [n] as a view one float into a NaN-filled buffer of n + 2 -> (view, buffer)."""
    buf = torch.full((a.size + 2,), NAN, dtype=torch.float32, device=DEV)
    buf[1:-1] = _t(a)
    return buf[1:-1], buf


def _flat_ok(buf):
    return bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))


def _strided(a, pad):
    """a [rows, cols] as a view of a wider NaN-filled buffer -> (view, buffer)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _t(a)
    return buf[:, :a.shape[1]], buf


def _out(rows, cols, pad):
    return _strided(np.full((rows, cols), np.nan, F32), pad)


def _pad_is_nan(buf, cols):
    return bool(torch.isnan(buf[:, cols:]).all())


def _twice(run):
    """run() -> a tuple of tensors, evaluated twice on fresh outputs: bit for bit the same -> the first."""
    a, b = run(), run()
    for x, y in zip(a, b):
        if x.is_floating_point():
            x, y = torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)
        assert torch.equal(x, y)
    return a


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------- dense optimizers (cap 2048 blocks)
ADAM = dict(lr=0.1, beta1=0.8, beta2=0.99, eps=1e-6)
ADAM_SCALE = 0.37


@functools.lru_cache(maxsize=None)
def _adam_problem():
    rng = np.random.default_rng(8)
    p, m = 0.1 * G.ramped(rng, N8), 0.05 * G.ramped(rng, N8)
    v, g = (0.02 * G.ramped(rng, N8)) ** 2, 0.1 * G.ramped(rng, N8)
    return _ro(p.astype(F32), m.astype(F32), v.astype(F32), g.astype(F32))


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
def test_adam_dense_past_cap(engine_lib, step):
    """rec_adam_dense at N8 from non-zero moments, hyper-parameters away from their defaults and a device grad_scale other
    than 1; p, m AND v.  The reference (oracle/deepfm_ref.adam_update) gets the float32 hyper-parameters widened to float64,
    not the decimal literals.  An off-by-one step moves p by 18 % at step 1 and 6 % at step 2."""
    from paddlerec_amd import ops
    from oracle import deepfm_ref as R
    p, m, v, g = _adam_problem()
    sc = _t(np.array([ADAM_SCALE], F32))
    g_d = _t(g)

    def run():
        views = [_flat(a) for a in (p, m, v)]
        ops.adam_dense(views[0][0], views[1][0], views[2][0], g_d, step, grad_scale=sc, **ADAM)
        assert all(_flat_ok(b) for _, b in views)
        return tuple(x for x, _ in views)
    got = _twice(run)
    hyper = {k: float(F32(x)) for k, x in ADAM.items()}
    refs = []
    for dt in (F64, F32):
        a = [x.astype(dt) for x in (p, m, v)]
        R.adam_update(a[0], a[1], a[2], g.astype(dt) * dt(F32(ADAM_SCALE)), step, **hyper)
        refs.append(a)
    assert G.relerr(refs[0][0], p) > 1e-3                                          # the update is visible in p
    for name, x, a, b in zip("pmv", got, *refs):
        _close_split(x, a, b, CAP8, "adam_dense step %d %s" % (step, name))


def test_adagrad_dense_past_cap(engine_lib):
    from paddlerec_amd import ops
    rng = np.random.default_rng(9)
    p, acc, g = G.ramped(rng, N8), G.ramped(rng, N8) ** 2, G.ramped(rng, N8)
    lr, eps = 0.05, 1e-6
    g_d = _t(g)

    def run():
        (pv, pb), (av, ab) = _flat(p), _flat(acc)
        ops.adagrad_dense(pv, av, g_d, lr, eps)
        assert _flat_ok(pb) and _flat_ok(ab)
        return pv, av
    gp, ga = _twice(run)
    (p64, a64), (p32, a32) = (G.adagrad_dense(p, acc, g, lr, eps, dt) for dt in (F64, F32))
    _close_split(gp, p64, p32, CAP8, "adagrad_dense p")
    _close_split(ga, a64, a32, CAP8, "adagrad_dense acc")


# -------------------------------------------------------------------------- L2 decay, dropout, BST glue (cap 4096 blocks)
@pytest.mark.parametrize("scaled", [False, True])
def test_l2_decay_grad_past_cap(engine_lib, scaled):
    from paddlerec_amd import ops
    rng = np.random.default_rng(10)
    grad, w = G.ramped(rng, N16), G.ramped(rng, N16)
    coeff, gs = 0.03, (0.7 if scaled else None)
    w_d, gs_d = _t(w), (_t(np.array([gs], F32)) if scaled else None)

    def run():
        gv, gb = _flat(grad)
        ops.l2_decay_grad(gv, w_d, coeff, gs_d)
        assert _flat_ok(gb)
        return (gv,)
    got, = _twice(run)
    r64, r32 = (G.l2_decay_grad(grad, w, coeff, gs, dt) for dt in (F64, F32))
    _close_split(got, r64, r32, CAP16, "l2_decay_grad scaled=%d" % scaled)


@pytest.mark.parametrize("nmask", [1, 2])
def test_dropout_past_cap(engine_lib, nmask):
    """rec_dropout over 4099 x 257 elements with row strides: the mask is oracle/dcn_v2_ref.dropout_keep (the counter-based
    restatement), a kept value ONE float32 product with the scale — mask and values bit for bit."""
    from paddlerec_amd import ops
    from oracle import dcn_v2_ref as X
    rows, cols = MAT16
    rng = np.random.default_rng(11)
    x = G.ramped(rng, rows, cols)
    p, seed, sa, sb = 0.3, 2 ** 63 + 5, 2 ** 40 + 3, 17
    xv, xb = _strided(x, 3)

    def run():
        ov, ob = _out(rows, cols, 2)
        ops.dropout(xv, p, seed, sa, sb if nmask == 2 else None, out=ov)
        assert _pad_is_nan(ob, cols)
        return (ov,)
    got, = _twice(run)
    p32 = float(F32(p))                                                            # the C entry point takes p as float
    keep = X.dropout_keep((rows, cols), p32, seed, sa)
    scale = F32(1) / (F32(1) - F32(p))
    if nmask == 2:
        keep, scale = keep & X.dropout_keep((rows, cols), p32, seed, sb), scale * scale
    want = np.where(keep, x * scale, F32(0)).astype(F32)
    assert 0.2 < 1 - keep[rows // 2:].mean() < (0.6 if nmask == 2 else 0.4)
    _exact_split(got, want, CAP16, "dropout nmask=%d" % nmask, flat=True)
    assert _pad_is_nan(xb, cols)


def test_bst_stream_glue_past_cap(engine_lib):
    """The stream_grid users of bst_ops.hip over 4099 x 257 elements: leaky_relu_fwd / _bwd, bst_add (with and without r) and
    bst_possum_bwd.  Each element is a copy or one float32 operation: bit for bit; dbias is a sum: the rule."""
    from paddlerec_amd import ops
    rows, cols = MAT16
    rng = np.random.default_rng(12)
    x, r = G.ramped(rng, rows, cols) - F32(1), G.ramped(rng, rows, cols)
    slope = 0.01
    (xv, _), (rv, _) = _strided(x, 1), _strided(r, 4)

    def run():
        outs = [_out(rows, cols, k) for k in (2, 3, 5, 6)]
        ops.leaky_relu_fwd(xv, slope, out=outs[0][0])
        ops.leaky_relu_bwd(xv, rv, slope, out=outs[1][0])
        ops.bst_add(xv, rv, out=outs[2][0])
        ops.bst_add(xv, None, out=outs[3][0])
        assert all(_pad_is_nan(b, cols) for _, b in outs)
        return tuple(v for v, _ in outs)
    y, dx, s, c = _twice(run)
    s32 = F32(slope)
    _exact_split(y, np.where(x > 0, x, s32 * x), CAP16, "leaky_relu_fwd", flat=True)
    _exact_split(dx, np.where(x > 0, r, s32 * r), CAP16, "leaky_relu_bwd", flat=True)
    _exact_split(s, x + r, CAP16, "bst_add", flat=True)
    _exact_split(c, x, CAP16, "bst_add copy", flat=True)
    dy = G.ramped(rng, rows)

    def possum():
        dbias = torch.full((1,), NAN, dtype=torch.float32, device=DEV)
        return ops.bst_possum_bwd(_t(dy), cols, dbias), dbias
    dz, dbias = _twice(possum)
    _exact_split(dz, np.repeat(dy, cols), CAP16, "bst_possum_bwd dz", flat=True)
    _close(dbias, [dy.astype(F64).sum()], [dy.sum(dtype=F32)], "bst_possum_bwd dbias")


# --------------------------------------------------------------------------------- CrossNet glue (cross_ops.hip, cap 2048)
@pytest.mark.parametrize("n", [2, 3])
def test_softmax_rows_past_cap(engine_lib, n):
    """One row per thread: m = N8 rows.  The backward starts from the reference's own p."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(13 + n)
    x, dp = G.ramped(rng, N8, n, scale=3.0), G.ramped(rng, N8, n)
    (xv, _), (dpv, _) = _strided(x, 1), _strided(dp, 2)
    f64, f32 = G.softmax_rows(x), G.softmax_rows(x, F32)
    p32 = f64.astype(F32)
    pv, _ = _strided(p32, 3)

    def run():
        (y, yb), (dz, dzb) = _out(N8, n, 2), _out(N8, n, 1)
        ops.softmax_rows(xv, out=y)
        ops.softmax_rows_bwd(pv, dpv, out=dz)
        assert _pad_is_nan(yb, n) and _pad_is_nan(dzb, n)
        return y, dz
    y, dz = _twice(run)
    _close_split(y, f64, f32, CAP8, "softmax_rows n=%d" % n)
    _close_split(dz, G.softmax_rows_bwd(p32, dp), G.softmax_rows_bwd(p32, dp, F32), CAP8, "softmax_rows_bwd n=%d" % n)


@pytest.mark.parametrize("acc", [False, True])
def test_moe_bwd_prep_past_cap(engine_lib, acc):
    """One row per wave, 4 per block: 2048 blocks own 8192 rows."""
    from paddlerec_amd import ops
    m, n, first = 8192 + 5, 5, 2048 * 4
    rng = np.random.default_rng(15)
    dX, X0, U, a0 = (G.ramped(rng, m, n) for _ in range(4))
    prob = G.ramped(rng, m, 2)
    ins = [_strided(a, k + 1)[0] for k, a in enumerate((dX, X0, U))]
    pv = _t(prob)[:, 1]

    def run():
        (dU, dUb), (av, ab) = _out(m, n, 2), (_strided(a0, 3) if acc else _out(m, n, 3))
        dpb = torch.full((m, 2), NAN, dtype=torch.float32, device=DEV)
        ops.moe_bwd_prep(*ins, pv, dU, av, acc, dpb[:, 0])
        assert _pad_is_nan(dUb, n) and _pad_is_nan(ab, n) and _pad_is_nan(dpb, 1)
        return dU, av, dpb[:, 0]
    got = _twice(run)
    r64, r32 = (G.moe_bwd_prep(dX, X0, U, prob[:, 1], a0 if acc else None, dt) for dt in (F64, F32))
    for name, x, a, b in zip(("dU", "dX0_acc", "dp_e"), got, r64, r32):
        _close_split(x, a, b, first, "moe_bwd_prep acc=%d %s" % (acc, name))


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("m,n", [(N8, 4), (174934, 3)])
def test_cross_bwd_prep_past_cap(engine_lib, m, n, acc):
    """float4 path (n = 4, strides multiples of 4): m n / 4 = N8 float4 elements; scalar path (n = 3): m n = CAP8 + 514."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(16 + n)
    dX, X0, U, a0 = (G.ramped(rng, m, n) for _ in range(4))
    pad = 4 if n % 4 == 0 else 1
    ins = [_strided(a, pad * (k + 1))[0] for k, a in enumerate((dX, X0, U))]

    def run():
        (dU, dUb), (av, ab) = _out(m, n, pad), (_strided(a0, 2 * pad) if acc else _out(m, n, 2 * pad))
        ops.cross_bwd_prep(*ins, dU, av, acc)
        assert _pad_is_nan(dUb, n) and _pad_is_nan(ab, n)
        return dU, av
    dU, av = _twice(run)
    r64, r32 = (G.cross_bwd_prep(dX, X0, U, a0 if acc else None, dt) for dt in (F64, F32))
    first = CAP8 * (4 if n % 4 == 0 else 1)
    what = "cross_bwd_prep %s acc=%d " % ((m, n), acc)
    _exact_split(dU, dX * X0, first, what + "dU", flat=True)                       # one float32 product
    _close_split(dU, r64[0], r32[0], first, what + "dU", flat=True)
    _close_split(av, r64[1], r32[1], first, what + "dX0_acc", flat=True)


# --------------------------------------------------------------------------------------------------------------- reductions
SUMSQ_CAP = 1024 * 8 * 256                        # kSumsqBlocks blocks x 8 elements per thread
AUC_CAP = 512 * 16 * 256                          # kNumCU * 2 blocks x 16 elements per thread
LOSS_CAP = 1024 * 256                             # kLossBlocks blocks x one element per thread


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n", [SUMSQ_CAP, SUMSQ_CAP + 513])
def test_sumsq_at_and_past_cap(engine_lib, n, acc):
    from paddlerec_amd import ops
    rng = np.random.default_rng(17)
    x = G.ramped(rng, n)
    ws, x_d, out0 = ops.Workspace(DEV), _t(x), 1234.5

    def run():
        out = torch.full((1,), out0 if acc else NAN, dtype=torch.float32, device=DEV)
        return (ops.sumsq(x_d, out, ws, accumulate=acc),)
    got, = _twice(run)
    _close(got, G.sumsq(x, out0 if acc else None), G.sumsq(x, out0 if acc else None, F32), "sumsq n=%d acc=%d" % (n, acc))


@functools.lru_cache(maxsize=None)
def _auc_problem(B, first):
    """Labels mostly 1 in what the first pass owns and mostly 0 behind it; predictions ramp with the position."""
    rng = np.random.default_rng(B)
    pred = np.clip(0.25 * rng.standard_normal(B) + np.linspace(0.2, 0.8, B), -0.1, 1.1).astype(F32)
    label = ((np.arange(B) < first) ^ (rng.random(B) < 0.2)).astype(np.int64)
    return _ro(pred, label)


@pytest.mark.parametrize("B", [AUC_CAP, AUC_CAP + 513])
def test_auc_histogram_at_and_past_cap(engine_lib, B):
    from paddlerec_amd import ops
    from oracle import deepfm_ref as R
    T = 4095
    pred, label = _auc_problem(B, AUC_CAP // 2)
    p_d, l_d = _t(pred), _t(label)

    def run():
        pos, neg = (torch.zeros(T + 1, dtype=torch.int64, device=DEV) for _ in range(2))
        ops.auc_histogram(p_d, l_d, pos, neg, T)
        return pos, neg
    pos, neg = _twice(run)
    wp, wn = R.auc_histogram(pred, label, T)
    assert np.array_equal(_n(pos), wp) and np.array_equal(_n(neg), wn)
    assert int(wp.sum() + wn.sum()) == B and wp[0] and wp[T]                         # the clamped ends are populated


def test_auc_histogram_wide_past_cap(engine_lib):
    """One element per thread, cap 2048 blocks: batch N8, pred a column of a [B, 3] tensor."""
    from paddlerec_amd import ops
    import aitm_ref as A
    T = 100000
    pred, label = _auc_problem(N8, CAP8)
    buf = torch.full((N8, 3), NAN, dtype=torch.float32, device=DEV)
    buf[:, 1] = _t(pred)
    l_d = _t(label)

    def run():
        pos, neg = (torch.zeros(T + 1, dtype=torch.int64, device=DEV) for _ in range(2))
        ops.auc_histogram_wide(buf[:, 1], l_d, pos, neg, T)
        return pos, neg
    pos, neg = _twice(run)
    wp, wn = A.auc_histogram(pred, label, T)
    assert np.array_equal(_n(pos), wp) and np.array_equal(_n(neg), wn)
    # the same counts from the two ranges alone: which pass lost or repeated a sample
    for name, sl in (("pass 1", slice(0, CAP8)), ("later passes", slice(CAP8, None))):
        pos, neg = (torch.zeros(T + 1, dtype=torch.int64, device=DEV) for _ in range(2))
        ops.auc_histogram_wide(buf[sl, 1], l_d[sl].contiguous(), pos, neg, T)
        wp, wn = A.auc_histogram(pred[sl], label[sl], T)
        assert np.array_equal(_n(pos), wp) and np.array_equal(_n(neg), wn), name


@pytest.mark.parametrize("B", [LOSS_CAP, LOSS_CAP + 513])
def test_sigmoid_logloss_at_and_past_cap(engine_lib, B):
    from paddlerec_amd import ops
    rng = np.random.default_rng(B)
    y1, y2, y3 = (G.ramped(rng, B, 1) - F32(1) for _ in range(3))
    label = ((np.arange(B) < LOSS_CAP // 2) ^ (rng.random(B) < 0.3)).astype(np.int64).reshape(B, 1)
    ws, eps = ops.Workspace(DEV), 1e-4
    ins = [_t(a) for a in (y1, y2, y3, label)]
    pred, dz, loss = _twice(lambda: ops.sigmoid_logloss(*ins, ws, eps=eps))
    r64, r32 = (G.sigmoid_logloss(y1, y2, y3, label, eps, 0, dt) for dt in (F64, F32))
    what = "sigmoid_logloss B=%d " % B
    if B > LOSS_CAP:
        _close_split(pred, r64[0], r32[0], LOSS_CAP, what + "pred", flat=True)
        _close_split(dz, r64[1], r32[1], LOSS_CAP, what + "dz", flat=True)
    else:
        _close(pred, r64[0], r32[0], what + "pred")
        _close(dz, r64[1], r32[1], what + "dz")
    _close(loss, r64[2], r32[2], what + "loss")


# ------------------------------------------------------------------------------------------------------ rec_shard_route
def test_shard_route_past_cap(engine_lib):
    """route_keys_kernel, one id per thread, cap 2048 blocks: N8 ids on 3 shards; ids of the first pass are even rows or
    padding, the ones behind it odd rows — every output equals oracle/shard_ref.shard_route."""
    from paddlerec_amd import ops
    from oracle import shard_ref as S
    G_, N = 3, 1 << 20
    rng = np.random.default_rng(18)
    ids = (2 * rng.integers(1, N // 2, N8) + (np.arange(N8) >= CAP8)).astype(np.int64)
    ids[::97] = 0                                                                    # padding
    ids = ids.reshape(N8, 1)
    want = S.shard_route(ids, G_, padding_idx=0)
    ws, ids_d = ops.Workspace(DEV), _t(ids)

    k = len(want["send_pos"])                                                        # what lies behind it is not written

    def run():
        route, status = ops.shard_route(ids_d, N, 0, G_, ws)
        assert int(status.item()) == 0
        return route.send_local_row[:k], route.send_pos[:k], route.send_sample[:k], route.slot_of_pos, route.send_counts
    got = _twice(run)
    assert np.array_equal(_n(got[4]), want["send_counts"]) and k == int(want["send_counts"][:G_].sum())
    for name, x in zip(("send_local_row", "send_pos", "send_sample"), got):
        assert np.array_equal(_n(x), want[name]), name
    _exact_split(got[3], want["slot_of_pos"], CAP8, "slot_of_pos")


# ------------------------------------------------------------------------------------------------ helpers of head_ops.hip
REC_OK, REC_EINVAL, REC_ESHAPE = 0, -1, -2             # include/recengine.h


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("rows,cols", [(1, 1), (32, 32), (33, 31), (31, 65), (100, 7)])
def test_transpose_f32(engine_lib, rows, cols):
    rng = np.random.default_rng(rows * 100 + cols)
    bits = rng.integers(0, 2 ** 32, (rows, cols), dtype=np.uint64).astype(np.uint32)   # every bit pattern: a copy
    src = _t(bits.view(np.int32)).view(torch.float32)

    def run():
        buf = torch.full((rows * cols + 2,), NAN, dtype=torch.float32, device=DEV)
        assert engine_lib.rec_transpose_f32(rows, cols, _ptr(src), _ptr(buf[1:]), _stream()) == REC_OK
        assert _flat_ok(buf)
        return (buf[1:-1].view(torch.int32),)
    got, = _twice(run)
    assert np.array_equal(_n(got).view(np.uint32).reshape(cols, rows), bits.T)


def test_transpose_f32_edges(engine_lib):
    out = torch.full((4,), NAN, dtype=torch.float32, device=DEV)
    for r, c in ((0, 5), (5, 0), (0, 0)):
        assert engine_lib.rec_transpose_f32(r, c, None, _ptr(out), _stream()) == REC_OK
    assert engine_lib.rec_transpose_f32(-1, 2, _ptr(out), _ptr(out), _stream()) == REC_ESHAPE
    assert engine_lib.rec_transpose_f32(2, 2, None, _ptr(out), _stream()) == REC_EINVAL
    assert bool(torch.isnan(out).all())


CAST_VALUES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0 ** 24 + 1, -(2.0 ** 24 + 1), 2.0 ** 24 + 2, 2.0 ** 40, -(2.0 ** 40), 0.0, -0.0,
               3.49, -3.51, 2.0 ** 62]


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n", [1, 256, 257])
def test_cast_f32_i64(engine_lib, n, stride):
    """(int64) llrintf: round half to even; +-(2^24 + 1) is not a float32 (it arrives as 2^24 and 2^24 + 2 is the next one);
    nothing outside the int64 range."""
    rng = np.random.default_rng(n + stride)
    v = (rng.standard_normal(n) * 1000).astype(F32)
    k = min(n, len(CAST_VALUES))
    v[n - k:] = np.array(CAST_VALUES[:k], F32)                                       # the planted values end at the ragged tail
    src = torch.full((n, stride), NAN, dtype=torch.float32, device=DEV)
    src[:, 0] = _t(v)

    def run():
        buf = torch.full((n + 2,), 7777, dtype=torch.int64, device=DEV)
        assert engine_lib.rec_cast_f32_i64(n, _ptr(src), stride, _ptr(buf[1:]), _stream()) == REC_OK
        assert int(buf[0]) == 7777 and int(buf[-1]) == 7777
        return (buf[1:-1],)
    got, = _twice(run)
    want = G.llrintf(v)
    assert np.array_equal(_n(got), want)
    if n >= len(CAST_VALUES):
        assert list(want[n - k:n - k + 6]) == [0, 0, 2, -2, 2, -2] and want[n - k + 9] == 2 ** 40


def test_cast_f32_i64_edges(engine_lib):
    buf = torch.full((4,), 7777, dtype=torch.int64, device=DEV)
    src = torch.ones(4, dtype=torch.float32, device=DEV)
    assert engine_lib.rec_cast_f32_i64(0, None, 1, _ptr(buf), _stream()) == REC_OK
    assert engine_lib.rec_cast_f32_i64(4, _ptr(src), 0, _ptr(buf), _stream()) == REC_EINVAL
    assert engine_lib.rec_cast_f32_i64(-1, _ptr(src), 1, _ptr(buf), _stream()) == REC_EINVAL
    assert engine_lib.rec_cast_f32_i64(4, None, 1, _ptr(buf), _stream()) == REC_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 7777).all())


@pytest.mark.parametrize("rows,width,sp,dp", [(1, 1, 2, 3), (7, 5, 9, 6), (300, 33, 40, 64)])
def test_copy_2d_async(engine_lib, rows, width, sp, dp):
    """Pitches wider than the width on both sides (in floats; the entry point takes bytes): the payload is copied bit for bit,
    the destination's padding stays NaN, the source is unchanged."""
    rng = np.random.default_rng(rows + width)
    bits = rng.integers(0, 2 ** 32, (rows, sp), dtype=np.uint64).astype(np.uint32)
    src = _t(bits.view(np.int32)).view(torch.float32)

    def run():
        dst = torch.full((rows, dp), NAN, dtype=torch.float32, device=DEV)
        assert engine_lib.rec_copy_2d_async(_ptr(dst), dp * 4, _ptr(src), sp * 4, width * 4, rows, _stream()) == REC_OK
        torch.cuda.synchronize()
        assert _pad_is_nan(dst, width)
        return (dst[:, :width].contiguous().view(torch.int32),)
    got, = _twice(run)
    assert np.array_equal(_n(got).view(np.uint32), bits[:, :width])
    assert np.array_equal(_n(src.view(torch.int32)).view(np.uint32), bits)


def test_copy_2d_async_edges(engine_lib):
    dst = torch.full((4, 4), NAN, dtype=torch.float32, device=DEV)
    src = torch.ones(4, 4, dtype=torch.float32, device=DEV)
    call = engine_lib.rec_copy_2d_async
    assert call(_ptr(dst), 16, _ptr(src), 16, 0, 4, _stream()) == REC_OK               # zero width
    assert call(_ptr(dst), 16, _ptr(src), 16, 16, 0, _stream()) == REC_OK              # zero rows
    assert call(None, 0, None, 0, 0, 0, _stream()) == REC_OK                           # ... with nothing to touch
    assert call(_ptr(dst), 8, _ptr(src), 16, 12, 4, _stream()) == REC_ESHAPE           # pitch < width: destination
    assert call(_ptr(dst), 16, _ptr(src), 8, 12, 4, _stream()) == REC_ESHAPE           # ... source
    assert b"pitch < width" in engine_lib.rec_last_error()
    assert call(None, 16, _ptr(src), 16, 16, 4, _stream()) == REC_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())


# ------------------------------------------------------------------------------------- batch norm: the two-pass variance
BN_M, BN_N = 4099, 70                             # 33 row blocks, the last ragged


@functools.lru_cache(maxsize=None)
def _bn_problem():
    """x = 1000 + N(0, 1): E[x^2] - E[x]^2 in float32 is rounding noise of 1e6 (a one-pass variance yields NaN or garbage);
    the two-pass form dlrm_ops.hip documents keeps 3e-6 on invstd."""
    rng = np.random.default_rng(19)
    x = (1000 + rng.standard_normal((BN_M, BN_N))).astype(F32)
    gamma, beta = (1 + 0.3 * rng.standard_normal(BN_N)).astype(F32), rng.standard_normal(BN_N).astype(F32)
    rm, rv = rng.standard_normal(BN_N).astype(F32), (1 + rng.random(BN_N)).astype(F32)
    dy = rng.standard_normal((BN_M, BN_N)).astype(F32)
    return _ro(x, gamma, beta, rm, rv, dy)


@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_two_pass_variance(engine_lib, relu):
    """rec_batchnorm_fwd/_bwd and the _relu_ pair on a column mean of 1000 and deviation 1.  The float32 restatement is the
    two-pass form (oracle/dlrm_ref.batchnorm_forward: mean, then the mean of (x - mean)^2); the backward starts from the
    reference's own statistics rounded to float32."""
    from paddlerec_amd import ops
    from oracle import dlrm_ref as D
    x, gamma, beta, rm, rv, dy = _bn_problem()
    M, N = BN_M, BN_N
    ws = ops.Workspace(DEV)
    (xv, xb), (dyv, _) = _strided(x, 3), _strided(dy, 1)
    g_d, b_d = _t(gamma), _t(beta)
    fwd = ops.batchnorm_relu_fwd if relu else ops.batchnorm_fwd
    refs = []
    for dt in (F64, F32):
        r_m, r_v = rm.astype(dt), rv.astype(dt)
        y, mean, invstd = D.batchnorm_forward(x.astype(dt), gamma.astype(dt), beta.astype(dt), r_m, r_v, True,
                                              float(F32(0.9)), float(F32(1e-5)))
        refs.append((np.maximum(y, 0) if relu else y, mean, invstd, r_m, r_v))

    def run():
        yv, yb = _out(M, N, 5)
        trm, trv = _t(rm), _t(rv)
        y, sm, si = fwd(xv, g_d, b_d, trm, trv, ws, True, out=yv)
        assert _pad_is_nan(yb, N)
        return y, sm, si, trm, trv
    got = _twice(run)
    what = "batchnorm%s fwd " % ("_relu" if relu else "")
    for name, t, a, b in zip(("y", "save_mean", "save_invstd", "running_mean", "running_var"), got, *refs):
        assert bool(torch.isfinite(t).all()), name
        _close(t, a, b, what + name)
    assert _pad_is_nan(xb, N)
    # backward from the reference's statistics
    mean32, inv32 = refs[0][1].astype(F32), refs[0][2].astype(F32)
    y32 = refs[0][0].astype(F32)
    sm, si, yv = _t(mean32), _t(inv32), _strided(y32, 2)[0]
    brefs = []
    for dt in (F64, F32):
        d = dy.astype(dt) * (y32 > 0) if relu else dy.astype(dt)
        brefs.append(D.batchnorm_backward(x.astype(dt), d, gamma.astype(dt), mean32.astype(dt), inv32.astype(dt)))

    def run_bwd():
        dxv, dxb = _out(M, N, 4)
        dg, db = (torch.full((N,), NAN, dtype=torch.float32, device=DEV) for _ in range(2))
        if relu:
            ops.batchnorm_relu_bwd(xv, yv, dyv, g_d, sm, si, ws, dgamma=dg, dbeta=db, out=dxv)
        else:
            ops.batchnorm_bwd(xv, dyv, g_d, sm, si, ws, dgamma=dg, dbeta=db, out=dxv)
        assert _pad_is_nan(dxb, N)
        return dxv, dg, db
    bgot = _twice(run_bwd)
    what = "batchnorm%s bwd " % ("_relu" if relu else "")
    for name, t, a, b in zip(("dx", "dgamma", "dbeta"), bgot, *brefs):
        assert bool(torch.isfinite(t).all()), name
        _close(t, a, b, what + name)


# ------------------------------------------------------------------------------------------------- the heads (head_ops.hip)
def _head_ref(act, w, bias, y1, y2, label, eps, relu, dtype):
    """Linear(n -> 1) + sigmoid + log_loss + mean and their backward: -> pred, dz, loss, dx, dw, db."""
    a, wv = act.astype(dtype), w.astype(dtype).reshape(-1)
    y = (a * wv).sum(axis=1, dtype=dtype) + dtype(bias[0])
    pred, dz, loss = G.sigmoid_logloss(y1, y2, y.astype(F32) if dtype is F32 else y, label, eps, 0, dtype)
    dx = dz[:, None] * wv[None, :]
    if relu:
        dx = dx * (act > 0)
    return pred, dz, loss, dx, (a * dz[:, None]).sum(axis=0, dtype=dtype), np.asarray([dz.sum(dtype=dtype)])


@functools.lru_cache(maxsize=None)
def _head_problem(B, n, first):
    rng = np.random.default_rng(B + n)
    act = np.maximum(G.ramped(rng, B, n) - F32(1), 0)                                 # behind a ReLU: about a third zeros
    w, bias = (rng.standard_normal(n) / np.sqrt(n)).astype(F32), np.array([0.1], F32)
    y1, y2 = (0.3 * (G.ramped(rng, B) - F32(1)) for _ in range(2))
    label = ((np.arange(B) < first // 2) ^ (rng.random(B) < 0.3)).astype(np.int64)
    return _ro(act, w, bias, y1.astype(F32), y2.astype(F32), label)


CTR_CAP = 1024 * 16                               # kCtrHeadMaxBlocks blocks x 4 waves x 4 rows (above batch 4096)


@pytest.mark.parametrize("B", [CTR_CAP, CTR_CAP + 5])
def test_ctr_head_at_and_past_cap(engine_lib, B):
    """rec_ctr_head_fwd_bwd: 16 samples per block above batch 4096, at most 1024 blocks.  A wave walks rows r, r + 4096 per
    trip (two in flight): two trips cover 16384 rows, the third only runs past the cap.  n = 8 (two float4 lanes), row
    strides 12."""
    from paddlerec_amd import ops
    n, eps = 8, 1e-4
    act, w, bias, y1, y2, label = _head_problem(B, n, CTR_CAP)
    ws = ops.Workspace(DEV)
    (av, ab), w_d, b_d = _strided(act, 4), _t(w.reshape(n, 1)), _t(bias)
    y1_d, y2_d, l_d = _t(y1.reshape(B, 1)), _t(y2.reshape(B, 1)), _t(label.reshape(B, 1))

    def run():
        dxv, dxb = _out(B, n, 4)
        pred, dz = (torch.full((B, 1), NAN, dtype=torch.float32, device=DEV) for _ in range(2))
        loss, db = (torch.full((1,), NAN, dtype=torch.float32, device=DEV) for _ in range(2))
        dw = torch.full((n, 1), NAN, dtype=torch.float32, device=DEV)
        ops.ctr_head(av, w_d, b_d, y1_d, y2_d, l_d, ws, dw, db, eps=eps, out=(pred, dz, loss, dxv))
        assert _pad_is_nan(dxb, n)
        return pred, dz, loss, dxv, dw, db
    got = _twice(run)
    r64, r32 = (_head_ref(act, w, bias, y1, y2, label, eps, True, dt) for dt in (F64, F32))
    what = "ctr_head B=%d " % B
    for k, name in enumerate(("pred", "dz", "loss", "dx", "dw", "db")):
        if name in ("pred", "dz", "dx") and B > CTR_CAP:
            _close_split(got[k], r64[k], r32[k], CTR_CAP, what + name)
        else:
            _close(got[k], r64[k], r32[k], what + name)
    assert _pad_is_nan(ab, n)


HEAD_CAP = 2048 * 32                              # kNumCU * 8 blocks x at least 32 rows


@pytest.mark.parametrize("B", [HEAD_CAP, HEAD_CAP + 33])
def test_mlp_head_bwd_at_and_past_cap(engine_lib, B):
    """rec_mlp_head_bwd: a block owns ceil(B / grid) consecutive rows; at 65536 that is 32 on 2048 blocks, at 65536 + 33 it
    is 33 (an odd count for the two row parities) and the last blocks own nothing."""
    from paddlerec_amd import ops
    n = 8
    act, w, bias, y1, y2, label = _head_problem(B, n, HEAD_CAP)
    dz = (y1 / F32(B)).astype(F32)
    ws = ops.Workspace(DEV)
    (av, ab), w_d, dz_d = _strided(act, 4), _t(w.reshape(n, 1)), _t(dz.reshape(B, 1))

    def run():
        dxv, dxb = _out(B, n, 8)
        dw, db = torch.full((n, 1), NAN, dtype=torch.float32, device=DEV), torch.full((1,), NAN, dtype=torch.float32, device=DEV)
        ops.mlp_head_bwd(av, dz_d, w_d, ws, dw, db, relu=True, out=dxv)
        assert _pad_is_nan(dxb, n)
        return dxv, dw, db
    dx, dw, db = _twice(run)
    what = "mlp_head_bwd B=%d " % B
    want_dx = np.where(act > 0, dz[:, None] * w[None, :], F32(0)).astype(F32)          # one float32 product or a zero
    refs = [((act.astype(dt) * dz.astype(dt)[:, None]).sum(axis=0, dtype=dt), np.asarray([dz.sum(dtype=dt)])) for dt in (F64, F32)]
    if B > HEAD_CAP:
        _exact_split(dx, want_dx, HEAD_CAP, what + "dx")
    else:
        assert np.array_equal(_bits(_n(dx)), _bits(want_dx)), what + "dx"
    _close(dw, refs[0][0], refs[1][0], what + "dw")
    _close(db, refs[0][1], refs[1][1], what + "db")
    assert _pad_is_nan(ab, n)


# ------------------------------------------------------------------------------------------------------- DLRM (dlrm_ops.hip)
DOT_CAP = 4096 * 4                                # 16 kNumCU blocks x one sample per wave


@pytest.mark.parametrize("F,D", [(3, 4), (9, 7)])
def test_dot_interact_past_cap(engine_lib, F, D):
    """rec_dot_interact_fwd / _bwd at B = 16384 + 5; (9, 7): an odd LDS pitch and 36 pairs."""
    from paddlerec_amd import ops
    from oracle import dlrm_ref as R
    B, P = DOT_CAP + 5, F * (F - 1) // 2
    rng = np.random.default_rng(F * 10 + D)
    T, dR = G.ramped(rng, B, F, D) - F32(1), G.ramped(rng, B, D + P)
    T_d, (dRv, _) = _t(T), _strided(dR, 3)

    def run():
        Rv, Rb = _out(B, D + P, 2)
        ops.dot_interact_fwd(T_d, out=Rv)
        dT = torch.full((B, F, D), NAN, dtype=torch.float32, device=DEV)
        ops.dot_interact_bwd(T_d, dRv, out=dT)
        assert _pad_is_nan(Rb, D + P)
        return Rv, dT
    Rg, dT = _twice(run)
    what = "dot_interact F=%d D=%d " % (F, D)
    _exact_split(_n(Rg)[:, :D], T[:, F - 1, :], DOT_CAP, what + "x copy")
    _close_split(Rg, R.dot_interact(T.astype(F64)), R.dot_interact(T), DOT_CAP, what + "R")
    _close_split(dT, R.dot_interact_backward(T.astype(F64), dR.astype(F64)), R.dot_interact_backward(T, dR), DOT_CAP, what + "dT")


# -------------------------------------------------------------------------------------------------------- CIN (cin_ops.hip)
CIN_B, CIN_D, CIN_F = 16384 + 5, 4, 3             # B D = 65 556 rows: past 65 536 (outer_fwd) and 32 768 (contract)


@pytest.mark.parametrize("S,ldz_pad,kernel", [(5, 2, "wave"), (8, 4, "float4"), (8, 1, "scalar")])
def test_cin_outer_past_cap(engine_lib, S, ldz_pad, kernel):
    """rec_cin_outer_fwd on its three kernels — one wave per row, capped at 16384 blocks x 4 rows (S % 4 != 0, F and S <= 64);
    one block per row with float4 columns, capped at 65536 blocks (S % 4 == 0, Z 16-byte rows); the same with scalar columns
    (S % 4 == 0 but an odd row stride of Z) — and rec_cin_outer_bwd (F, S <= 64: one wave per row on a grid of resident
    blocks, at most 2048 x 4 rows a pass) on the same shape.  Z is one float32 product per element: bit for bit."""
    from paddlerec_amd import ops
    B, D, F = CIN_B, CIN_D, CIN_F
    rows = B * D
    rng = np.random.default_rng(S + ldz_pad)
    feat, xt = G.ramped(rng, B, F, D + 3) - F32(1), G.ramped(rng, rows, S)
    dZ, dpool, d0 = G.ramped(rng, rows, F * S) - F32(1), G.ramped(rng, B, S), G.ramped(rng, B, F, D)
    tf = _t(feat)[:, :, 1:1 + D]
    feat = feat[:, :, 1:1 + D]
    (xk_t, _), (dZv, _), (dpv, _) = _strided(xt, 4), _strided(dZ, 3), _strided(dpool, 2)
    xk = xt.reshape(B, D, S).transpose(0, 2, 1)                                          # [B, S, D]
    v0, vk = ops.cin_view(tf, "bfd"), ops.cin_view((xk_t, D), "xt")

    def run():
        Zv, Zb = _out(rows, F * S, ldz_pad)
        assert S % 4 != 0 or (Zv.stride(0) % 4 == 0) == (kernel == "float4")
        ops.cin_outer_fwd(B, D, F, S, tf, v0, xk_t, vk, Zv)
        td0 = _t(d0)
        dkv, dkb = _out(rows, S, 3)
        ops.cin_outer_bwd(B, D, F, S, dZv, tf, v0, xk_t, vk, td0, ops.cin_view(td0, "bfd"), True, dkv,
                          ops.cin_view((dkv, D), "xt"), False, dpv)
        assert _pad_is_nan(Zb, F * S) and _pad_is_nan(dkb, S)
        return Zv, td0, dkv
    Z, dX0, dXk = _twice(run)
    what = "cin_outer %s S=%d " % (kernel, S)
    _exact_split(Z, np.einsum("bfd,bsd->bdfs", feat, xk).reshape(rows, F * S), 65536, what + "Z")
    refs = []
    for dt in (F64, F32):
        dz4 = dZ.reshape(B, D, F, S).astype(dt)
        a = np.einsum("bdfs,bsd->bfd", dz4, xk.astype(dt))
        bk = np.einsum("bdfs,bfd->bsd", dz4, feat.astype(dt))
        refs.append((d0.astype(dt) + a, (bk + dpool.astype(dt)[:, :, None]).transpose(0, 2, 1).reshape(rows, S)))
    _close_split(dX0, refs[0][0], refs[1][0], 2048, what + "dX0")                       # samples: 2048 x 4 rows / D
    _close_split(dXk, refs[0][1], refs[1][1], 2048 * 4, what + "dXk")


def test_cin_outer_bwd_block_kernel_past_resident_grid(engine_lib):
    """rec_cin_outer_bwd with F > 64 takes the block-per-row kernel on a grid of resident blocks (at most 8 per CU: 2048):
    B D = 2053 rows."""
    from paddlerec_amd import ops
    B, D, F, S = 2053, 1, 65, 2
    rows = B * D
    rng = np.random.default_rng(65)
    feat, xt = G.ramped(rng, B, F, D) - F32(1), G.ramped(rng, rows, S)
    dZ, d0 = G.ramped(rng, rows, F * S) - F32(1), G.ramped(rng, B, F, D)
    tf, (xk_t, _), (dZv, _) = _t(feat), _strided(xt, 1), _strided(dZ, 3)
    xk = xt.reshape(B, D, S).transpose(0, 2, 1)
    v0, vk = ops.cin_view(tf, "bfd"), ops.cin_view((xk_t, D), "xt")

    def run():
        td0 = _t(d0)
        dkv, dkb = _out(rows, S, 3)
        ops.cin_outer_bwd(B, D, F, S, dZv, tf, v0, xk_t, vk, td0, ops.cin_view(td0, "bfd"), True, dkv,
                          ops.cin_view((dkv, D), "xt"), False, None)
        assert _pad_is_nan(dkb, S)
        return td0, dkv
    dX0, dXk = _twice(run)
    refs = []
    for dt in (F64, F32):
        dz4 = dZ.reshape(B, D, F, S).astype(dt)
        refs.append((d0.astype(dt) + np.einsum("bdfs,bsd->bfd", dz4, xk.astype(dt)),
                     np.einsum("bdfs,bfd->bsd", dz4, feat.astype(dt)).transpose(0, 2, 1).reshape(rows, S)))
    _close_split(dX0, refs[0][0], refs[1][0], 2048, "cin_outer_bwd block kernel dX0")
    _close_split(dXk, refs[0][1], refs[1][1], 2048, "cin_outer_bwd block kernel dXk")


@pytest.mark.parametrize("C", [5, 8])
def test_cin_contract_past_cap(engine_lib, C):
    """rec_cin_contract_fwd / _bwd: one wave per row, at most 32 kNumCU blocks x 4 rows = 32768 rows a pass; B D = 65556 makes
    a second and a (ragged) third."""
    from paddlerec_amd import ops
    B, D, F = CIN_B, CIN_D, CIN_F
    rows, first = B * D, 32768
    rng = np.random.default_rng(C)
    feat, y = G.ramped(rng, B, F, D + 2) - F32(1), G.ramped(rng, rows, C * F) - F32(1)
    g, d0 = G.ramped(rng, rows, C), G.ramped(rng, B, F, D)
    tf = _t(feat)[:, :, 1:1 + D]
    feat = feat[:, :, 1:1 + D]
    (ty, _), (tg, _) = _strided(y, 3), _strided(g, 1)
    v0 = ops.cin_view(tf, "bfd")

    def run():
        (xt, xtb), (dy, dyb) = _out(rows, C, 1), _out(rows, C * F, 2)
        ops.cin_contract_fwd(B, D, F, ty, tf, v0, xt)
        td0 = _t(d0)
        ops.cin_contract_bwd(B, D, F, ty, tg, tf, v0, dy, td0, ops.cin_view(td0, "bfd"), True)
        assert _pad_is_nan(xtb, C) and _pad_is_nan(dyb, C * F)
        return xt, dy, td0
    xt, dy, dX0 = _twice(run)
    what = "cin_contract C=%d " % C
    refs = []
    for dt in (F64, F32):
        y4, g3 = y.reshape(B, D, C, F).astype(dt), g.reshape(B, D, C).astype(dt)
        refs.append((np.einsum("bfd,bdcf->bdc", feat.astype(dt), y4).reshape(rows, C),
                     d0.astype(dt) + np.einsum("bdc,bdcf->bfd", g3, y4)))
    _close_split(xt, refs[0][0], refs[1][0], first, what + "XT")
    _exact_split(dy, np.einsum("bdc,bfd->bdcf", g.reshape(B, D, C), feat).reshape(rows, C * F), first, what + "dY")
    _close_split(dX0, refs[0][1], refs[1][1], first // D, what + "dX0")


# ------------------------------------------------------------------------------------- rec_gemm_f32: the split-K reduce
def test_gemm_splitk_reduce_past_cap(engine_lib):
    """launch_reduce (splitk_reduce_kernel, one element per thread, cap 2048 blocks): M N = 1030 x 510 = 525 300 elements on
    the tiled kernel with split_k = 2 and the bias epilogue, which the reduce applies — the route is asserted.  (The
    small-n row kernel's clamp is crossed by tests/test_gemm_routes_gpu.py, route skinny_grid_stride: M = 9000 > 8192.)"""
    from paddlerec_amd import ops
    M, N, K = 1030, 510, 130
    rng = np.random.default_rng(20)
    A, Bm = G.ramped(rng, M, K) - F32(1), (G.ramped(rng, K, N) - F32(1)) / F32(np.sqrt(K))
    bias = G.ramped(rng, N)
    ws = ops.Workspace(DEV)
    (Av, _), (Bv, _), b_d = _strided(A, 4), _strided(Bm.astype(F32), 2), _t(bias)

    def run():
        Cv, Cb = _out(M, N, 2)
        ops.gemm(Av, Bv, ws, epilogue="bias", bias=b_d, out=Cv, split_k=2)
        route = ops.gemm_last_route()
        assert route.family == "tiled" and route.splits == 2, route
        assert _pad_is_nan(Cb, N)
        return (Cv,)
    got, = _twice(run)
    r64 = A.astype(F64) @ Bm.astype(F64) + bias.astype(F64)
    r32 = A @ Bm.astype(F32) + bias
    _close_split(got, r64, r32, CAP8, "gemm split_k=2 bias", flat=True)


# ------------------------------------------------------------------------------------------------- FEFM: the symmetrised FE
def test_fefm_sym_past_cap(engine_lib):
    """fefm_sym (fefm_ops.hip; one element per thread, cap 4 kNumCU blocks = 262144 elements) symmetrises FE [P, D, D] into the
    workspace for rec_fefm_fwd and rec_fefm_bwd: 12 fields (P = 66 pairs) of dim 64 are 270336 elements, the first pass owns
    the matrices of pairs 0..63 exactly.  Pair p's term t_p = x_i^T (FE_p + FE_p^T) x_j is column S D + p of dnn_in: the pairs
    of the first pass and the two behind it are held to the rule separately."""
    from paddlerec_amd import ops
    import deepfefm_ref as FR
    B, S, D, N = 3, 12, 64, 40
    P, first = S * (S - 1) // 2, 1024 * 256 // (D * D)
    assert P * D * D > 1024 * 256 and first * D * D == 1024 * 256 and first < P
    rng = np.random.default_rng(21)
    p = dict(W=(0.3 * rng.standard_normal((N, D))).astype(F32), W1=(0.1 * rng.standard_normal((N, 1))).astype(F32),
             dense_w_one=np.zeros(0, F32), FE=0.3 * (G.ramped(rng, P, D, D) - F32(1)))
    ids = rng.integers(1, N, (B, S), dtype=np.int64)
    dense = np.zeros((B, 0), F32)
    dz, dd = rng.standard_normal(B).astype(F32), rng.standard_normal((B, S * D + P)).astype(F32)
    W, W1, FE, ids_d, dense_d = _t(p["W"]), _t(p["W1"]), _t(p["FE"]), _t(ids), _t(dense)

    def run():
        ws, st = ops.Workspace(DEV), ops.new_status(DEV)
        buf = torch.full((B, S * D + P + 3), NAN, dtype=torch.float32, device=DEV)
        out = (torch.full((B, 1), NAN, device=DEV), torch.full((B, 1), NAN, device=DEV), buf,
               torch.zeros(B, S, dtype=torch.int64, device=DEV))
        y1, y2, dnn_in, ids_all, _ = ops.fefm_fwd(ids_d, dense_d, W, W1, _t(p["dense_w_one"]), FE, D, ws, status=st, out=out)
        rg, _, dfe = ops.fefm_bwd(ids_all, dense_d, W, FE, _t(dz), _t(dd), S, D, ws, want_d_fe=True, status=st)
        assert int(st.item()) == 0 and _pad_is_nan(buf, S * D + P)
        return y2, buf[:, :S * D + P], rg, dfe
    y2, dnn_in, rg, dfe = _twice(run)
    r64, r32 = (FR.kernel_reference(ids, dense, p, D, dz, dd, dt) for dt in (torch.float64, torch.float32))
    t = lambda a: np.ascontiguousarray(np.asarray(a)[:, S * D:].T)                        # [P, B]: pairs lead
    _close_split(t(_n(dnn_in)), t(r64["dnn_in"]), t(r32["dnn_in"]), first, "fefm pair terms")
    _close(y2, r64["y2"], r32["y2"], "fefm y2")
    _close(_n(rg)[:, :D], r64["row_grad"], r32["row_grad"], "fefm row_grad")
    _close_split(dfe, r64["d_FE"], r32["d_FE"], first, "fefm d_FE")


# ----------------------------------------------------------------------------------------------------------------- AutoFIS
def test_autofis_past_cap(engine_lib):
    """rec_autofis_fwd (training and eval) and rec_autofis_bwd: a block takes chunks of 4 samples (3 fields of dim 2), at most
    8 kNumCU = 2048 chunks a pass forward (8192 samples) and 6 kNumCU = 1536 backward (6144 samples); B = 8192 + 5.  The
    ids of the two ranges come from different halves of the table."""
    from paddlerec_amd import ops
    import autofis_ref as AR
    B, S, D, N, first_f, first_b = 8192 + 5, 3, 2, 50, 8192, 6144
    rng = np.random.default_rng(22)
    cols, rows = AR.generate_pairs(S)
    P = len(cols)
    v, w = rng.uniform(-1, 1, (N, D)).astype(F32), rng.uniform(-1, 1, (N, 1)).astype(F32)
    ids = rng.integers(0, N // 2, (B, S), dtype=np.int64) + (N // 2) * (np.arange(B) >= first_f)[:, None]
    gamma, beta = (1 + 0.2 * rng.standard_normal(P)).astype(F32), (0.1 * rng.standard_normal(P)).astype(F32)
    mask = rng.uniform(0.3, 0.9, P).astype(F32)
    rm0, rv0 = (0.3 * rng.standard_normal(P)).astype(F32), (0.5 + rng.random(P)).astype(F32)
    dz, dx0 = (G.ramped(rng, B) / F32(B)).astype(F32), G.ramped(rng, B, S * D)
    pairs = ops.AutofisPairs(cols, rows, S, DEV)
    ws, status = ops.Workspace(DEV), ops.new_status(DEV)
    V, W1, ids_d, dz_d = _t(v), _t(w), _t(ids), _t(dz)
    g_d, b_d, m_d = _t(gamma), _t(beta), _t(mask)

    def run():
        (x0, xb), (L, lb) = _out(B, S * D, 3), _out(B, P, 1)
        rm, rv = _t(rm0), _t(rv0)
        _, s, _, sm, si, _ = ops.autofis_fwd(ids_d, V, W1, pairs, g_d, b_d, m_d, rm, rv, ws, True, status=status, out=(x0, L))
        dX, db = _strided(dx0, 3)
        _, d_mask, d_gamma, d_beta = ops.autofis_bwd(dz_d, L, x0, pairs, sm, si, g_d, b_d, m_d, dX, ws)
        rm_e, rv_e = _t(rm0), _t(rv0)
        _, s_ev, _, _, _, _ = ops.autofis_fwd(ids_d, V, W1, pairs, g_d, b_d, m_d, rm_e, rv_e, ws, False, status=status)
        assert _pad_is_nan(xb, S * D) and _pad_is_nan(lb, P) and _pad_is_nan(db, S * D) and int(status.item()) == 0
        return x0, s, L, sm, si, rm, rv, dX, d_mask, d_gamma, d_beta, s_ev
    got = dict(zip(("X0", "s", "L", "mean", "invstd", "rm", "rv", "dX", "d_mask", "d_gamma", "d_beta", "s_eval"), _twice(run)))
    refs = []
    for dt in (F64, F32):
        xv, xw = AR.lookup(ids, v, dt)[0], AR.lookup(ids, w, dt)[0][..., 0]
        args = (cols, rows, gamma, beta, mask)
        s, L, mean, var, invstd = AR.pair_forward(xv, xw, *args, dtype=dt)
        dxv, dm, dg, db = AR.pair_backward(xv, L, dz, *args, mean, invstd, dtype=dt)
        mom = dt(F32(0.9))
        refs.append(dict(s=s, L=L, mean=mean, invstd=invstd, rm=mom * rm0.astype(dt) + (1 - mom) * mean,
                         rv=mom * rv0.astype(dt) + (1 - mom) * var, dX=dx0.astype(dt) + dxv.reshape(B, -1), d_mask=dm,
                         d_gamma=dg, d_beta=db, s_eval=AR.pair_forward(xv, xw, *args, rm0, rv0, dtype=dt)[0]))
    _exact_split(got["X0"], v[ids].reshape(B, S * D), first_f, "autofis X0")
    for k in ("s", "L", "s_eval"):
        _close_split(got[k], refs[0][k], refs[1][k], first_f, "autofis " + k)
    _close_split(got["dX"], refs[0]["dX"], refs[1]["dX"], first_b, "autofis dX")
    for k in ("mean", "invstd", "rm", "rv", "d_mask", "d_gamma", "d_beta"):
        _close(got[k], refs[0][k], refs[1][k], "autofis " + k)


# ---------------------------------------------------------------------------------------------- the DeepFM FM block's kernels
@pytest.mark.parametrize("B,D,kernels", [(2048 * 4 + 5, 64, "row-group"), (2048 * 16 + 5, 5, "tile")])
def test_deepfm_fm_past_max_blocks(engine_lib, B, D, kernels):
    """rec_deepfm_fm_fwd / _bwd with kMaxBlocks = 2048 blocks (and the resident grid, at most 8 blocks per CU = 2048).  D = 64:
    the row-group kernels, one sample per wave, 4 per block — 2050 blocks wanted.  D = 5 (not a multiple of 4, at most 12): the
    tile kernels, 16 samples per tile — 2049 tiles.  One slot and one dense field."""
    from paddlerec_amd import ops
    from oracle import deepfm_ref as R
    S, Dn, N, first = 1, 1, 60, B - 5
    rng = np.random.default_rng(D)
    W, W1 = (0.3 * rng.standard_normal((N, D))).astype(F32), (0.1 * rng.standard_normal((N, 1))).astype(F32)
    dense_w, dense_w_one = (0.3 * rng.standard_normal((1, Dn, D))).astype(F32), rng.standard_normal(Dn).astype(F32)
    ids = (rng.integers(1, N // 2, (B, S)) + (N // 2) * (np.arange(B) >= first)[:, None]).astype(np.int64)
    dense = G.ramped(rng, B, Dn)
    dfeat, dz, dz2 = 1e-3 * G.ramped(rng, B, S + Dn, D), 1e-3 * G.ramped(rng, B, 1), 1e-3 * G.ramped(rng, B, 1)
    dev = [_t(a) for a in (ids, dense, W, W1, dense_w, dense_w_one, dfeat, dz, dz2)]
    ws = ops.Workspace(DEV)
    f64, f32 = (R.fm_forward(ids, dense, W1.astype(dt), W.astype(dt), dense_w_one.astype(dt), dense_w.astype(dt), 0, None)
                for dt in (F64, F32))

    def run():
        full = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=DEV)
        out = (full(B, 1), full(B, 1), full(B, S + Dn, D), full(B, D))
        y1, y2, feat, sum_emb, status = ops.deepfm_fm_fwd(*dev[:6], 0, None, out=out)
        assert int(status.item()) == 0
        bout = (full(B * S, D), full(Dn, D), full(Dn))
        rg, ddw, ddw1 = ops.deepfm_fm_bwd(dev[1], feat, sum_emb, dev[6], dev[7], dev[8], S, ws, out=bout)
        return y1, y2, feat, sum_emb, rg, ddw, ddw1
    y1, y2, feat, sum_emb, rg, ddw, ddw1 = _twice(run)
    what = "deepfm_fm %s " % kernels
    _exact_split(feat, f32[2], first, what + "feat")                                   # a gather and one float32 product
    _close_split(y1, f64[0], f32[0], first, what + "y1")
    _close_split(y2, f64[1], f32[1], first, what + "y2")
    _close_split(sum_emb, f64[2].sum(1), f32[2].sum(1, dtype=F32), first, what + "sum_emb")
    b64, b32 = (R.fm_backward(ids, dense.astype(dt), f32[2].astype(dt), dfeat.astype(dt), dz.astype(dt), dz2.astype(dt), 0, None)
                for dt in (F64, F32))
    _close_split(rg, b64["row_grad"], b32["row_grad"], first * S, what + "row_grad")
    _close(ddw, b64["d_dense_w"][0], b32["d_dense_w"][0], what + "d_dense_w")
    _close(ddw1, b64["d_dense_w_one"], b32["d_dense_w_one"], what + "d_dense_w_one")


# ------------------------------------------------------------------------------------- TiSASRec: the sequence embedding
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_tisas_embed_past_cap(engine_lib, p):
    """ts_embed_kernel (ts_grid: one element per thread, cap 2048 blocks) forward and backward: 174934 ids x dim 3 = CAP8 + 514
    elements; the mask is the counter-based one of oracle/dcn_v2_ref.dropout_keep on the flat element index.  Every element is
    a gather and one (p = 0) or two float32 products: bit for bit."""
    from paddlerec_amd import ops
    from oracle import dcn_v2_ref as X
    n, dim, N, seed, stream, scale = 174934, 3, 50, 2 ** 63 + 9, 2 ** 33 + 1, 3.0 ** 0.5
    rng = np.random.default_rng(23)
    table, d_out = G.ramped(rng, N, dim), G.ramped(rng, n, dim)
    first_rows = CAP8 // dim + 1                                                      # the row that straddles the cap
    ids = (rng.integers(0, N // 2, n) + (N // 2) * (np.arange(n) >= first_rows)).astype(np.int64)
    ids[::53] = 0                                                                      # padding: zero rows
    (tv, _), (dv, _), ids_d = _strided(table, 1), _strided(d_out, 2), _t(ids)
    status = ops.new_status(DEV)

    def run():
        (o, ob), (g, gb) = _out(n, dim, 3), _out(n, dim, 1)
        ops.tisas_embed_fwd(ids_d, tv, scale, p, seed, stream, status=status, out=o)
        ops.tisas_embed_bwd(ids_d, dv, N, scale, p, seed, stream, out=g)
        assert _pad_is_nan(ob, dim) and _pad_is_nan(gb, dim) and int(status.item()) == 0
        return o, g
    o, g = _twice(run)
    keep = X.dropout_keep((n, dim), float(F32(p)), seed, stream) if p else np.ones((n, dim), bool)
    ik, live = F32(1) / (F32(1) - F32(p)), (ids != 0)[:, None]
    for name, got, src in (("fwd", o, table[ids]), ("bwd", g, d_out)):
        x = src * F32(scale)
        want = np.where(keep & live, x * ik if p else x, F32(0)).astype(F32)
        _exact_split(got, want, CAP8, "tisas_embed %s p=%g" % (name, p), flat=True)
    assert p == 0 or 0.24 < 1 - keep.mean() < 0.26


# --------------------------------------------------------------------------------- CrossNetMix: add_into (crossnet_layers.hip)
def test_crossnet_mix_add_into_past_cap(engine_lib):
    """add_into (one element per thread, cap 2048 blocks) folds the parameter gradients of rec_crossnet_mix_layer_bwd: gbias
    (n = d, once per expert, accumulating from the second), g_gate_w (n = d E) and g_gate_b (n = E) — its sizes are those of
    the PARAMETERS, never B d.  d = CAP8 + 513 features, rank 1, two experts, one sample (tests/test_cross_layers_gpu.py's
    harness and float64 reference).  What add_into itself does is one float32 addition or a copy, checked bit for bit on
    both sides of the cap: a backward that accumulates the gate gradients into given values must leave old + (what the same
    backward writes without accumulating); with one sample gbias is the sum over the experts of (dxnext x0) prob_e."""
    import test_cross_layers_gpu as TC
    B, d, r, E = 1, N8, 1, 2
    rng = np.random.default_rng(24)
    old_w, old_b = G.ramped(rng, d, E), G.ramped(rng, E)
    got0, want0, _, _ = TC._mix_run(B, d, r, E, seed=25, fold=True)                      # accumulate_gate = 0, over NaN
    got1, want1, _, _ = TC._mix_run(B, d, r, E, seed=25, fold=True, gate_old=(old_w, old_b))
    # (the layer's long reductions — the gate's dp is a cancelling sum over d = 524801 terms — are not add_into's business and
    # not held to a bar here: tests/test_cross_layers_gpu.py does that at the shipped widths)
    for k in TC.MIX_OUT[:10]:                                                             # everything but the gate gradients
        assert got0[k].tobytes() == got1[k].tobytes(), k
    _exact_split(got1["g_gate_w"], old_w + got0["g_gate_w"], CAP8, "g_gate_w accumulated", flat=True)
    assert np.array_equal(_bits(got1["g_gate_b"]), _bits(old_b + got0["g_gate_b"]))
    x0, xl, Um, Vm, Cm, bias, gw, gb, dxn, old = TC._mix_inputs(B, d, r, E, 25)
    # one sample: g_gate_w[j, e] = x_l[j] dgate[e], one product — dgate[e] (no output of the layer) is the least-squares factor
    x64 = xl.reshape(d).astype(F64)
    c = (got0["g_gate_w"].astype(F64).T @ x64) / (x64 @ x64)
    _close_split(got0["g_gate_w"], x64[:, None] * c[None, :], xl.reshape(d, 1) * c.astype(F32)[None, :], CAP8,
                 "crossnet_mix g_gate_w", flat=True)
    du = (dxn * x0).reshape(d)
    want = du * got0["prob"][0, 0] + du * got0["prob"][0, 1]                              # float32: two products, one addition
    _close_split(got0["gbias"], want.astype(F64), want, CAP8, "crossnet_mix gbias")


# --------------------------------------------------------------------------- row updates under a grouping: lane-per-row kernels
def _host_groups(ops, rows):
    """The grouping rec_ids_group gives for `rows` [n] (every one a valid row), built on the host: positions sorted by row,
    stable; -> (IdGroups on the device, uniq [U] ascending, order [n], seg_offset [U + 1])."""
    n = len(rows)
    order = np.argsort(rows, kind="stable")
    uniq, start = np.unique(rows[order], return_index=True)
    seg = np.concatenate([start, [n]]).astype(np.int32)
    g = ops.IdGroups(n, DEV)
    g.sorted_pos.copy_(_t(order.astype(np.int32)))
    g.uniq_rows[:len(uniq)] = _t(uniq.astype(np.int64))
    g.seg_offset[:len(seg)] = _t(seg)
    g.n_uniq[:2] = _t(np.array([len(uniq), n], np.int32))
    return g, uniq, order, seg


NARROW_CAP = 8192 * 256                           # 32 kNumCU blocks x one row per thread


def test_sparse_adam_rows_narrow_past_cap(engine_lib):
    """rec_sparse_adam_rows on rows without float4 groups (D = 1: sparse_adam_rows_narrow_kernel, one lane per unique row, cap
    8192 blocks): 2 097 152 + 513 unique rows of a table of 7 more, 300 of them looked up twice, a device grad_scale."""
    from paddlerec_amd import ops
    from oracle import deepfm_ref as R
    U, dup = NARROW_CAP + 513, 300
    N = U + 7
    rng = np.random.default_rng(26)
    touched = np.setdiff1d(np.arange(N), np.linspace(3, N - 3, 7).astype(np.int64))
    rows = np.concatenate([touched, touched[np.linspace(0, U - 1, dup).astype(np.int64)]])
    rows = rows[rng.permutation(len(rows))]
    n = len(rows)
    P0, M0, V0 = 0.1 * G.ramped(rng, N), 0.05 * G.ramped(rng, N), (0.02 * G.ramped(rng, N)) ** 2
    grad = 0.1 * G.ramped(rng, n)
    step, hyper, sc = 3, dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8), F32(0.5)
    groups, uniq, order, seg = _host_groups(ops, rows)
    assert len(uniq) == U > NARROW_CAP and np.array_equal(uniq, touched)
    g_d, sc_d = _t(grad.reshape(n, 1)), _t(np.array([sc], F32))

    def run():
        P, M, V = (_t(a.reshape(N, 1)) for a in (P0, M0, V0))
        ops.sparse_adam_rows(groups, g_d, 1, P, M, V, step, grad_scale=sc_d, **hyper)
        return P, M, V
    got = _twice(run)
    refs = []
    for dt in (F64, F32):
        # at most two lookups a row: their float64 sum is exact, its rounding the float32 sum in either order
        merged = np.bincount(rows, weights=grad.astype(F64), minlength=N).astype(dt)
        a = [x[uniq].astype(dt) for x in (P0, M0, V0)]
        R.adam_update(a[0], a[1], a[2], merged[uniq] * dt(sc), step, **{k: float(F32(x)) for k, x in hyper.items()})
        full = [x.astype(dt) for x in (P0, M0, V0)]
        for f, x in zip(full, a):
            f[uniq] = x
        refs.append(full)
    first = int(uniq[NARROW_CAP])                                                      # rows below it: the first pass
    untouched = np.setdiff1d(np.arange(N), uniq)
    for name, x, a, b, x0 in zip("PMV", got, refs[0], refs[1], (P0, M0, V0)):
        x = _n(x).reshape(N)
        _close_split(x, a, b, first, "sparse_adam_rows narrow " + name)
        assert np.array_equal(_bits(x[untouched]), _bits(x0[untouched])), name
    assert G.relerr(refs[0][0], P0) > 1e-3


def test_ps_push_rows_narrow_past_cap(engine_lib):
    """rec_ps_push_rows on its lane-per-feature kernel (no float4 groups, embedx_dim <= 16; cap 8192 blocks): 2 097 152 + 2561
    touched features of the narrowest 'slot' record, 9 floats = embed_w | embedx(1) | 7 statistics, a third of them unborn, a
    third without and a third with their embedx part.  oracle/ps_ref.push_rows is a per-row Python loop, so the ORACLE IS
    SAMPLED: 4096 touched features, half of them from segment indices above 2 097 152 (all of the second pass but its last
    513), compared exactly those rows; show and click (integer counts) are checked on EVERY feature, and every untouched row
    bit for bit with its initial value."""
    from oracle import ps_ref
    from paddlerec_amd import ops
    U, D = NARROW_CAP + 2561, 2
    N = U + 5
    rng = np.random.default_rng(27)
    kw = dict(embedx_threshold=1.5, initial_range=1e-2, seed=77, lr=0.05, embedx_lr=0.02, initial_g2sum=3.0, embedx_initial_g2sum=1.0,
              bounds=(-10.0, 10.0), embedx_bounds=(-0.25, 0.25), embedx_initial_range=2e-2, grad_scale=8.0, show_scale=True,
              embed_zero_init=False)
    make = lambda: ops.PsTable(N, D, DEV, kind="slot", row_stride=9, **kw)
    L = make().layout
    assert (L.row_stride, L.embed_off, L.embedx_off, L.embedx_dim, L.stat_off) == (9, 0, 1, 1, 2)
    lay = dict(embed_off=L.embed_off, embedx_off=L.embedx_off, embedx_dim=L.embedx_dim, stat_off=L.stat_off)
    acc = dict(kw, nonclk_coeff=0.1, click_coeff=1.0)
    so = L.stat_off
    state = (np.arange(N) % 3).astype(F32)
    rec = np.zeros((N, 9), F32)
    born = state > 0
    rec[:, 0] = np.where(born, 0.1 * G.ramped(rng, N), 0)
    rec[:, 1] = np.where(state == 2, 0.1 * (G.ramped(rng, N) - F32(1)), 0)
    show0 = rng.integers(0, 30, N)
    rec[:, so], rec[:, so + 1] = show0 * born, np.minimum(rng.integers(0, 3, N), show0) * born
    rec[:, so + 2], rec[:, so + 3] = rng.random(N) * 0.5 * born, rng.random(N) * 0.5 * (state == 2)
    rec[:, so + 4], rec[:, so + 5], rec[:, so + 6] = state, rng.random(N) * born, rng.integers(0, 9, N) * born
    touched = np.setdiff1d(np.arange(N), np.linspace(2, N - 2, 5).astype(np.int64))
    rows = np.concatenate([touched, touched[np.linspace(0, U - 1, 200).astype(np.int64)]])   # 200 features looked up twice
    rows = rows[rng.permutation(len(rows))]
    n = len(rows)
    grad = 0.05 * (G.ramped(rng, n, D) - F32(1))
    click = (rng.random(n) < 0.4).astype(np.int64)
    groups, uniq, order, seg = _host_groups(ops, rows)
    assert len(uniq) == U and np.array_equal(uniq, touched)
    rec_d, grad_d, click_d = _t(rec), _t(grad), _t(click)

    def run():
        table = make()
        table.rec.copy_(rec_d)
        ops.ps_push_rows(table, groups, grad_d, 1, click=click_d)
        return (table.rec,)
    got = _n(_twice(run)[0])
    cnt = np.bincount(rows, minlength=N)
    clk = np.bincount(rows, weights=click, minlength=N)
    assert np.array_equal(got[:, so], rec[:, so] + cnt.astype(F32)) and np.array_equal(got[:, so + 1], rec[:, so + 1] + clk.astype(F32))
    assert not got[uniq, so + 6].any() and got[uniq, so + 4].min() >= 1                 # seen today; every touched feature exists
    untouched = np.setdiff1d(np.arange(N), uniq)
    assert np.array_equal(got[untouched].view(np.uint32), rec[untouched].view(np.uint32))
    # the sampled oracle
    su = np.sort(np.concatenate([rng.choice(NARROW_CAP, 2048, replace=False), NARROW_CAP + rng.choice(2561, 2048, replace=False)]))
    want = rec.copy()
    merged = np.zeros((len(su), D), F32)
    for k, u in enumerate(su):                                                         # float32 sums in ascending position
        for pos in order[seg[u]:seg[u + 1]]:
            merged[k] += grad[pos]
    ps_ref.push_rows(want, lay, uniq[su], merged[:, 0], merged[:, 1:], cnt[uniq[su]], clk[uniq[su]], acc)
    lo = su < NARROW_CAP
    for name, cols in (("embed_w", [0]), ("embedx", [1]), ("g2sum_w", [so + 2]), ("g2sum_x", [so + 3]), ("delta_score", [so + 5])):
        for rng_name, sel in ((" pass 1", lo), (" later passes", ~lo)):
            r = uniq[su[sel]]
            _close(got[r][:, cols], want[r][:, cols].astype(F64), want[r][:, cols], "ps_push_rows narrow " + name + rng_name)
    assert np.array_equal(got[uniq[su], so + 4], want[uniq[su], so + 4])                  # feature states: exact
    assert (got[uniq[su], so + 4] == 2).sum() > len(su) // 3                              # some were extended by this push


# ------------------------------------------------------------------------------------------ word2vec: rec_w2v_target_update
def test_w2v_target_update_past_caps(engine_lib):
    """w2v_update_short_kernel (one wave per unique target row, cap 8 kNumCU blocks x 4 rows = 8192 rows a pass) and the scan of
    w2v_update_long_kernel (1024 unique rows per block and step, cap 4 kNumCU blocks = 1 048 576 rows a pass): 1 048 601 unique
    target rows, every row of the tables, each looked up once — except the LAST, behind both caps, which 20 positions share (more
    than 16: the long kernel's row).  D = 1, one negative."""
    from paddlerec_amd import ops
    U, hot, lr = 1024 * 1024 + 25, 20, 0.25
    n = U - 1 + hot
    assert n % 2 == 0
    B = n // 2
    rng = np.random.default_rng(28)
    tgt = np.concatenate([np.arange(U - 1), np.full(hot, U - 1)])[rng.permutation(n)].astype(np.int64).reshape(B, 2)
    in_ids = rng.integers(0, U, B).astype(np.int64)
    emb, w0, b0 = G.ramped(rng, U, 1), G.ramped(rng, U, 1), G.ramped(rng, U, 1)
    g = G.ramped(rng, B, 2) - F32(1)
    groups, uniq, order, seg = _host_groups(ops, tgt.reshape(-1))
    assert len(uniq) == U and seg[U] - seg[U - 1] == hot
    emb_d, g_d, in_d = _t(emb), _t(g), _t(in_ids)

    def run():
        (w, wb), (b, bb) = _strided(w0, 1), _strided(b0, 2)
        (dw, dwb), db = _out(n, 1, 1), torch.full((n,), NAN, dtype=torch.float32, device=DEV)
        ops.w2v_target_update(groups, g_d, in_d, emb_d, w, b, lr, dw, db)
        assert _pad_is_nan(wb, 1) and _pad_is_nan(bb, 1) and _pad_is_nan(dwb, 1)
        assert bool(torch.isnan(dw[U:]).all()) and bool(torch.isnan(db[U:]).all())      # nothing behind row U
        return w, b, dw[:U], db[:U]
    w, b, dw, db = _twice(run)
    refs = []
    for dt in (F64, F32):
        gf, x = g.reshape(-1).astype(dt), emb[np.repeat(in_ids, 2), 0].astype(dt)
        flat, c = tgt.reshape(-1), gf * x
        mw, mb = (np.bincount(flat, weights=t.astype(F64), minlength=U).astype(dt) for t in (c, gf))   # single lookups: exact
        hot_pos = order[seg[U - 1]:seg[U]]                                              # the long row: ascending position, in dt
        mw[U - 1], mb[U - 1] = functools.reduce(lambda a, t: a + t, c[hot_pos], dt(0)), functools.reduce(lambda a, t: a + t, gf[hot_pos], dt(0))
        refs.append((w0[:, 0].astype(dt) - dt(F32(lr)) * mw, b0[:, 0].astype(dt) - dt(F32(lr)) * mb, mw, mb))
    for name, x, a, c in zip(("emb_w", "emb_b", "d_w_rows", "d_b_rows"), (w, b, dw, db), refs[0], refs[1]):
        x = _n(x).reshape(U)
        _close_split(x, a, c, 8192, "w2v_target_update " + name)
        _close(x[U - 1:], a[U - 1:], c[U - 1:], "w2v_target_update %s, the long row" % name)
    _exact_split(_n(dw).reshape(U)[:U - 1], refs[1][2][:U - 1], 8192, "w2v d_w_rows of the single lookups")   # one product


# ------------------------------------------------------------------ TiSASRec: the table gradients of rec_tisas_attn_bwd
def test_tisas_attn_bwd_table_gradients_past_cap(engine_lib):
    """ts_pos_grad_kernel (seq_len x hidden elements) and ts_time_fold_kernel (2 x time_rows x hidden), both on ts_grid (one
    element per thread, cap 2048 blocks).  The limits of the attention (seq_len <= 128, seq_len (head | 1) <= 7168) leave one
    way past 524 288 elements: many heads.  seq_len 128, 75 heads of 55 (hidden 4125), 64 time rows, one sample: 528 000
    elements each.  Harness and float64 / float32 reference: tests/test_tisas_gpu.py, tests/tisas_ref.py."""
    import test_tisas_gpu as TT
    B, L, H, hd, T = 1, 128, 75, 55, 64
    D = H * hd
    assert L * D > CAP8 and 2 * T * D > CAP8
    c = TT.case(B, L, D, T, seed=29)
    a, b = TT.gpu_attn(c, H), TT.gpu_attn(c, H)
    r64, r32 = TT.ref_attn(c, H, None, F64), TT.ref_attn(c, H, None, F32)
    assert a["status"] == 0
    for n in TT.NAMES:
        assert a[n].tobytes() == b[n].tobytes(), n
        if n in ("d_pos_k", "d_pos_v"):
            _close_split(a[n], r64[n], r32[n], CAP8, "tisas_attn_bwd " + n, flat=True)
        elif n in ("d_time_k", "d_time_v"):
            _close(a[n], r64[n], r32[n], "tisas_attn_bwd " + n)
        else:
            _close(a[n], r64[n], r32[n], "tisas_attn_bwd " + n)
    both = np.concatenate([a["d_time_k"].reshape(-1), a["d_time_v"].reshape(-1)])      # the fold's own flat index: k side, then v
    w64, w32 = (np.concatenate([r["d_time_k"].reshape(-1), r["d_time_v"].reshape(-1)]) for r in (r64, r32))
    _close_split(both, w64, w32, CAP8, "tisas_attn_bwd d_time (k | v)")


@pytest.mark.parametrize("U", [1024 * 256, 1024 * 256 + 513])
def test_sparse_rows_sumsq_at_and_past_cap(engine_lib, U):
    """rec_sparse_rows_sumsq at D = 1 (one lane per merged row, kSumsqBlocks = 1024 blocks): U unique rows, 100 looked up
    twice."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(U)
    rows = np.concatenate([np.arange(U), np.linspace(0, U - 1, 100).astype(np.int64)])
    rows = rows[rng.permutation(len(rows))]
    grad = G.ramped(rng, len(rows)) - F32(1)
    groups, uniq, order, seg = _host_groups(ops, rows)
    assert len(uniq) == U
    ws, g_d = ops.Workspace(DEV), _t(grad.reshape(-1, 1))

    def run():
        out = torch.full((1,), NAN, dtype=torch.float32, device=DEV)
        return (ops.sparse_rows_sumsq(groups, g_d, 1, out, ws),)
    got, = _twice(run)
    merged = np.bincount(rows, weights=grad.astype(F64), minlength=U)                   # two terms at most: exact in float64
    _close(got, G.sumsq(merged), G.sumsq(merged.astype(F32), dtype=F32), "sparse_rows_sumsq U=%d" % U)


# ------------------------------------------------------------------------------------------- DIN: the attention pool's grids
@pytest.mark.parametrize("Ei,Ec", [(8, 8), (64, 64)])      # the runtime-shaped kernels / the compile-time-shaped pair (E 128)
def test_din_attention_pool_past_resident_grid(engine_lib, Ei, Ec):
    """rec_din_attention_pool_fwd / _bwd run on grids of resident blocks (at most 8 per CU: 2048), a block walking samples
    b, b + grid, ...: 4099 samples of 3 positions are more than two passes.  Backward with and without the saved activations."""
    from paddlerec_amd import ops
    from oracle import din_ref as Dn
    B, Tn, first = 4099, 3, 2048
    rng = np.random.default_rng(Ei)
    ni, nc, E = 500, 41, Ei + Ec
    tabs = [rng.uniform(-0.3, 0.3, (n, d)).astype(F32) for n, d in ((ni, Ei), (nc, Ec), (ni, Ei), (nc, Ec))]
    lens = rng.integers(1, Tn + 1, B)
    valid = np.arange(Tn)[None] < lens[:, None]
    half = (np.arange(B) >= first)[:, None]                                             # ids of the two ranges: other table halves
    hi = (rng.integers(1, ni // 2, (B, Tn)) + (ni // 2) * half) * valid
    hc = (rng.integers(1, nc // 2, (B, Tn)) + (nc // 2) * half) * valid
    mask = np.where(valid, 0, -1000000000).astype(np.int64)
    ti, tc = (np.repeat(rng.integers(1, n, B)[:, None], Tn, 1) for n in (ni, nc))
    aw = [rng.uniform(-0.2, 0.2, s).astype(F32) for s in ((4 * E, 80), (80, 40), (40, 1))]
    ab = [rng.uniform(-0.1, 0.1, s).astype(F32) for s in ((80,), (40,), (1,))]
    dout = G.ramped(rng, B, E) - F32(1)
    ids = [_t(a.astype(np.int64)) for a in (hi, hc, ti, tc)]
    tt, taw, tab, m_d, do_d = [_t(t) for t in tabs], [_t(w) for w in aw], [_t(b) for b in ab], _t(mask), _t(dout)

    def run():
        saved = {}
        out, attw, status = ops.din_attention_pool(*ids, m_d, *tt, taw, tab, saved=saved)
        assert int(status.item()) == 0
        dh, dq = ops.din_attention_pool_bwd(*ids, *tt, taw, tab, attw, do_d, saved=saved)
        dh2, dq2 = ops.din_attention_pool_bwd(*ids, *tt, taw, tab, attw, do_d, saved=None)
        return out, attw, dh, dq, dh2, dq2
    out, attw, dh, dq, dh2, dq2 = _twice(run)
    h = np.concatenate([tabs[0][hi], tabs[1][hc]], 2)
    q = np.concatenate([tabs[2][ti], tabs[3][tc]], 2)
    refs = []
    for dt in (F64, F32):
        c = lambda a: [x.astype(dt) for x in a]
        want, wts = Dn.attention_pool(h.astype(dt), q.astype(dt), mask.astype(dt), c(aw), c(ab), return_weights=True)
        bw = Dn.attention_pool_backward(h.astype(dt), q.astype(dt), mask.astype(dt), c(aw), c(ab), dout.astype(dt))
        refs.append((want, wts, bw["dh"], bw["dq"]))
    what = "din_attention_pool E=%d " % E
    for name, x, k in (("out", out, 0), ("att_weight", attw, 1), ("dh", dh, 2), ("dq", dq, 3), ("dh recomputed", dh2, 2),
                       ("dq recomputed", dq2, 3)):
        _close_split(x, refs[0][k], refs[1][k], first, what + name)
    assert np.all(_n(attw)[~valid] == 0.0)
