"""rank/dcn on the HIP kernels (csrc/dcn_cross.hip): rec_dcn_cross_fwd / rec_dcn_cross_bwd against the float64 NumPy
restatement (tests/dcn_ref.py), the layer against the fixture, the trainer loops.

Inputs of the kernel tests: x_0 ~ N(0, 1), w ~ N(0, 0.5 / sqrt(d)), b ~ N(0, 0.1), so s_l = <x_l, w> is O(1) at every d
and the stack grows by a small factor per layer.  Tolerance: helpers.assert_close_scaled at 2e-5, the bar of the FFM /
FEFM kernels against float64.  The float32 restatement's own scaled error |err| / (|want| + max|want|) against float64
on these inputs, measured on the CPU over every (d, L, B) of the parametrised test below, the reference shape, the l2
case and the B 20000 rerun case, is at most 1.7e-6 (d_b at B 20000; d_w 1.4e-6, dx0 7.4e-7, x_L / s_l / l2 under 3.3e-7)
— a factor 12 under the bar, so no case asks for more."""
import numpy as np
import pytest
import torch

import dcn_ref as DR
from helpers import assert_close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 2e-5


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _problem(B, d, seed):
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((B, d)).astype(np.float32)
    w = (rng.standard_normal(d) * 0.5 / np.sqrt(d)).astype(np.float32)
    b = (rng.standard_normal(d) * 0.1).astype(np.float32)
    dxl = rng.standard_normal((B, d)).astype(np.float32)
    return x0, w, b, dxl


def _rows(a, ld, offset=0, fill=np.nan):
    """`a` [B, d] as a device view of row stride ld, starting `offset` floats into its buffer; the rest holds `fill`."""
    B, d = a.shape
    buf = torch.full((B * ld + offset + 8,), fill, dtype=torch.float32, device=DEV)
    v = torch.as_strided(buf, (B, d), (ld, 1), offset)
    v.copy_(_t(a))
    return v, buf


def _run(x0, w, b, dxl, L, coeff=1.0, ld=None, offset=0):
    """fwd + bwd (the matrix form) through ops at row stride ld -> numpy (x_L, saved, l2, dx0, d_w, d_b)."""
    from paddlerec_amd import ops
    B, d = x0.shape
    ld = ld or d
    ws = ops.Workspace(DEV)
    xv, _ = _rows(x0, ld, offset)
    gv, _ = _rows(dxl, ld, offset)
    ov, _ = _rows(np.zeros_like(x0), ld, offset)
    dv, _ = _rows(np.zeros_like(x0), ld, offset)
    xl, saved, l2 = ops.dcn_cross_fwd(xv, _t(w), _t(b), L, ws, l2_coeff=coeff, out=(ov, None, None))
    dx0, dw, db = ops.dcn_cross_bwd(xv, _t(w), _t(b), saved, gv, ws, l2_coeff=coeff, out=(dv, None, None))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (xl, saved, l2, dx0, dw, db)]


def _check(x0, w, b, dxl, L, coeff=1.0, ld=None, offset=0):
    xl, saved, l2, dx0, dw, db = _run(x0, w, b, dxl, L, coeff, ld, offset)
    B, d = x0.shape
    assert xl.shape == (B, d) and saved.shape == (B, L) and dx0.shape == (B, d) and dw.shape == db.shape == (d,)
    if B == 0:
        assert not l2.any() and not dw.any() and not db.any()             # empty sums
        return
    wxl, ws_, wl2, _ = DR.cross_forward(x0, w, b, L)
    wdx0, wdw, wdb = DR.cross_backward(x0, w, b, L, dxl, coeff)
    assert_close_scaled(xl, wxl, REL, "x_L")
    assert_close_scaled(saved, ws_, REL, "saved s_l")
    assert_close_scaled(l2, np.asarray([coeff * wl2]), REL, "l2")
    assert_close_scaled(dx0, wdx0, REL, "dx0")
    assert_close_scaled(dw, wdw, REL, "d_w")
    assert_close_scaled(db, wdb, REL, "d_b")


@pytest.mark.parametrize("ld", [247, 248])
def test_reference_shape_b4096(engine_lib, ld):
    """d 247, L 2, B 4096: rows back to back (247: the scalar form) and at the layer's padded stride (248: 16-byte vectors,
    the tail chunk of a row element by element)."""
    _check(*_problem(4096, 247, seed=1), 2, ld=ld)


@pytest.mark.parametrize("B", [0, 1, 63, 1000])
@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 5, 64, 247, 429, 512])
def test_odd_shapes(engine_lib, d, L, B):
    """Multiples of 4 and not, both register widths (d <= 256: 4 floats per lane, above: 8); contiguous rows, so d 64 and
    512 run the vector form and the others the scalar one.  B 1000 gives every backward wave several rows' worth of
    blocks to fold."""
    _check(*_problem(B, d, seed=d * 1000 + L * 10 + B % 7), L)


@pytest.mark.parametrize("d,ld,offset", [(247, 300, 3), (247, 252, 4), (429, 432, 0), (64, 100, 0), (5, 8, 0)])
def test_strided_rows(engine_lib, d, ld, offset):
    """Rows inside wider buffers: aligned and padded (vector form with a masked tail), and off by 3 floats (scalar)."""
    _check(*_problem(300, d, seed=ld), 3, ld=ld, offset=offset)


def test_output_lands_in_a_column_block_and_touches_nothing_else(engine_lib):
    """x_L into columns [128, 375) of a [B, 376] fc input, dx0 into a [B, 248] buffer: every float outside the [B, d]
    blocks — the pad column of each row included — keeps its value."""
    from paddlerec_amd import ops
    B, d, H, L = 333, 247, 128, 2
    x0, w, b, dxl = _problem(B, d, seed=3)
    ws = ops.Workspace(DEV)
    xv, _ = _rows(x0, 248)
    gv, _ = _rows(dxl, 248)
    last = torch.full((B, 376), 7.5, device=DEV)
    dbuf = torch.full((B, 248), -3.25, device=DEV)
    saved = torch.full((B + 1, L), 9.0, device=DEV)
    _, s, _ = ops.dcn_cross_fwd(xv, _t(w), _t(b), L, ws, out=(last[:, H:H + d], saved[:B], None))
    ops.dcn_cross_bwd(xv, _t(w), _t(b), s, gv, ws, out=(dbuf[:, :d], None, None))
    torch.cuda.synchronize()
    got = last.cpu().numpy()
    assert (got[:, :H] == 7.5).all() and (got[:, H + d:] == 7.5).all()
    assert_close_scaled(got[:, H:H + d], DR.cross_forward(x0, w, b, L)[0], REL, "x_L")
    assert (dbuf[:, d:].cpu().numpy() == -3.25).all() and (saved[B].cpu().numpy() == 9.0).all()
    assert_close_scaled(dbuf[:, :d].cpu().numpy(), DR.cross_backward(x0, w, b, L, dxl)[0], REL, "dx0")


@pytest.mark.parametrize("ld", [247, 248])
def test_dx0_accumulate_and_overwrite(engine_lib, ld):
    from paddlerec_amd import ops
    B, d, L = 500, 247, 3
    x0, w, b, dxl = _problem(B, d, seed=4)
    base = np.random.default_rng(5).standard_normal((B, d)).astype(np.float32)
    ws = ops.Workspace(DEV)
    xv, _ = _rows(x0, ld)
    gv, _ = _rows(dxl, ld)
    _, s, _ = ops.dcn_cross_fwd(xv, _t(w), _t(b), L, ws)
    want = DR.cross_backward(x0, w, b, L, dxl)[0]
    acc, _ = _rows(base, ld)
    ops.dcn_cross_bwd(xv, _t(w), _t(b), s, gv, ws, accumulate=True, out=(acc, None, None))
    assert_close_scaled(acc.cpu().numpy(), want + base, REL, "dx0 (accumulate)")
    ovr, _ = _rows(base, ld)
    ops.dcn_cross_bwd(xv, _t(w), _t(b), s, gv, ws, accumulate=False, out=(ovr, None, None))
    assert_close_scaled(ovr.cpu().numpy(), want, REL, "dx0 (overwrite)")
    with pytest.raises(Exception, match="accumulate"):
        ops.dcn_cross_bwd(xv, _t(w), _t(b), s, gv, ws, accumulate=True)


@pytest.mark.parametrize("coeff", [0.0, 1.0, 0.37])
def test_l2_coefficient(engine_lib, coeff):
    """0 drops the term from the loss and from every gradient, 1 is the reference; the terms are large next to the
    stack's own gradient here (w^2 is not small), so a missing or doubled factor cannot hide in the tolerance."""
    x0, w, b, dxl = _problem(700, 247, seed=6)
    w = (w * 8).astype(np.float32)
    a = DR.cross_backward(x0, w, b, 2, dxl, 0.0)
    c = DR.cross_backward(x0, w, b, 2, dxl, 1.0)
    assert np.abs(c[1] - a[1]).max() > 0.5 * np.abs(a[1]).max()            # the l2 part of d_w is not a rounding matter
    _check(x0, w, b, dxl, 2, coeff=coeff, ld=248)


def test_inference_form_without_saved_and_l2(engine_lib):
    from paddlerec_amd import ops
    x0, w, b, _ = _problem(1000, 247, seed=7)
    ws = ops.Workspace(DEV)
    xv, _ = _rows(x0, 248)
    full = ops.dcn_cross_fwd(xv, _t(w), _t(b), 2, ws)
    lean = ops.dcn_cross_fwd(xv, _t(w), _t(b), 2, ws, want_saved=False, want_l2=False)
    assert lean[1] is None and lean[2] is None
    assert torch.equal(full[0], lean[0])                                      # the same x_L, bit for bit
    assert_close_scaled(lean[0].cpu().numpy(), DR.cross_forward(x0, w, b, 2)[0], REL, "x_L")


@pytest.mark.parametrize("d,ld", [(247, 248), (247, 247), (429, 432)])
def test_rank1_form_equals_the_matrix_form(engine_lib, d, ld):
    """dXL = NULL with dz [B] and u [d]: the upstream gradient dz[r] * u[k] formed in registers, against the restatement
    on the materialised matrix, next to the matrix form of the kernel on the same values."""
    from paddlerec_amd import ops
    B, L = 777, 3
    x0, w, b, _ = _problem(B, d, seed=8)
    rng = np.random.default_rng(9)
    dz = rng.standard_normal(B).astype(np.float32)
    u = rng.standard_normal(d).astype(np.float32)
    mat = (dz[:, None] * u[None, :]).astype(np.float32)                      # what the kernel forms: one f32 product
    ws = ops.Workspace(DEV)
    xv, _ = _rows(x0, ld)
    gv, _ = _rows(mat, ld)
    _, s, _ = ops.dcn_cross_fwd(xv, _t(w), _t(b), L, ws)
    r1 = ops.dcn_cross_bwd(xv, _t(w), _t(b), s, None, ws, dz=_t(dz).reshape(B, 1), u=_t(u))
    mf = ops.dcn_cross_bwd(xv, _t(w), _t(b), s, gv, ws)
    want = DR.cross_backward(x0, w, b, L, mat)
    for got, other, wv, name in zip(r1, mf, want, ("dx0", "d_w", "d_b")):
        assert_close_scaled(got.cpu().numpy(), wv, REL, name + " (rank-1)")
        assert_close_scaled(other.cpu().numpy(), wv, REL, name + " (matrix)")


def test_backward_bit_identical_reruns(engine_lib):
    """d_w / d_b are batch sums folded in a fixed order: two runs on the same inputs give identical bits (B large enough
    for every resident block to hold rows, both forms of the upstream gradient)."""
    from paddlerec_amd import ops
    B, d, L = 20000, 247, 2
    x0, w, b, dxl = _problem(B, d, seed=10)
    ws = ops.Workspace(DEV)
    xv, _ = _rows(x0, 248)
    gv, _ = _rows(dxl, 248)
    dz, u = _t(dxl[:, 0].copy()), _t(dxl[0].copy())
    outs = []
    for _ in range(2):
        xl, s, l2 = ops.dcn_cross_fwd(xv, _t(w), _t(b), L, ws)
        a = ops.dcn_cross_bwd(xv, _t(w), _t(b), s, gv, ws)
        c = ops.dcn_cross_bwd(xv, _t(w), _t(b), s, None, ws, dz=dz, u=u)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (xl, s, l2) + tuple(a) + tuple(c)])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    assert_close_scaled(outs[0][4], DR.cross_backward(x0, w, b, L, dxl)[1], REL, "d_w")


def test_ops_reject_bad_arguments(engine_lib):
    from paddlerec_amd import _lib, ops
    ws = ops.Workspace(DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(_lib.RecError, match="rc=-1"):
        ops.dcn_cross_fwd(z(4, 513), z(513), z(513), 2, ws)
    with pytest.raises(_lib.RecError, match="rc=-1"):
        ops.dcn_cross_fwd(z(4, 8), z(8), z(8), 65, ws)
    with pytest.raises(_lib.RecError, match="d = 8"):
        ops.dcn_cross_fwd(z(4, 8), z(7), z(8), 2, ws)
    with pytest.raises(_lib.RecError, match="rank-1"):
        ops.dcn_cross_bwd(z(4, 8), z(8), z(8), z(4, 2), None, ws)
    with pytest.raises(_lib.RecError, match="device"):
        ops.dcn_cross_fwd(torch.zeros(4, 8), z(8), z(8), 2, ws)


# ------------------------------------------------------------------ the layer and the loops
def test_layer_matches_fixture_gpu(engine_lib):
    import test_dcn
    test_dcn.check_layer_on_fixture(DEV, None, 2e-5)


@pytest.mark.parametrize("lazy", [False, True])
def test_adam_trajectory_gpu(engine_lib, lazy):
    import test_dcn
    test_dcn.check_adam_trajectory(DEV, None, lazy, 1e-5)


@pytest.mark.parametrize("lazy", [False, True])
def test_full_size_step_b512(engine_lib, lazy):
    """dcn/config_bigdata.yaml: 1 000 001 rows, D 9, cross_num 2, the [512, 256, 128] tower, batch 512.  Two train steps;
    the loss and prediction of the first equal the restatement's on the same draw, and exactly the rows the batches
    touched have moved (a zero gradient on zero moments moves nothing under either Adam; the padding row never moves)."""
    from paddlerec_amd.dcn import DeepCroLayer
    N, B = 1000001, 512
    m = DeepCroLayer(N, 9, 13, 26, [512, 256, 128], 2, 100.0, 5e-5, False, device=DEV)
    m.lazy_mode = lazy
    rng = np.random.default_rng(B + lazy)
    ids = rng.integers(1, N, (B, 26), dtype=np.int64)
    ids[rng.random((B, 26)) < 0.05] = 0
    ids[:, 1] = N - 1                                                         # a hot row at the table's end
    dense = rng.random((B, 13), dtype=np.float32)
    label = (rng.random((B, 1)) < 0.3).astype(np.int64)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    loss, pred = m.train_step(_t(ids), _t(dense), _t(label), lr=1e-3)
    f = DR.forward(ids, dense, sd, 9, 2)
    want = float(DR.log_loss_mean(f["pred"], label) + f["l2"])
    np.testing.assert_allclose(float(loss), want, rtol=1e-5)
    np.testing.assert_allclose(pred.cpu().numpy(), f["pred"], rtol=1e-5, atol=1e-6)
    m.train_step(_t(ids), _t(dense), _t(label), lr=1e-3)
    assert int(m.status.item()) == 0 and m.step_count == 2
    moved = (m.embedding.cpu().numpy() != sd["embedding.weight"]).any(axis=1)
    touched = np.zeros(N, bool)
    touched[ids.reshape(-1)] = True
    touched[0] = False
    assert np.array_equal(moved, touched)
    assert not m.rec[:, 9:].any()
    for k in ("layer_w", "layer_b", "fc.weight", "linear_0.weight"):
        assert (m.state_dict()[k].cpu().numpy() != sd[k]).any(), k
    del m


@pytest.mark.parametrize("lazy", [True, False])
def test_dcn_trainer_loops_gpu(engine_lib, tmp_path, lazy):
    import test_dcn
    test_dcn.run_trainer_loops(tmp_path, "cuda", None, lazy)
