"""FFM on the HIP kernels (csrc/ffm_ops.hip) and the wide-row sparse updates it needs (csrc/sparse_update.hip) against
float64 NumPy (tests/ffm_ref.py, oracle/deepfm_ref.py)."""
import numpy as np
import pytest
import torch

import ffm_ref
from helpers import assert_close_scaled
from oracle import deepfm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _problem(B, S, Dn, D, N, seed, stride=None):
    rng = np.random.default_rng(seed)
    R_ = (S + Dn) * D
    stride = stride or (R_ + 3) // 4 * 4
    Wfull = np.zeros((N, stride), np.float32)
    Wfull[:, :R_] = rng.normal(0, 0.3, (N, R_)).astype(np.float32)
    p = dict(W=Wfull, W1=rng.normal(0, 0.1, (N, 1)).astype(np.float32),
             dense_w=rng.normal(0, 0.3, (1, Dn, R_)).astype(np.float32),
             dense_w_one=rng.normal(0, 0.5, Dn).astype(np.float32), bias=np.zeros(1, np.float32))
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    dense = rng.random((B, Dn), dtype=np.float32)
    dz = rng.normal(0, 1, B).astype(np.float32)
    return p, ids, dense, dz


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _run(p, ids, dense, dz, D, grad_stride=None, status=None):
    from paddlerec_amd import ops
    W = _t(p["W"])
    st = status if status is not None else ops.new_status(DEV)
    y1, y2, _ = ops.ffm_fwd(_t(ids), _t(dense), W, _t(p["W1"]), _t(p["dense_w"]), _t(p["dense_w_one"]), D, st)
    rg, dw, dw1 = ops.ffm_bwd(_t(ids), _t(dense), W, _t(p["dense_w"]), _t(dz), D, ops.Workspace(DEV), status=st,
                              grad_stride=grad_stride)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (y1, y2, rg, dw, dw1)], int(st.item())


def _check(p, ids, dense, dz, D, rel=2e-5, grad_stride=None):
    (y1, y2, rg, dw, dw1), st = _run(p, ids, dense, dz, D, grad_stride)
    assert st == 0
    B, S = ids.shape
    gs = rg.shape[1] if B else (grad_stride or ((S + dense.shape[1]) * D + 3) // 4 * 4)
    wy1, wy2 = ffm_ref.forward(ids, dense, p, D)
    wrg, wdw, wdw1 = ffm_ref.backward(ids, dense, p, D, dz, gs)
    if B == 0:
        assert y1.size == 0 and rg.size == 0
        return
    assert_close_scaled(y1, wy1, rel, "y1")
    assert_close_scaled(y2, wy2, rel, "y2")
    assert_close_scaled(rg, wrg, rel, "row_grad")
    R_ = (S + dense.shape[1]) * D
    assert not rg[:, R_:].any(), "pad columns of row_grad must be written 0"
    if dense.shape[1]:
        assert_close_scaled(dw, wdw, rel, "d_dense_w")
        assert_close_scaled(dw1, wdw1, rel, "d_dense_w_one")


def test_ffm_reference_shape_b4096(engine_lib):
    p, ids, dense, dz = _problem(4096, 26, 13, 9, 20000, seed=1)
    _check(p, ids, dense, dz, 9)


@pytest.mark.parametrize("B", [0, 1, 333])
@pytest.mark.parametrize("D", [1, 4, 9, 16])
@pytest.mark.parametrize("S,Dn", [(26, 13), (3, 0), (1, 2)])
def test_ffm_odd_shapes(engine_lib, B, D, S, Dn):
    """D 16 at F 39 (a 97 KB cube) runs the path that reads partners through L2; the others stage the cube in LDS."""
    p, ids, dense, dz = _problem(B, S, Dn, D, 300, seed=B * 100 + D * 10 + S)
    _check(p, ids, dense, dz, D)


def test_ffm_unpadded_stride_and_wide_grad_stride(engine_lib):
    """row_stride = R (351: scalar staging loads) and a row_grad pitch wider than the padded row."""
    p, ids, dense, dz = _problem(257, 26, 13, 9, 500, seed=5, stride=351)
    _check(p, ids, dense, dz, 9, grad_stride=360)


def test_ffm_heavy_duplicates_oob_and_bit_identical_reruns(engine_lib):
    from paddlerec_amd import ops
    p, ids, dense, dz = _problem(1500, 26, 13, 9, 64, seed=7)
    ids[:, :10] = 3                                        # one row in 10 of 26 slots of every sample
    _check(p, ids, dense, dz, 9)
    a, _ = _run(p, ids, dense, dz, 9)
    b, _ = _run(p, ids, dense, dz, 9)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                        # fixed-order reductions: bit-identical
    bad = ids.copy()
    bad[5, 2], bad[9, 25], bad[11, 0] = -1, 64, 10 ** 12    # outside [0, N)
    st = ops.new_status(DEV)
    (y1, y2, rg, dw, dw1), s = _run(p, bad, dense, dz, 9, status=st)
    assert s & 1
    Wz = dict(p)
    Wz["W"] = np.vstack([p["W"], np.zeros((1, p["W"].shape[1]), np.float32)])
    Wz["W1"] = np.vstack([p["W1"], np.zeros((1, 1), np.float32)])
    zero_row = np.where((bad < 0) | (bad >= 64), 64, bad)  # an OOB id reads as a zero row
    wy1, wy2 = ffm_ref.forward(zero_row, dense, Wz, 9)
    assert_close_scaled(y1, wy1, 2e-5, "y1")
    assert_close_scaled(y2, wy2, 2e-5, "y2")
    wrg, _, _ = ffm_ref.backward(zero_row, dense, Wz, 9, dz, rg.shape[1])
    assert_close_scaled(rg, wrg, 2e-5, "row_grad")


def test_ffm_full_size_table_high_row_ids(engine_lib):
    """The reference table, 1 000 001 x 352 floats: byte offsets of the last rows pass 2^31."""
    from paddlerec_amd import ops
    N, B, S, Dn, D = 1000001, 64, 26, 13, 9
    W = torch.zeros(N, 352, dtype=torch.float32, device=DEV)
    rng = np.random.default_rng(11)
    ids = rng.integers(N - 100, N, (B, S), dtype=np.int64)
    ids[0, 0] = 0
    rows = np.unique(ids)
    vals = rng.normal(0, 0.3, (len(rows), 351)).astype(np.float32)
    W[_t(rows), :351] = _t(vals)
    W1 = torch.zeros(N, 1, dtype=torch.float32, device=DEV)
    dense = rng.random((B, Dn), dtype=np.float32)
    dense_w = rng.normal(0, 0.3, (1, Dn, 351)).astype(np.float32)
    dense_w_one = rng.normal(0, 0.5, Dn).astype(np.float32)
    dz = rng.normal(0, 1, B).astype(np.float32)
    st = ops.new_status(DEV)
    y1, y2, _ = ops.ffm_fwd(_t(ids), _t(dense), W, W1, _t(dense_w), _t(dense_w_one), D, st)
    rg, _, _ = ops.ffm_bwd(_t(ids), _t(dense), W, _t(dense_w), _t(dz), D, ops.Workspace(DEV), status=st)
    assert int(st.item()) == 0
    local = np.searchsorted(rows, ids)
    Wl = np.zeros((len(rows), 352), np.float32)
    Wl[:, :351] = vals
    p = dict(W=Wl, W1=np.zeros((len(rows), 1), np.float32), dense_w=dense_w, dense_w_one=dense_w_one)
    wy1, wy2 = ffm_ref.forward(local, dense, p, D)
    wrg, _, _ = ffm_ref.backward(local, dense, p, D, dz, 352)
    assert_close_scaled(y1.cpu().numpy(), wy1, 2e-5, "y1")
    assert_close_scaled(y2.cpu().numpy(), wy2, 2e-5, "y2")
    assert_close_scaled(rg.cpu().numpy(), wrg, 2e-5, "row_grad")
    del W


# ------------------------------------------------------------------ wide rows in the sparse updates
@pytest.mark.parametrize("width", [352, 624])
@pytest.mark.parametrize("lazy", [True, False])
def test_wide_row_updates(engine_lib, width, lazy):
    """segment_partials + sparse_adam_rows / adam_rows_all at rows of 352 and 624 floats (LANES 128 / 256): against the
    NumPy merge + Adam, with a hot row long enough for the tile partials; the last column plays FFM's pad column (zero
    gradient, zero start) and must stay exactly 0."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(width + lazy)
    N, n = 700, 5000
    ids = rng.integers(0, N, n, dtype=np.int64)
    ids[rng.random(n) < 0.4] = 17                          # one hot row: long segments -> tile partials
    ids[-1] = N - 1
    grad = rng.normal(0, 1, (n, width)).astype(np.float32)
    grad[:, -1] = 0.0
    P = rng.normal(0, 0.1, (N, width)).astype(np.float32)
    P[:, -1] = 0.0
    M = np.zeros_like(P)
    V = np.zeros_like(P)
    Pt, Mt, Vt, gt = _t(P), _t(M), _t(V), _t(grad)
    idt = _t(ids.reshape(-1, 1))
    groups, _ = ops.ids_group(idt, N, None, ops.Workspace(DEV))
    upd = ops.sparse_adam_rows if lazy else ops.adam_rows_all
    for step in (1, 2):
        pp = ops.segment_partials(groups, gt, width)
        upd(groups, gt, 1, Pt, Mt, Vt, step, lr=1e-2, partials=pp)
        uniq, merged, _ = R.merge_rows(ids, np.ones(n, bool), grad)
        (R.adam_update_rows if lazy else R.adam_update_dense_equivalent)(P, M, V, uniq, merged, step, lr=1e-2)
    torch.cuda.synchronize()
    for got, want, name in ((Mt, M, "m"), (Vt, V, "v"), (Pt, P, "P")):
        assert_close_scaled(got.cpu().numpy(), want, 1e-5, name)
    for t in (Pt, Mt, Vt):
        assert not t[:, -1].cpu().numpy().any()


def test_wide_rows_reject_unvectorisable_widths(engine_lib):
    from paddlerec_amd import _lib, ops
    N, n, width = 50, 64, 351                              # > 256 floats but not a multiple of 4
    groups, _ = ops.ids_group(_t(np.arange(n, dtype=np.int64).reshape(-1, 1) % N), N, None, ops.Workspace(DEV))
    P = torch.zeros(N, width, device=DEV)
    with pytest.raises(_lib.RecError, match="rc=-2"):
        ops.sparse_adam_rows(groups, torch.zeros(n, width, device=DEV), 1, P, torch.zeros_like(P),
                             torch.zeros_like(P), 1)


# ------------------------------------------------------------------ the layer and the loops
@pytest.mark.parametrize("lazy", [True, False])
def test_ffm_layer_gpu(engine_lib, lazy):
    import test_ffm
    test_ffm.check_layer("cuda", None, 1e-5, lazy)


@pytest.mark.parametrize("lazy", [True, False])
def test_ffm_trainer_loops_gpu(engine_lib, tmp_path, lazy):
    import test_ffm
    test_ffm.run_trainer_loops(tmp_path, "cuda", None, lazy)
