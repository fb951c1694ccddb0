"""The CrossNet layer entry points (csrc/crossnet_layers.hip) and their glue kernels (csrc/cross_ops.hip: cross_bwd_prep,
moe_bwd_prep, softmax_rows{,_bwd}; csrc/sparse_update.hip: sumsq, clip_scale) driven directly through their C-ABI over a
shape / stride grid, each against a float64 restatement of the same operation.

The models' own tests reach these kernels only at d = 39 * D (a multiple of 4), E = 4, r in {8, 16} and contiguous
buffers.  The numbered gaps the cases below close (each docstring names its own):
  1. the scalar branch of cross_bwd_prep_kernel (n % 4 != 0, a leading dimension % 4 != 0, a pointer not 16-byte aligned)
  2. moe_bwd_prep_kernel with N < 64 / N % 64 != 0 (idle lanes of the wave reduction) and > 8192 rows (grid-stride loop)
  3. softmax_rows{,_bwd} for E != 4 and logits that need the max subtraction
  4. rec_crossnet_v2_layer_bwd in place (dXl = dXnext) and accumulate_dx0 = 0 over garbage
  5. rec_crossnet_mix_layer_* with E != 4, r % 4 != 0, the reference's d 1560 / r 256 / E 4, saturated tanh,
     accumulate_gate on its own
  6. gradient buffers strided wider than every stride of the descriptor (include/recengine.h: all-or-nothing)
  7. rec_sumsq / rec_clip_scale against NumPy

Bounds.  Layers: helpers.assert_close_floor — the NumPy formulas run in float64 (reference) and in float32 (the measured
noise floor); 1e-5 of the tensor's scale or 4x the floor, whichever is larger, and outside the two named noisy cases
(E = 64, saturated tanh) the test asserts that the 1e-5 term is the binding one.  Elementwise glue: a few float32
roundings u = 2^-24 of an exact expression (stated per kernel below).  Every input is np.random.default_rng(<seed>).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_close_floor
from oracle import dcn_v2_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24          # unit roundoff of float32
SENT = -7.0             # what every byte outside a strided operand's columns holds before and after a call
P = X.P
f32, f64 = np.float32, np.float64


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def N_(t):
    return t.detach().cpu().numpy()


def _ops():
    from paddlerec_amd import ops
    return ops


class Wide:
    """A [m, n] operand as columns [col, col + n) of a [m, ld] buffer pre-filled with the sentinel (ld = n, col = 0:
    contiguous).  .v is the view handed to the kernel; .intact() says whether every other column still is the sentinel."""

    def __init__(self, shape, ld=None, col=0, a=None, fill=None):
        m, n = shape
        ld = n if ld is None else ld
        assert col + n <= ld
        self.n, self.col = n, col
        self.buf = torch.full((m, ld), SENT, dtype=torch.float32, device=DEV)
        self.v = self.buf[:, col:col + n]
        if a is not None:
            self.v.copy_(T(np.asarray(a, f32)))
        elif fill is not None:
            self.v.fill_(fill)

    def intact(self):
        b = N_(self.buf).copy()
        b[:, self.col:self.col + self.n] = SENT
        return bool(np.all(b == SENT))

    def untouched(self):
        return bool(np.all(N_(self.buf) == SENT))


def both(fn, *arrays, **kw):
    """fn on the float64 and on the float32 version of the same (float32-valued) inputs -> (want64, want32)."""
    a64 = [None if a is None else np.asarray(a, f64) for a in arrays]
    a32 = [None if a is None else np.asarray(a, f32) for a in arrays]
    return fn(*a64, **kw), fn(*a32, **kw)


def close(got, w64, w32, name, noisy=False):
    """assert_close_floor, plus the condition of the file's header: outside the named noisy cases the 1e-5-of-scale
    term must be the binding one (a later change of inputs cannot quietly turn this into a floor-only comparison)."""
    got = N_(got) if torch.is_tensor(got) else np.asarray(got)
    w64, w32 = np.asarray(w64, f64), np.asarray(w32, f64)
    scale = float(np.abs(w64).max())
    floor = float(np.abs(w32.reshape(w64.shape) - w64).max())
    if noisy:
        print("%s: bound is %s (1e-5 of scale %.3e, 4 x fp32 floor %.3e)" % (
            name, "the measured floor" if 4 * floor > 1e-5 * scale else "1e-5 of scale", 1e-5 * scale, 4 * floor))
    else:
        assert 4 * floor <= 1e-5 * scale, "%s: fp32 floor %.3e is not below 1e-5 of scale %.3e / 4" % (name, floor, scale)
    assert np.all(np.isfinite(got)), name + " is not finite"
    assert_close_floor(got, w64, w32.reshape(w64.shape), err_msg=name)


# ====================================================================================================== cross_bwd_prep
def _cross_prep(m, n, seed, accumulate=False, lay=None, poison=False):
    """dU = dX * X0 is ONE float32 product: bit-equal to NumPy's.  dX0_acc = (old +) dX * U is a rounded product and,
    when accumulating, a rounded sum: |err| <= 2u (|dX U| + |old|) against float64."""
    ops = _ops()
    rng = np.random.default_rng(seed)
    g, x, u, old = (rng.standard_normal((m, n)).astype(f32) for _ in range(4))
    lay = lay or {}
    w = {k: Wide((m, n), *lay.get(k, (n, 0)), a=a) for k, a in
         (("dX", g), ("X0", x), ("U", u), ("dU", None), ("acc", old if accumulate else None))}
    if poison:
        w["acc"].v.fill_(float("nan"))
    ops.cross_bwd_prep(w["dX"].v, w["X0"].v, w["U"].v, w["dU"].v, w["acc"].v, accumulate)
    torch.cuda.synchronize()
    dU, acc = N_(w["dU"].v), N_(w["acc"].v)
    assert np.array_equal(dU, g * x), "dU is not the float32 product dX * X0"
    prod = g.astype(f64) * u.astype(f64)
    want = prod + (old.astype(f64) if accumulate else 0.0)
    bound = 2 * U * (np.abs(prod) + (np.abs(old.astype(f64)) if accumulate else 0.0))
    assert np.all(np.isfinite(acc))
    err = np.abs(acc - want)
    assert np.all(err <= bound), "dX0_acc: worst err / bound = %.3f" % float((err / np.maximum(bound, 1e-300)).max())
    for k, t in w.items():
        assert t.intact(), "columns outside the %s slice were written" % k


@pytest.mark.parametrize("n", [1, 3, 4, 39, 156, 351, 1560])
@pytest.mark.parametrize("m", [1, 2, 255, 257])
@pytest.mark.parametrize("accumulate", [False, True])
def test_cross_bwd_prep_grid(engine_lib, m, n, accumulate):
    """Gap 1: n in {1, 3, 39, 351} is the scalar branch (n % 4 != 0: d = 39 * 9), n in {4, 156, 1560} the float4 one;
    accumulate = 0 writes over NaN (the kernel must not read what it overwrites)."""
    _cross_prep(m, n, seed=1000 * n + m, accumulate=accumulate, poison=not accumulate)


@pytest.mark.parametrize("m,n", [(4096, 1560), (4099, 351)])
def test_cross_bwd_prep_grid_stride_loop(engine_lib, m, n):
    """More elements than the capped grid's 2048 * 256 threads: the grid-stride loop, on the float4 branch
    (4096 x 1560 = 1.6 M float4s) and on the scalar one (4099 x 351: gap 1)."""
    _cross_prep(m, n, seed=m + n, accumulate=True)


@pytest.mark.parametrize("case", ["vec_strided", "unaligned", "odd_ld_acc"])
def test_cross_bwd_prep_strided(engine_lib, case):
    """Gap 1, n = 156: (vec_strided) all five operands at column 4 of [m, 176] — float4 branch with row strides;
    (unaligned) the same at column 1 — 4-byte aligned pointers must take the scalar branch and still be right;
    (odd_ld_acc) only dX0_acc in a [m, 157] buffer.  Nothing outside the slices is written."""
    names = ("dX", "X0", "U", "dU", "acc")
    lay = {"vec_strided": {k: (176, 4) for k in names}, "unaligned": {k: (176, 1) for k in names},
           "odd_ld_acc": {"acc": (157, 0)}}[case]
    for m, acc in ((1, False), (130, True), (257, False)):
        _cross_prep(m, 156, seed=7 + m, accumulate=acc, lay=lay, poison=not acc)


def test_cross_bwd_prep_edges(engine_lib):
    """m = 0 succeeds without touching anything; a leading dimension below n is REC_EINVAL."""
    ops = _ops()
    e = torch.empty(0, 8, device=DEV)
    ops.cross_bwd_prep(e, e, e, torch.empty(0, 8, device=DEV), torch.empty(0, 8, device=DEV), False)
    t = [Wide((3, 8), fill=1.0) for _ in range(5)]
    p = [C.c_void_p(w.v.data_ptr()) for w in t]
    for bad in range(5):
        lds = [8] * 5
        lds[bad] = 7
        rc = engine_lib.rec_cross_bwd_prep(3, 8, p[0], lds[0], p[1], lds[1], p[2], lds[2], p[3], lds[3], p[4], lds[4], 0,
                                           ops._stream())
        assert rc == -1
    torch.cuda.synchronize()
    assert all(bool((w.v == 1.0).all()) for w in t)


# ======================================================================================================== moe_bwd_prep
def _moe_prep(m, n, seed, E=1, e=0, accumulate=False, lay=None, poison=False):
    """du = (g x) p: two roundings, 2u |g x p|.  dX0_acc = (old +) (g p) u: three, 4u (|g p u| + |old|).  dp = sum_j
    g x u: the GEMM tests' dot-product bound 4e-7 * sum_j |g x u| per row (tests/test_gemm_gpu.py)."""
    ops = _ops()
    rng = np.random.default_rng(seed)
    g, x, u, old = (rng.standard_normal((m, n)).astype(f32) for _ in range(4))
    prob = rng.uniform(0.05, 1.0, (m, E)).astype(f32)
    lay = lay or {}
    w = {k: Wide((m, n), *lay.get(k, (n, 0)), a=a) for k, a in
         (("dX", g), ("X0", x), ("U", u), ("dU", None), ("acc", old if accumulate else None))}
    if poison:
        w["acc"].v.fill_(float("nan"))
    pt = T(prob)
    dp = torch.full((m, E), SENT, dtype=torch.float32, device=DEV)
    ops.moe_bwd_prep(w["dX"].v, w["X0"].v, w["U"].v, pt[:, e], w["dU"].v, w["acc"].v, accumulate, dp[:, e])
    torch.cuda.synchronize()
    g6, x6, u6, p6 = g.astype(f64), x.astype(f64), u.astype(f64), prob[:, e:e + 1].astype(f64)
    du, acc, dpn = N_(w["dU"].v), N_(w["acc"].v), N_(dp)
    assert np.all(np.isfinite(du)) and np.all(np.isfinite(acc)) and np.all(np.isfinite(dpn))
    assert np.all(np.abs(du - g6 * x6 * p6) <= 2 * U * np.abs(g6 * x6 * p6)), "du"
    term = g6 * p6 * u6
    want = term + (old.astype(f64) if accumulate else 0.0)
    bound = 4 * U * (np.abs(term) + (np.abs(old.astype(f64)) if accumulate else 0.0))
    assert np.all(np.abs(acc - want) <= bound), "dX0_acc"
    dots = g6 * x6 * u6
    err = np.abs(dpn[:, e] - dots.sum(axis=1))
    assert np.all(err <= 4e-7 * np.abs(dots).sum(axis=1)), "dp: worst err / bound %.3f" % float(
        (err / (4e-7 * np.abs(dots).sum(axis=1))).max())
    other = np.delete(dpn, e, axis=1)
    assert np.all(other == SENT), "dp columns of other experts were written"
    for k, t in w.items():
        assert t.intact(), "columns outside the %s slice were written" % k


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 351, 1560])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 130])
def test_moe_bwd_prep_grid(engine_lib, m, n):
    """Gap 2: n < 64 leaves lanes of the wave without an element (their partial dot must be 0 in the shuffle
    reduction), n % 64 != 0 a ragged last sweep; m in {1, 3, 5} leaves waves of the last block without a row."""
    _moe_prep(m, n, seed=100 * n + m, accumulate=bool((m + n) % 2), poison=not (m + n) % 2)


def test_moe_bwd_prep_more_rows_than_one_sweep(engine_lib):
    """Gap 2: 8195 rows are more than the 2048 blocks x 4 rows of the capped grid cover at once."""
    _moe_prep(8195, 24, seed=8195, accumulate=True)


@pytest.mark.parametrize("E,e", [(1, 0), (3, 0), (3, 1), (3, 2), (64, 0), (64, 31), (64, 63)])
def test_moe_bwd_prep_expert_columns(engine_lib, E, e):
    """prob and dp as column e of [m, E] tensors (strides E): the other experts' dp stay untouched."""
    for m in (1, 130):
        _moe_prep(m, 39, seed=E * 64 + e + m, E=E, e=e, accumulate=False, poison=True)


def test_moe_bwd_prep_strided(engine_lib):
    """dU and dX0_acc (and the inputs) as column slices of wider buffers, even and odd offsets; accumulate = 0 writes
    over NaN."""
    for col in (4, 1):
        lay = {k: (176, col) for k in ("dX", "X0", "U", "dU", "acc")}
        _moe_prep(130, 156, seed=col, E=4, e=2, accumulate=False, lay=lay, poison=True)
        _moe_prep(5, 156, seed=col + 10, E=4, e=3, accumulate=True, lay={"dU": (157, 0), "acc": (161, 5)})


# ============================================================================================================ softmax
def _softmax_rows_for(E, m, seed):
    """Rows that stress the max subtraction, cycled over the m rows: random O(1); all equal; one +1e4 among zeros; all
    -1e4; spread over +-80 (some probabilities underflow to exactly 0)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, E)).astype(f32)
    kind = np.arange(m) % 5
    x[kind == 1] = f32(3.25)
    hot = np.zeros((m, E), f32)
    hot[np.arange(m), rng.integers(0, E, m)] = f32(1e4)
    x[kind == 2] = hot[kind == 2]
    x[kind == 3] = f32(-1e4)
    x[kind == 4] = rng.uniform(-80, 80, (int((kind == 4).sum()), E)).astype(f32)
    return x


@pytest.mark.parametrize("E,m,strided", [(E, m, s) for E in (1, 2, 4, 5, 64) for m in (1, 257) for s in (False, True)] +
                         [(4, 524293, False)])
def test_softmax_rows_fwd_bwd(engine_lib, E, m, strided):
    """Gap 3: the gate softmax for 1 <= E <= 64 (the models only ever run E = 4 with O(1) logits); m = 524293 is more
    rows than the capped grid has threads.  Forward: assert_close_floor against NumPy, rows sum to 1 within E * 2^-23,
    everything finite and in [0, 1].  Backward dz_e = p_e (dp_e - sum_j p_j dp_j): the worst case of any summation
    order, (E + 4) u p_e (|dp_e| + sum_j |p_j dp_j|), plus one float32 denormal step (a relative bound cannot hold
    below the format's smallest spacing; the spread rows produce denormal p).  strided: ldx = E + 3, sentinel intact."""
    ops = _ops()
    x = _softmax_rows_for(E, m, seed=E * 7 + m % 1000)
    ld, col = (E + 3, 2) if strided else (E, 0)
    wx, wy = Wide((m, E), ld, col, a=x), Wide((m, E), ld, col)
    ops.softmax_rows(wx.v, out=wy.v)
    torch.cuda.synchronize()
    y = N_(wy.v)
    w64, w32 = both(X._softmax, x)
    assert np.all(np.isfinite(y)) and y.min() >= 0.0 and y.max() <= 1.0
    assert_close_floor(y, w64, w32, err_msg="softmax E=%d" % E)
    assert np.all(np.abs(y.astype(f64).sum(axis=1) - 1.0) <= E * 2.0 ** -23)
    if E > 1 and m > 4:
        assert (w32 == 0).any(), "the spread rows were meant to underflow somewhere"
    assert wx.intact() and wy.intact()
    # backward from the float32 probabilities of the same rows and a random dp
    rng = np.random.default_rng(E + m)
    p = w32.astype(f32)
    dp = rng.standard_normal((m, E)).astype(f32)
    wp, wd, wz = Wide((m, E), ld, col, a=p), Wide((m, E), ld, col, a=dp), Wide((m, E), ld, col)
    ops.softmax_rows_bwd(wp.v, wd.v, out=wz.v)
    torch.cuda.synchronize()
    dz = N_(wz.v)
    p6, d6 = p.astype(f64), dp.astype(f64)
    want = p6 * (d6 - (p6 * d6).sum(axis=1, keepdims=True))
    bound = (E + 4) * U * p6 * (np.abs(d6) + np.abs(p6 * d6).sum(axis=1, keepdims=True)) + 2.0 ** -149
    assert np.all(np.isfinite(dz))
    err = np.abs(dz - want)
    assert np.all(err <= bound), "dgate: worst err / bound %.3f" % float((err / bound).max())
    assert wp.intact() and wd.intact() and wz.intact()


# ==================================================================================================== sumsq, clip_scale
@pytest.mark.parametrize("n", [0, 1, 255, 256, 2049, 2 ** 21 + 1, 5_000_003])
def test_sumsq(engine_lib, n):
    """Gap 7: rec_sumsq against float64 sum(x * x) at rtol 1e-5 (the bar rec_sparse_rows_sumsq is held to), bit-identical
    across two calls (fixed reduction order).  The grid is ceil(n / 2048) capped at 1024 blocks: the last two sizes run
    the stride loop.  accumulate = 0 writes over NaN, accumulate = 1 adds to a known value; n = 0 leaves it as it was."""
    ops = _ops()
    rng = np.random.default_rng(n)
    # entries spanning 1e-3 .. 1e3 in magnitude, both signs
    x = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)) * rng.choice([-1.0, 1.0], n)).astype(f32)
    want = float((x.astype(f64) ** 2).sum())
    xt = T(x)
    outs = []
    for _ in range(2):
        out = torch.full((1,), float("nan"), device=DEV)
        ops.sumsq(xt, out, ops.Workspace(DEV), accumulate=False)
        outs.append(N_(out).copy())
    assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ: the reduction order is not fixed"
    if n == 0:
        assert outs[0][0] == 0.0
    else:
        np.testing.assert_allclose(float(outs[0][0]), want, rtol=1e-5)
    out = T(f32([1234.5]))
    ops.sumsq(xt, out, ops.Workspace(DEV), accumulate=True)
    if n == 0:
        assert float(out.item()) == 1234.5
    else:
        np.testing.assert_allclose(float(out.item()), want + 1234.5, rtol=1e-5)
    # O(1) entries: the common case of a gradient buffer
    y = rng.standard_normal(n).astype(f32)
    out = torch.full((1,), float("nan"), device=DEV)
    ops.sumsq(T(y), out, ops.Workspace(DEV))
    np.testing.assert_allclose(float(out.item()), float((y.astype(f64) ** 2).sum()), rtol=1e-5, atol=0.0)


@pytest.mark.parametrize("clip", [0.5, 10.0])
def test_clip_scale(engine_lib, clip):
    """Gap 7: scale = clip / max(sqrt(ss), clip) against the same expression in float32 NumPy, within 2 ulp; clip^2 is
    exact in float32 for both norms, so the scale is exactly 1.0 up to and including ss == clip^2 (ss = 0 too)."""
    ops = _ops()
    c2 = clip * clip
    assert float(f32(clip)) == clip and float(f32(c2)) == c2
    for ss in (0.0, 0.25 * c2, c2, 4.0 * c2, 1e30, 3.0 * c2, 1.7 * c2):
        out = torch.full((1,), float("nan"), device=DEV)
        ops.clip_scale(T(f32([ss])), clip, out)
        got = N_(out)[0]
        want = f32(clip) / np.maximum(np.sqrt(f32(ss)), f32(clip))
        assert want.dtype == f32
        assert abs(float(got) - float(want)) <= 2 * float(np.spacing(want)), (ss, got, want)
        if ss <= c2:
            assert got == f32(1.0)
        if ss == 4.0 * c2:
            assert got == f32(0.5)


# =========================================================================================== CrossNetV2 layer, one call
def v2_ref(x0, xl, W, b, dxn, old, accumulate=False, fold=False):
    """One layer of oracle/dcn_v2_ref.py cross_v2_forward / cross_v2_backward, with x_l independent of x_0 (the oracle's
    own layer 0 always has x_l = x_0, which would let swapped operands pass) — dtype-generic."""
    u = xl @ W + b
    out = dict(xnext=xl + x0 * u, u=u)
    du = dxn * x0
    acc = dxn * u + (old if accumulate else 0)
    out.update(dx0_acc=acc, dW=xl.T @ du, db=du.sum(axis=0), dxl=dxn + du @ W.T + (acc if fold else 0))
    return out


def _v2_inputs(B, d, seed):
    rng = np.random.default_rng(seed)
    x0, xl, dxn, old = (rng.standard_normal((B, d)).astype(f32) for _ in range(4))
    bound = np.sqrt(3.0 / d)                                     # DCN_V2Layer's initialisation of cross_layers.weight
    W = rng.uniform(-bound, bound, (d, d)).astype(f32)
    b = (rng.standard_normal(d) * 0.05).astype(f32)
    return x0, xl, W, b, dxn, old


def _v2_run(B, d, seed, accumulate=False, fold=False, lay=None, save_u=True, inplace=False, poison=None):
    """Forward then backward of one layer through ops.crossnet_v2_layer_{fwd,bwd}, a fresh Workspace per call (exactly
    the queried size).  -> dict of numpy results, plus the Wide operands."""
    ops = _ops()
    lay = lay or {}
    x0, xl, W, b, dxn, old = _v2_inputs(B, d, seed)
    w = {k: Wide((B, d), *lay.get(k, (d, 0)), a=a) for k, a in
         (("x0", x0), ("xl", xl), ("out", None), ("u", None), ("dxnext", dxn), ("acc", old), ("dxl", None))}
    if poison is None:
        poison = not accumulate
    if poison:
        w["acc"].v.fill_(float("nan"))
    Wt, bt = T(W), T(b)
    ops.crossnet_v2_layer_fwd(w["x0"].v, w["xl"].v, Wt, bt, ops.Workspace(DEV), out=w["out"].v,
                              u=w["u"].v if save_u else None)
    if not save_u:
        ops.crossnet_v2_layer_fwd(w["x0"].v, w["xl"].v, Wt, bt, ops.Workspace(DEV), out=torch.empty(B, d, device=DEV),
                                  u=w["u"].v)
    dW = torch.full((d, d), SENT, device=DEV)
    db = torch.full((d,), SENT, device=DEV)
    dst = w["dxnext"].v if inplace else w["dxl"].v
    r = ops.crossnet_v2_layer_bwd(w["x0"].v, w["xl"].v, Wt, w["u"].v, w["dxnext"].v, w["acc"].v, accumulate, fold, dW, db,
                                  ops.Workspace(DEV), out=dst)
    torch.cuda.synchronize()
    assert r.data_ptr() == dst.data_ptr()
    got = dict(xnext=N_(w["out"].v), u=N_(w["u"].v), dx0_acc=N_(w["acc"].v), dW=N_(dW), db=N_(db), dxl=N_(dst))
    for k, t in w.items():
        assert t.intact(), "columns outside the %s slice were written" % k
    want = both(v2_ref, x0, xl, W, b, dxn, old, accumulate=accumulate, fold=fold)
    return got, want, w


def _v2_check(got, want, tag):
    for k in ("xnext", "u", "dxl", "dx0_acc", "dW", "db"):
        close(got[k], want[0][k], want[1][k], "%s %s" % (tag, k))


@pytest.mark.parametrize("B,d", [(B, d) for B in (1, 3, 130, 4099) for d in (1, 7, 39, 156, 351)] + [(512, 1560)])
def test_v2_layer_grid(engine_lib, B, d):
    """rec_crossnet_v2_layer_{fwd,bwd}, every output against float64.  d in {1, 7, 39, 351} puts the backward on the
    scalar branch of cross_bwd_prep (gap 1) and the GEMMs on ragged tiles; B = 4099 is a ragged last row tile;
    (512, 1560) is the reference's own batch and width.  accumulate_dx0 = 0 writes over NaN (gap 4)."""
    got, want, _ = _v2_run(B, d, seed=B * 10000 + d)
    _v2_check(got, want, "v2 B%d d%d" % (B, d))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("fold", [False, True])
def test_v2_layer_accumulate_and_fold(engine_lib, accumulate, fold):
    """The four combinations of accumulate_dx0 and fold_dx0, at a float4 width and at a scalar one; accumulate_dx0 = 0
    runs over a NaN-filled dX0_acc (gap 4: garbage must not be read, also not by the fold)."""
    for B, d in ((130, 156), (67, 39)):
        got, want, _ = _v2_run(B, d, seed=d + 2 * accumulate + fold, accumulate=accumulate, fold=fold)
        _v2_check(got, want, "v2 acc%d fold%d d%d" % (accumulate, fold, d))


def test_v2_layer_without_saved_u(engine_lib):
    """U_saved = NULL in the forward: Xnext is the same bits as with it."""
    a, want, _ = _v2_run(130, 156, seed=5, save_u=True)
    b, _, _ = _v2_run(130, 156, seed=5, save_u=False)
    assert np.array_equal(a["xnext"], b["xnext"])
    _v2_check(b, want, "v2 no-u")


@pytest.mark.parametrize("B,d", [(130, 156), (64, 39), (3, 7)])
def test_v2_layer_layouts(engine_lib, B, d):
    """The non-stacked layout (Xnext = columns [16, 16 + d) of a [B, 16 + d] buffer) and a deliberately awkward one:
    x0, xl, out, u — and the gradient buffers — each at a different odd column offset of its own wider buffer.  Right
    results, and every column outside the slices keeps the sentinel."""
    got, want, _ = _v2_run(B, d, seed=B + d, lay={"out": (16 + d, 16)})
    _v2_check(got, want, "v2 non-stacked")
    lay = {"x0": (d + 9, 1), "xl": (d + 5, 3), "out": (d + 11, 5), "u": (d + 7, 7), "dxnext": (d + 3, 1),
           "acc": (d + 13, 9), "dxl": (d + 6, 3)}
    for accumulate, fold in ((False, True), (True, False)):
        got, want, _ = _v2_run(B, d, seed=B + d + 1, accumulate=accumulate, fold=fold, lay=lay)
        _v2_check(got, want, "v2 awkward layout")


@pytest.mark.parametrize("B,d", [(130, 156), (64, 156), (257, 351), (3, 7), (512, 1560)])
def test_v2_layer_bwd_in_place(engine_lib, B, d):
    """Gap 4: dXl given as the SAME tensor as dXnext (include/recengine.h allows it) equals the out-of-place result bit
    for bit — with and without the dX0_acc fold, at shapes whose dXl GEMM splits K (64 x 156) and does not."""
    for fold in (False, True):
        a, want, _ = _v2_run(B, d, seed=B ^ d, fold=fold, inplace=False)
        b, _, _ = _v2_run(B, d, seed=B ^ d, fold=fold, inplace=True)
        for k in ("dxl", "dx0_acc", "dW", "db"):
            assert np.array_equal(a[k], b[k]), "in place: %s differs" % k
        _v2_check(b, want, "v2 in place")


def test_v2_layer_empty_batch(engine_lib):
    """B = 0: both directions succeed and write nothing."""
    ops = _ops()
    d = 12
    e = lambda: torch.empty(0, d, device=DEV)
    W, b = T(np.ones((d, d), f32)), T(np.ones(d, f32))
    dW, db = torch.full((d, d), SENT, device=DEV), torch.full((d,), SENT, device=DEV)
    out = ops.crossnet_v2_layer_fwd(e(), e(), W, b, ops.Workspace(DEV), u=e())
    assert tuple(out.shape) == (0, d)
    ops.crossnet_v2_layer_bwd(e(), e(), W, e(), e(), e(), False, True, dW, db, ops.Workspace(DEV))
    torch.cuda.synchronize()
    assert bool((dW == SENT).all()) and bool((db == SENT).all())


# ========================================================================================== CrossNetMix layer, one call
def mix_ref(x0, xl, Um, Vm, Cm, bias, gw, gb, dxn, old, accumulate=False, fold=False):
    """One layer of oracle/dcn_v2_ref.py cross_mix_forward / cross_mix_backward with the E gating Linear(d, 1) layers as
    one [d, E] matrix (how the engine keeps them) and x_l independent of x_0 — dtype-generic."""
    E = Um.shape[0]
    prob = X._softmax(xl @ gw + gb)
    t1 = [np.tanh(xl @ Vm[e]) for e in range(E)]
    t2 = [np.tanh(t1[e] @ Cm[e].T) for e in range(E)]
    u = [t2[e] @ Um[e].T + bias for e in range(E)]
    xn = xl + sum(prob[:, e:e + 1] * (x0 * u[e]) for e in range(E))
    dp = np.stack([(dxn * x0 * u[e]).sum(axis=1) for e in range(E)], axis=1)
    dgate = prob * (dp - (prob * dp).sum(axis=1, keepdims=True))
    dxl = dxn.copy()
    acc = old.copy() if accumulate else np.zeros_like(old)
    gU, gV, gC = np.zeros_like(Um), np.zeros_like(Vm), np.zeros_like(Cm)
    gbias = np.zeros_like(bias)
    for e in range(E):
        do = dxn * prob[:, e:e + 1]
        du = do * x0
        acc = acc + do * u[e]
        gbias = gbias + du.sum(axis=0)
        gU[e] = du.T @ t2[e]
        dc = (du @ Um[e]) * (1 - t2[e] ** 2)
        gC[e] = dc.T @ t1[e]
        da = (dc @ Cm[e]) * (1 - t1[e] ** 2)
        gV[e] = xl.T @ da
        dxl = dxl + da @ Vm[e].T
    dxl = dxl + dgate @ gw.T + (acc if fold else 0)
    return dict(xnext=xn, t1=np.concatenate(t1, axis=1), t2=np.concatenate(t2, axis=1), prob=prob, dxl=dxl, dx0_acc=acc,
                gU=gU, gV=gV, gC=gC, gbias=gbias, g_gate_w=xl.T @ dgate, g_gate_b=dgate.sum(axis=0))


MIX_OUT = ("xnext", "t1", "t2", "prob", "dxl", "dx0_acc", "gU", "gV", "gC", "gbias", "g_gate_w", "g_gate_b")


def _mix_inputs(B, d, r, E, seed, v_scale=1.0, gate_scale=1.0, x_scale=0.5):
    """x_0, x_l ~ N(0, x_scale^2): at 0.5 the pre-activations x_l V_e have a standard deviation of about 0.7 and the
    float32 floor of every output stays below 1e-5 of its scale / 4 (close() asserts it)."""
    rng = np.random.default_rng(seed)
    x0, xl, dxn, old = (rng.standard_normal((B, d)).astype(f32) for _ in range(4))
    x0, xl = x0 * f32(x_scale), xl * f32(x_scale)
    sd = np.sqrt(2.0 / (d + r))                                  # DCN_V2Layer's initialisation of U / V / C / gating
    Um = (rng.standard_normal((E, d, r)) * sd).astype(f32)
    Vm = (rng.standard_normal((E, d, r)) * sd * v_scale).astype(f32)
    Cm = (rng.standard_normal((E, r, r)) * np.sqrt(1.0 / r)).astype(f32)
    bias = (rng.standard_normal(d) * 0.05).astype(f32)
    gbound = np.sqrt(6.0 / (d + 1)) * gate_scale
    gw = rng.uniform(-gbound, gbound, (d, E)).astype(f32)
    gb = (rng.standard_normal(E) * 0.05).astype(f32)
    return x0, xl, Um, Vm, Cm, bias, gw, gb, dxn, old


def _mix_run(B, d, r, E, seed, accumulate=False, fold=False, gate_old=None, lay=None, v_scale=1.0, gate_scale=1.0,
             x_scale=0.5):
    """Forward then backward of one layer through ops.crossnet_mix_layer_{fwd,bwd} (fresh Workspace per call).
    gate_old = (g_gate_w, g_gate_b) to accumulate into, None: accumulate_gate = 0 over NaN."""
    ops = _ops()
    lay = lay or {}
    inp = _mix_inputs(B, d, r, E, seed, v_scale, gate_scale, x_scale)
    x0, xl, Um, Vm, Cm, bias, gw, gb, dxn, old = inp
    w = {k: Wide((B, d), *lay.get(k, (d, 0)), a=a) for k, a in
         (("x0", x0), ("xl", xl), ("out", None), ("dxnext", dxn), ("acc", old), ("dxl", None))}
    if not accumulate:
        w["acc"].v.fill_(float("nan"))
    Ut, Vt, Ct, bt, gwt, gbt = (T(a) for a in (Um, Vm, Cm, bias, gw, gb))
    xn, t1, t2, prob = ops.crossnet_mix_layer_fwd(w["x0"].v, w["xl"].v, Ut, Vt, Ct, bt, gwt, gbt, ops.Workspace(DEV),
                                                  out=w["out"].v)
    full = lambda shape, v: torch.full(shape, v, dtype=torch.float32, device=DEV)
    gU, gV, gC, gbias = full((E, d, r), SENT), full((E, d, r), SENT), full((E, r, r), SENT), full((d,), SENT)
    if gate_old is None:
        ggw, ggb = full((d, E), float("nan")), full((E,), float("nan"))
    else:
        ggw, ggb = T(gate_old[0]), T(gate_old[1])

    def bwd():
        return ops.crossnet_mix_layer_bwd(w["x0"].v, w["xl"].v, Ut, Vt, Ct, bt, gwt, t1, t2, prob, w["dxnext"].v,
                                          w["acc"].v, accumulate, fold, gU, gV, gC, gbias, ggw, ggb,
                                          gate_old is not None, ops.Workspace(DEV), out=w["dxl"].v)
    bwd()
    torch.cuda.synchronize()
    got = dict(xnext=N_(xn), t1=N_(t1), t2=N_(t2), prob=N_(prob), dxl=N_(w["dxl"].v), dx0_acc=N_(w["acc"].v),
               gU=N_(gU), gV=N_(gV), gC=N_(gC), gbias=N_(gbias), g_gate_w=N_(ggw), g_gate_b=N_(ggb))
    for k, t in w.items():
        assert t.intact(), "columns outside the %s slice were written" % k
    want = both(mix_ref, *inp, accumulate=accumulate, fold=fold)
    if gate_old is not None:
        for wv, dt in zip(want, (f64, f32)):
            wv["g_gate_w"] = wv["g_gate_w"] + gate_old[0].astype(dt)
            wv["g_gate_b"] = wv["g_gate_b"] + gate_old[1].astype(dt)
    return got, want, bwd, (gU, gV, gC, gbias, ggw, ggb, w)


def _mix_check(got, want, tag, noisy=False):
    for k in MIX_OUT:
        close(got[k], want[0][k], want[1][k], "%s %s" % (tag, k), noisy=noisy)


@pytest.mark.parametrize("B,d,r,E", [(3, 7, 1, 1), (130, 39, 5, 3), (64, 24, 4, 64), (257, 351, 16, 4),
                                     (130, 156, 16, 4), (512, 1560, 256, 4)])
def test_mix_layer_grid(engine_lib, B, d, r, E):
    """Gap 5: rec_crossnet_mix_layer_{fwd,bwd} with E in {1, 3, 64}, r in {1, 5} (not multiples of 4), d = 351 (scalar
    glue, ragged tiles) and the reference's own d 1560 / r 256 / E 4 — every output and saved tensor against float64.
    accumulate_dx0 = 0 and accumulate_gate = 0 run over NaN.  E = 64 is one of the two named noisy cases (the gate
    gradients are sums of 64 cancelling terms): there the binding bound is printed, not asserted."""
    got, want, bwd, outs = _mix_run(B, d, r, E, seed=B + d + r + E, fold=True)
    _mix_check(got, want, "mix B%d d%d r%d E%d" % (B, d, r, E), noisy=E == 64)
    # a rerun of the backward on the same inputs leaves the same bits (fixed-order reductions: GEMM, rec_colsum)
    first = [N_(t).copy() for t in outs[:6]] + [N_(outs[6]["dxl"].v).copy(), N_(outs[6]["acc"].v).copy()]
    bwd()
    torch.cuda.synchronize()
    again = [N_(t) for t in outs[:6]] + [N_(outs[6]["dxl"].v), N_(outs[6]["acc"].v)]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes(), "the backward is not deterministic"


def test_mix_layer_saturated_tanh(engine_lib):
    """Gap 5: V scaled by 40, so that almost every t1 is beyond +-0.999: 1 - t^2 must come from the SAVED t (recomputing
    it from a rounded pre-activation would not reproduce it), and the gradients that vanish come out as (near) zeros,
    not NaN.  The second named noisy case: the binding bound is printed."""
    inp = _mix_inputs(130, 156, 16, 4, seed=40, v_scale=40.0, x_scale=1.0)
    t1 = np.tanh(inp[1].astype(f64) @ inp[3][0].astype(f64))
    assert float((np.abs(t1) > 0.999).mean()) > 0.9
    got, want, _, _ = _mix_run(130, 156, 16, 4, seed=40, v_scale=40.0, x_scale=1.0)
    _mix_check(got, want, "mix saturated", noisy=True)


def test_mix_layer_gate_with_spread(engine_lib):
    """Gap 3 inside the layer: gate weights scaled so that the logits span about +-60 and some probabilities are exactly
    0 — the gate gradient still matches."""
    got, want, _, _ = _mix_run(130, 156, 16, 4, seed=41, gate_scale=40.0)
    assert (want[1]["prob"] == 0).any() and (got["prob"] == 0).any()
    _mix_check(got, want, "mix gate spread")


def test_mix_layer_accumulate_gate(engine_lib):
    """Gap 5: accumulate_gate = 1 over known contents adds the layer's gate gradients to them (= 0 over NaN is what
    every other case runs); with accumulate_dx0 = 1 and without the fold."""
    rng = np.random.default_rng(9)
    B, d, r, E = 130, 39, 5, 3
    old = ((rng.standard_normal((d, E)) * 3).astype(f32), (rng.standard_normal(E) * 3).astype(f32))
    got, want, _, _ = _mix_run(B, d, r, E, seed=77, accumulate=True, fold=False, gate_old=old)
    _mix_check(got, want, "mix accumulate_gate")
    plain, _, _, _ = _mix_run(B, d, r, E, seed=77, accumulate=True, fold=False)
    assert np.abs(got["g_gate_w"] - plain["g_gate_w"] - old[0]).max() <= 1e-5 * np.abs(old[0]).max()


@pytest.mark.parametrize("B,d,r,E", [(130, 156, 16, 4), (3, 7, 1, 1), (64, 39, 5, 3)])
def test_mix_layer_layouts(engine_lib, B, d, r, E):
    """x0 / xl / out / dXnext / dX0_acc / dXl as column slices of wider buffers (the non-stacked layout at column 16, and
    odd offsets): right results, sentinel intact outside the slices."""
    got, want, _, _ = _mix_run(B, d, r, E, seed=B + E, fold=True, lay={"out": (16 + d, 16)})
    _mix_check(got, want, "mix non-stacked")
    lay = {"x0": (d + 9, 1), "xl": (d + 5, 3), "out": (d + 11, 5), "dxnext": (d + 3, 1), "acc": (d + 13, 9),
           "dxl": (d + 6, 3)}
    for accumulate, fold in ((False, True), (True, False)):
        got, want, _, _ = _mix_run(B, d, r, E, seed=B + E + 1, accumulate=accumulate, fold=fold, lay=lay)
        _mix_check(got, want, "mix awkward layout")


def test_mix_layer_empty_batch(engine_lib):
    ops = _ops()
    d, r, E = 12, 4, 3
    e = lambda: torch.empty(0, d, device=DEV)
    one = lambda *s: torch.ones(*s, device=DEV)
    xn, t1, t2, prob = ops.crossnet_mix_layer_fwd(e(), e(), one(E, d, r), one(E, d, r), one(E, r, r), one(d), one(d, E),
                                                  one(E), ops.Workspace(DEV))
    outs = [torch.full(s, SENT, device=DEV) for s in ((E, d, r), (E, d, r), (E, r, r), (d,), (d, E), (E,))]
    ops.crossnet_mix_layer_bwd(e(), e(), one(E, d, r), one(E, d, r), one(E, r, r), one(d), one(d, E), t1, t2, prob, e(),
                               e(), False, True, *outs, False, ops.Workspace(DEV))
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs)


# ======================================================================================== three-layer chains vs the oracle
def test_v2_three_layer_chain_vs_oracle_stack(engine_lib):
    """Three layers through the entry points, backward included, against oracle/dcn_v2_ref.py's stack functions:
    accumulate_dx0 / fold_dx0 driven as DCN_V2Layer.train_step drives them (first layer processed overwrites dX0_acc,
    the others add, layer 0 folds it into d x_0).  d = 351: the scalar glue branch (gap 1)."""
    ops = _ops()
    B, d, L = 257, 351, 3
    rng = np.random.default_rng(351)
    x0 = rng.standard_normal((B, d)).astype(f32)
    dout = rng.standard_normal((B, d)).astype(f32)
    bound = np.sqrt(3.0 / d)
    p = {}
    for i in range(L):
        p[P + "cross_layers.%d.weight" % i] = rng.uniform(-bound, bound, (d, d)).astype(f32)
        p[P + "cross_layers.%d.bias" % i] = (rng.standard_normal(d) * 0.05).astype(f32)
    ws = ops.Workspace(DEV)
    x0t = T(x0)
    Wt = [T(p[P + "cross_layers.%d.weight" % i]) for i in range(L)]
    bt = [T(p[P + "cross_layers.%d.bias" % i]) for i in range(L)]
    xs, us = [x0t], []
    for i in range(L):
        u = torch.empty(B, d, device=DEV)
        xs.append(ops.crossnet_v2_layer_fwd(x0t, xs[i], Wt[i], bt[i], ws, u=u))
        us.append(u)
    dW = [torch.full((d, d), SENT, device=DEV) for _ in range(L)]
    db = [torch.full((d,), SENT, device=DEV) for _ in range(L)]
    dx, acc, have = T(dout), torch.full((B, d), float("nan"), device=DEV), False
    for i in reversed(range(L)):
        dx = ops.crossnet_v2_layer_bwd(x0t, xs[i], Wt[i], us[i], dx, acc, have, i == 0, dW[i], db[i], ws)
        have = True
    torch.cuda.synchronize()

    def oracle(dt):
        q = {k: v.astype(dt) for k, v in p.items()}
        y, saved = X.cross_v2_forward(x0.astype(dt), q, L)
        dx0, g = X.cross_v2_backward(dout.astype(dt), x0.astype(dt), saved, q, L)
        return y, dx0, g
    (y64, dx64, g64), (y32, dx32, g32) = oracle(f64), oracle(f32)
    assert y64.dtype == f64 and y32.dtype == f32
    close(xs[-1], y64, y32, "v2 chain x_L")
    close(dx, dx64, dx32, "v2 chain d x_0")
    for i in range(L):
        for leaf, got in (("weight", dW[i]), ("bias", db[i])):
            k = P + "cross_layers.%d.%s" % (i, leaf)
            close(got, g64[k], g32[k], "v2 chain " + k)


def test_mix_three_layer_chain_vs_oracle_stack(engine_lib):
    """Three CrossNetMix layers through the entry points against the oracle's stack functions: the shared gating
    gradients are written by the first layer processed (accumulate_gate = 0 over NaN) and added to by the others, as
    DCN_V2Layer._cross_mix_backward drives them.  The oracle keeps the gates as E Linear(d, 1): gating.%d.weight [d, 1]
    are the columns of the engine's [d, E] matrix.  E = 3, r = 5 (gap 5)."""
    ops = _ops()
    B, d, r, E, L = 130, 39, 5, 3, 3
    rng = np.random.default_rng(3905)
    x0 = rng.standard_normal((B, d)).astype(f32)
    dout = rng.standard_normal((B, d)).astype(f32)
    sd = np.sqrt(2.0 / (d + r))
    p = {}
    for i in range(L):
        p[P + "U_list.%d" % i] = (rng.standard_normal((E, d, r)) * sd).astype(f32)
        p[P + "V_list.%d" % i] = (rng.standard_normal((E, d, r)) * sd).astype(f32)
        p[P + "C_list.%d" % i] = (rng.standard_normal((E, r, r)) * np.sqrt(1.0 / r)).astype(f32)
        p[P + "bias.%d" % i] = (rng.standard_normal((d, 1)) * 0.05).astype(f32)
    gbound = np.sqrt(6.0 / (d + 1))
    gw = rng.uniform(-gbound, gbound, (d, E)).astype(f32)
    gb = (rng.standard_normal(E) * 0.05).astype(f32)
    for e in range(E):
        p[P + "gating.%d.weight" % e] = gw[:, e:e + 1].copy()
        p[P + "gating.%d.bias" % e] = gb[e:e + 1].copy()
    ws = ops.Workspace(DEV)
    x0t, gwt, gbt = T(x0), T(gw), T(gb)
    par = [[T(p[P + "%s.%d" % (n, i)]) for n in ("U_list", "V_list", "C_list")] + [T(p[P + "bias.%d" % i].reshape(-1))]
           for i in range(L)]
    x, saved = x0t, []
    for i in range(L):
        xn, t1, t2, prob = ops.crossnet_mix_layer_fwd(x0t, x, *par[i], gwt, gbt, ws)
        saved.append((x, t1, t2, prob))
        x = xn
    full = lambda shape, v: torch.full(shape, v, dtype=torch.float32, device=DEV)
    grads = [[full((E, d, r), SENT), full((E, d, r), SENT), full((E, r, r), SENT), full((d,), SENT)] for _ in range(L)]
    ggw, ggb = full((d, E), float("nan")), full((E,), float("nan"))
    dx, acc, have = T(dout), full((B, d), float("nan")), False
    for i in reversed(range(L)):
        xl, t1, t2, prob = saved[i]
        dx = ops.crossnet_mix_layer_bwd(x0t, xl, *par[i], gwt, t1, t2, prob, dx, acc, have, i == 0, *grads[i], ggw, ggb,
                                        i != L - 1, ws)
        have = True
    torch.cuda.synchronize()

    def oracle(dt):
        q = {k: v.astype(dt) for k, v in p.items()}
        y, sv = X.cross_mix_forward(x0.astype(dt), q, L, E)
        dx0, g = X.cross_mix_backward(dout.astype(dt), x0.astype(dt), sv, q, L, E)
        g[P + "gating.weight"] = np.concatenate([g[P + "gating.%d.weight" % e] for e in range(E)], axis=1)
        g[P + "gating.bias"] = np.concatenate([g[P + "gating.%d.bias" % e] for e in range(E)])
        return y, dx0, g
    (y64, dx64, g64), (y32, dx32, g32) = oracle(f64), oracle(f32)
    assert y64.dtype == f64 and y32.dtype == f32
    close(x, y64, y32, "mix chain x_L")
    close(dx, dx64, dx32, "mix chain d x_0")
    for i in range(L):
        for j, n in enumerate(("U_list.%d", "V_list.%d", "C_list.%d", "bias.%d")):
            k = P + n % i
            close(grads[i][j], g64[k].reshape(tuple(grads[i][j].shape)), g32[k].reshape(tuple(grads[i][j].shape)),
                  "mix chain " + k)
    close(ggw, g64[P + "gating.weight"], g32[P + "gating.weight"], "mix chain gating.weight")
    close(ggb, g64[P + "gating.bias"], g32[P + "gating.bias"], "mix chain gating.bias")


# ============================================================================== gap 6: gradient strides the query never saw
def _plan_splits(lib, m, n, k, lda, ldb, ldc, ta, tb, epi):
    from paddlerec_amd import _lib
    sp = C.c_int32(0)
    g = _lib.GemmDesc(m, n, k, lda, ldb, ldc, ta, tb, epi, 0)
    assert lib.rec_gemm_plan_splits(C.byref(g), 0, C.byref(sp)) == 0
    return sp.value


def _vp(t):
    return C.c_void_p(t.data_ptr())


WIDE_CASES = [(64, 156, 176), (3, 7, 23)]


@pytest.mark.parametrize("B,d,wide", WIDE_CASES)
@pytest.mark.parametrize("which", ["dxl", "acc", "dxnext", "all"])
@pytest.mark.parametrize("named", [False, True])
def test_v2_bwd_wide_gradient_strides(engine_lib, B, d, wide, which, named):
    """Gap 6.  dXl / dX0_acc / dXnext as slices of a buffer WIDER than every stride of the descriptor, every output
    pre-filled with the sentinel, the workspace exactly bwd_bytes.  The contract of include/recengine.h: the call either
    returns 0 and every output is right, or returns a negative status and has written NOTHING.  named = True: the
    descriptor's ld_out names the wide stride (what ops.crossnet_v2_layer_bwd does) and the call must succeed.
    At 64 x 156 the dXl GEMM splits K (its partials are [splits][B][ld_dxl], which is what the query has to know);
    at 3 x 7 nothing splits."""
    from paddlerec_amd import _lib
    ops, L = _ops(), engine_lib
    splits = _plan_splits(L, B, d, d, d, d, wide, 0, 1, 7)
    if B == 64 and splits < 2:
        pytest.skip("the dXl GEMM %d x %d x %d at ldc %d no longer splits K (plan: %d splits)" % (B, d, d, wide, splits))
    x0, xl, W, b, dxn, old = _v2_inputs(B, d, seed=B + d)
    u = (xl.astype(f64) @ W.astype(f64) + b).astype(f32)
    is_wide = lambda k: which in (k, "all")
    w = {k: Wide((B, d), wide if is_wide(k) else d, 4 if is_wide(k) else 0, a=a)
         for k, a in (("dxnext", dxn), ("acc", None), ("dxl", None))}
    x0t, xlt, Wt, ut = T(x0), T(xl), T(W), T(u)
    dW, db = torch.full((d, d), SENT, device=DEV), torch.full((d,), SENT, device=DEV)
    ld = lambda k: w[k].buf.shape[1]
    desc = _lib.CrossV2Desc(B, d, d, d, max(ld("dxnext"), ld("acc"), ld("dxl")) if named else d, d)
    nb = C.c_size_t(0)
    assert L.rec_crossnet_v2_layer_workspace_bytes(C.byref(desc), None, C.byref(nb)) == 0
    wsp = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=DEV)
    rc = L.rec_crossnet_v2_layer_bwd(C.byref(desc), _vp(x0t), _vp(xlt), _vp(Wt), _vp(ut), _vp(w["dxnext"].v), ld("dxnext"),
                                     _vp(w["acc"].v), ld("acc"), 0, 1, _vp(w["dxl"].v), ld("dxl"), _vp(dW), _vp(db),
                                     _vp(wsp), C.c_size_t(nb.value), ops._stream())
    torch.cuda.synchronize()
    if named:
        assert rc == 0, L.rec_last_error()
    if rc == 0:
        want = both(lambda *a: v2_ref(*a, accumulate=False, fold=True), x0, xl, W, b, dxn, old)
        # the saved u handed in is the float64 product rounded once: the same tensor the float32 run computes within noise
        got = dict(dxl=N_(w["dxl"].v), dx0_acc=N_(w["acc"].v), dW=N_(dW), db=N_(db))
        for k in got:
            close(got[k], want[0][k], want[1][k], "v2 wide %s: %s" % (which, k))
        assert all(t.intact() for t in w.values())
    else:
        assert rc < 0
        assert w["dxl"].untouched() and w["acc"].untouched() and w["dxnext"].intact(), \
            "a refused call wrote a gradient buffer (status %d: %s)" % (rc, L.rec_last_error())
        assert bool((dW == SENT).all()) and bool((db == SENT).all()), "a refused call wrote dW / db"


@pytest.mark.parametrize("B,d,wide", WIDE_CASES)
@pytest.mark.parametrize("which", ["dxl", "acc", "dxnext", "all"])
@pytest.mark.parametrize("named", [False, True])
def test_mix_bwd_wide_gradient_strides(engine_lib, B, d, wide, which, named):
    """Gap 6 for rec_crossnet_mix_layer_bwd (r 16, E 4): the same all-or-nothing contract; the two GEMMs that write dXl
    run at ld_dxl."""
    from paddlerec_amd import _lib
    ops, L = _ops(), engine_lib
    r, E = 16, 4
    inp = _mix_inputs(B, d, r, E, seed=B + d + 1)
    x0, xl, Um, Vm, Cm, bias, gw, gb, dxn, old = inp
    ref64, ref32 = both(mix_ref, *inp, accumulate=False, fold=True)
    is_wide = lambda k: which in (k, "all")
    w = {k: Wide((B, d), wide if is_wide(k) else d, 4 if is_wide(k) else 0, a=a)
         for k, a in (("dxnext", dxn), ("acc", None), ("dxl", None))}
    ts = [T(a) for a in (x0, xl, Um, Vm, Cm, bias, gw, ref32["t1"], ref32["t2"], ref32["prob"])]
    outs = [torch.full(s, SENT, device=DEV) for s in ((E, d, r), (E, d, r), (E, r, r), (d,), (d, E), (E,))]
    ld = lambda k: w[k].buf.shape[1]
    desc = _lib.CrossMixDesc(B, d, r, E, d, d, max(ld("dxnext"), ld("acc"), ld("dxl")) if named else d)
    nb = C.c_size_t(0)
    assert L.rec_crossnet_mix_layer_workspace_bytes(C.byref(desc), None, C.byref(nb)) == 0
    wsp = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=DEV)
    rc = L.rec_crossnet_mix_layer_bwd(C.byref(desc), *[_vp(t) for t in ts], _vp(w["dxnext"].v), ld("dxnext"),
                                      _vp(w["acc"].v), ld("acc"), 0, 1, _vp(w["dxl"].v), ld("dxl"),
                                      *[_vp(t) for t in outs], 0, _vp(wsp), C.c_size_t(nb.value), ops._stream())
    torch.cuda.synchronize()
    if named:
        assert rc == 0, L.rec_last_error()
    if rc == 0:
        got = dict(dxl=N_(w["dxl"].v), dx0_acc=N_(w["acc"].v))
        got.update({k: N_(t) for k, t in zip(("gU", "gV", "gC", "gbias", "g_gate_w", "g_gate_b"), outs)})
        for k in got:
            close(got[k], ref64[k], ref32[k], "mix wide %s: %s" % (which, k))
        assert all(t.intact() for t in w.values())
    else:
        assert rc < 0
        assert w["dxl"].untouched() and w["acc"].untouched() and w["dxnext"].intact(), \
            "a refused call wrote a gradient buffer (status %d: %s)" % (rc, L.rec_last_error())
        assert all(bool((t == SENT).all()) for t in outs), "a refused call wrote a parameter gradient"


def test_wide_gradient_strides_through_ops(engine_lib):
    """Gap 6 through the Python wrappers: they name the widest gradient stride in the descriptor, so a fresh Workspace
    (exactly the queried size) carries a wide dXl / dX0_acc / dXnext at the K-splitting shape."""
    lay = {"dxnext": (176, 4), "acc": (176, 8), "dxl": (176, 12)}
    got, want, _ = _v2_run(64, 156, seed=6, fold=True, lay=lay)
    _v2_check(got, want, "v2 wide via ops")
    got, want, _, _ = _mix_run(64, 156, 16, 4, seed=6, fold=True, lay=lay)
    _mix_check(got, want, "mix wide via ops")
