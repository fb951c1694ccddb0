"""The glue and loss entry points of paddlerec_amd/ops.py that only layer tests used to reach, called directly on the GPU
against tests/glue_ref.py: bce_with_logits, the DMR tail glue, DIEN's attention features and masked softmax weighting,
record_gather, sgd_dense, copy_f32 and fill_uniform.

Tolerance, the project's rule (tests/mtl_checks.py, mind_checks.py), for every tensor: err = max|got - ref64| / max|ref64|,
bound max(8 x the float32 restatement's error on the same inputs, 1e-6); both errors are printed.  An output that is a copy or
ONE float32 operation must match bit for bit; nothing with two or more operations is held to that (the compiler may contract
it into an FMA).  Every kernel runs twice and the two results are compared bit for bit; every strided output is a view of a
NaN-filled wider buffer whose padding must still be NaN afterwards.

Shapes: the smallest that reach each path of a 256-thread block / 64-lane wave — see each test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32, F64 = np.float32, np.float64
SENTINEL = 7777                                  # what the padding of an int64 view holds


def _t(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _close(got, ref64, ref32, what):
    got = _n(got) if torch.is_tensor(got) else np.asarray(got)
    e, r = G.relerr(got.reshape(np.shape(ref64)), ref64), G.relerr(ref32, ref64)
    print("%-52s err %.3g  float32-ref err %.3g" % (what, e, r))
    assert e <= max(8 * r, 1e-6), (what, e, r)


def _exact(got, want, what):
    got = _n(got) if torch.is_tensor(got) else np.asarray(got)
    assert np.array_equal(_bits(got).reshape(np.shape(want)), _bits(want)), what


def _strided(a, pad):
    """a [rows, cols] as a view of a wider NaN-filled buffer -> (view, buffer)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _t(a)
    return buf[:, :a.shape[1]], buf


def _strided3(a, pad):
    """a [B, T, D] as a view with ONE row stride D + pad of a NaN-filled buffer -> (view, buffer [B*T, D + pad])."""
    B, T, D = a.shape
    v, buf = _strided(a.reshape(B * T, D), pad)
    return buf.view(B, T, D + pad)[:, :, :D], buf


def _out(rows, cols, pad):
    return _strided(np.full((rows, cols), np.nan, F32), pad)


def _pad_is_nan(buf, cols):
    return bool(torch.isnan(buf[:, cols:]).all())


def _twice(run):
    """run() -> a tuple of tensors, evaluated twice on fresh outputs: bit for bit the same -> the first."""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0))
    return a


# ---------------------------------------------------------------------------------------------------- bce_with_logits
PLANTED = (30.0, -30.0, 100.0, -100.0, 1e4, -1e4)
BCE_B = [1, 256, 257, 1000, 262144 + 513]       # one thread; one block = its own fold; the first fold; four blocks (one
#                                                 ragged); above the 1024-block cap: the grid-stride loop makes a second pass


@functools.lru_cache(maxsize=None)
def _bce_problem(B):
    rng = np.random.default_rng(B)
    z = rng.standard_normal(B).astype(F32)
    t = rng.integers(0, 2, B).astype(F32)
    t[::3] = rng.choice(np.array([0.3, 0.75, 0.5], F32), len(t[::3]))            # soft labels: the label is float32
    pos = None
    if B >= 256:
        pos = np.array([0, 63, 64, 200, B // 2, B - 1])                            # first and last lane, a wave edge, the tail
        z[pos] = PLANTED
        t[pos] = [0.0, 1.0, 0.3, 0.0, 1.0, 0.75]
    refs = {m: [G.bce(z, t, m, dt) for dt in (F64, F32)] for m in (0, 3 * B)}
    for arr in (z, t):
        arr.setflags(write=False)
    return z, t, pos, refs


@pytest.mark.parametrize("mul", [0, 3])
@pytest.mark.parametrize("B", BCE_B)
def test_bce_with_logits(engine_lib, B, mul):
    from paddlerec_amd import ops
    z, t, pos, refs = _bce_problem(B)
    r64, r32 = refs[mul * B]
    ws = ops.Workspace(DEV)
    pred, dz, loss = _twice(lambda: ops.bce_with_logits(_t(z).reshape(B, 1), _t(t).reshape(B, 1), ws, mean_over=mul * B))
    assert tuple(pred.shape) == (B, 1) and tuple(dz.shape) == (B, 1) and tuple(loss.shape) == (1,)
    what = "bce B=%d mean_over=%d " % (B, mul * B)
    for name, got, a, b in zip(("pred", "dz", "loss"), (pred, dz, loss), r64, r32):
        assert bool(torch.isfinite(got).all()), name
        _close(got, a, b, what + name)
    p = _n(pred).reshape(-1)
    assert p.min() >= 0.0 and p.max() <= 1.0
    if pos is not None:
        # float32 saturates: 1 + exp(-30) rounds to 1, exp(100) and exp(1e4) are above the largest float
        assert np.array_equal(p[pos[[0, 2, 4]]], np.ones(3, F32)) and np.array_equal(p[pos[[3, 5]]], np.zeros(2, F32))
    # sum(dz): a sum's round-off scales with sum|dz|, not with the (cancelling) sum itself
    scale = float(np.abs(r64[1]).sum())
    e = abs(float(_n(dz).astype(F64).sum()) - float(r64[1].sum())) / scale
    r = abs(float(r32[1].astype(F64).sum()) - float(r64[1].sum())) / scale
    print("%-52s err %.3g  float32-ref err %.3g" % (what + "sum(dz)", e, r))
    assert e <= max(8 * r, 1e-6), (e, r)


def test_bce_saturated_logits_cost_their_magnitude(engine_lib):
    """Each planted logit alone (B = 1, the loss IS its cost): on the wrong side of its label the cost is |z| to round-off,
    on the right side it is below 1e-12 — and finite either way (log(1 - sigmoid(z)) would be -inf there)."""
    from paddlerec_amd import ops
    ws = ops.Workspace(DEV)
    for z in PLANTED:
        for label, want in ((float(z < 0), abs(z)), (float(z > 0), 0.0)):
            pred, dz, loss = ops.bce_with_logits(_t(np.array([[z]], F32)), _t(np.array([[label]], F32)), ws)
            got = float(loss.item())
            print("bce z=%g label=%g loss %.9g" % (z, label, got))
            assert np.isfinite(got) and abs(got - want) <= max(1e-6 * want, 1e-12), (z, label, got)
            assert abs(float(dz.item()) - (float(pred.item()) - label)) <= 1e-6


# ---------------------------------------------------------------------------------------------------- DMR tail glue
TAIL = [(1, 1, 1), (3, 2, 2), (5, 50, 16), (2, 3, 160), (2, 2, 300), (300, 3, 4)]
# D = 2E reaches 320 and 600 (the d loop AND the e loop make a second and third pass over the 256 threads); B E is no multiple
# of 256 in the flat backward (and above one block: 300 x 4); T D lies below and above 256
TAIL_C = 7


@functools.lru_cache(maxsize=None)
def _tail_problem(B, T, E):
    rng = np.random.default_rng(B * 10000 + T * 100 + E)
    D = 2 * E
    n = lambda *s: rng.standard_normal(s).astype(F32)
    p = dict(hist=n(B, T, D), item_eb=n(B, D), uv=n(B, 2, E), V=n(TAIL_C, E), d_rel=n(B, 1), dU2=n(B, E), f1=n(B, T, D), f2=n(B, T, D),
             d_sum=n(B, D), d_prod=n(B, D), d_item_direct=n(B, D), d_ctx=n(B * T, D + 2), d_hist0=n(B, T, D))
    mm = rng.integers(0, 2, (B, 1)).astype(np.int64)
    if B > 2:
        mm[:3, 0] = [0, 1, 2]                                                    # 2: the kernel multiplies by float(mask)
    else:
        mm[B // 2] = 2
    cid = rng.integers(0, TAIL_C, B).astype(np.int64)
    clean = cid.copy()
    if B >= 3:
        cid[0], cid[B - 1] = -1, TAIL_C                                          # one out-of-range id at each end
    elif B == 2:
        cid[0] = -1 if T == 3 else TAIL_C
    p.update(match_mask=mm, cate_id=cid, clean_id=clean, bad=cid != clean)
    for v in p.values():
        v.setflags(write=False)
    return p


@pytest.mark.parametrize("B,T,E", TAIL)
def test_dmr_tail_fwd(engine_lib, B, T, E):
    from paddlerec_amd import ops
    p, D = _tail_problem(B, T, E), 2 * E
    hist, hbuf = _strided3(p["hist"], 3)
    item, ibuf = _strided(p["item_eb"], 5)
    V, _ = _strided(p["V"], 1)
    mbuf = torch.full((B, 2), SENTINEL, dtype=torch.int64, device=DEV)
    mbuf[:, :1] = _t(p["match_mask"])
    uv = _t(p["uv"])

    def run(ids, status):
        (hs, hs_b), (pr, pr_b), (rel, rel_b) = _out(B, D, 1), _out(B, D, 4), _out(B, 1, 2)
        U2 = ops.dmr_tail_fwd(hist, item, uv, mbuf[:, :1], V, _t(ids), hs, pr, rel, status)
        assert _pad_is_nan(hs_b, D) and _pad_is_nan(pr_b, D) and _pad_is_nan(rel_b, 1)
        return hs, pr, rel, U2

    status, clean_status = ops.new_status(DEV), ops.new_status(DEV)
    hs, pr, rel, U2 = _twice(lambda: run(p["cate_id"], status))
    assert _pad_is_nan(hbuf, D) and _pad_is_nan(ibuf, D) and bool((mbuf[:, 1] == SENTINEL).all())
    r64, r32 = (G.dmr_tail_fwd(p["hist"], p["item_eb"], p["uv"], p["match_mask"], p["V"], p["cate_id"], dt) for dt in (F64, F32))
    what = "tail fwd %s " % ((B, T, E),)
    for name, got, a, b in zip(("hist_sum", "prod", "rel_u2i"), (hs, pr, rel), r64, r32):
        _close(got, a, b, what + name)
    _exact(U2, p["uv"][:, 0] * p["match_mask"].astype(F32), what + "U2")          # one float32 product
    assert int(status.item()) == (G.REC_FLAG_INDEX_OOB if p["bad"].any() else 0) == r64[4]
    assert not _n(rel)[p["bad"]].any()                                             # V reads as zero there: exactly 0
    clean = run(p["clean_id"], clean_status)
    assert int(clean_status.item()) == 0
    ok = ~p["bad"]
    assert np.array_equal(_bits(_n(clean[2])[ok]), _bits(_n(rel)[ok])) and (B < 3 or _n(clean[2])[p["bad"]].all())


@pytest.mark.parametrize("B,T,E", TAIL)
def test_dmr_tail_bwd_match(engine_lib, B, T, E):
    from paddlerec_amd import ops
    p = _tail_problem(B, T, E)
    d_rel, _ = _strided(p["d_rel"], 2)
    V, _ = _strided(p["V"], 1)
    mbuf = torch.full((B, 3), SENTINEL, dtype=torch.int64, device=DEV)
    mbuf[:, :1] = _t(p["match_mask"])
    uv, cid, ok = _t(p["uv"]), _t(p["cate_id"]), ~p["bad"]
    for dU2 in (p["dU2"], None):
        def run():
            dvr, dvr_b = _out(B, E, 3)
            d_uv = ops.dmr_tail_bwd_match(None if dU2 is None else _t(dU2), d_rel, uv, mbuf[:, :1], V, cid, dvr)
            assert _pad_is_nan(dvr_b, E)
            return d_uv, dvr
        d_uv, dvr = (_n(x) for x in _twice(run))
        w32 = G.dmr_tail_bwd_match(dU2, p["d_rel"], p["uv"], p["match_mask"], p["V"], p["cate_id"], F32)
        what = "tail bwd_match %s dU2=%s " % ((B, T, E), dU2 is not None)
        # every output is one float32 product (or a zero)
        _exact(dvr, w32[1], what + "dV_rows")                                     # written for the out-of-range samples too
        _exact(d_uv[ok, 1], w32[0][ok, 1], what + "d_uv[:,1]")
        assert not d_uv[p["bad"], 1].any()
        if dU2 is None:
            assert not d_uv[:, 0].any()
        else:
            _exact(d_uv[:, 0], w32[0][:, 0], what + "d_uv[:,0]")
        w64 = G.dmr_tail_bwd_match(dU2, p["d_rel"], p["uv"], p["match_mask"], p["V"], p["cate_id"])
        _close(d_uv, w64[0], w32[0], what + "d_uv")
        _close(dvr, w64[1], w32[1], what + "dV_rows")


@pytest.mark.parametrize("B,T,E", TAIL)
def test_dmr_tail_bwd_hist(engine_lib, B, T, E):
    from paddlerec_amd import ops
    p, D = _tail_problem(B, T, E), 2 * E
    hsum = G.dmr_tail_fwd(p["hist"], p["item_eb"], p["uv"], p["match_mask"], p["V"], p["cate_id"])[0].astype(F32)
    ins = [_strided(a, k + 1)[0] for k, a in enumerate((p["d_sum"], p["d_prod"], p["item_eb"], hsum, p["d_item_direct"]))]
    cbuf = _strided(p["d_ctx"], 3)[1]
    d_ctx = cbuf[:, :D + 1]                                                      # [B*T, >= D]: only the first D columns count
    for f1, f2 in ((p["f1"], p["f2"]), (p["f1"], None), (None, p["f2"]), (None, None)):
        def run():
            dh, dh_b = _strided3(p["d_hist0"], 3)                                  # pre-filled: the kernel accumulates into it
            di, di_b = _out(B, D, 2)                                               # NaN: the kernel overwrites it
            ops.dmr_tail_bwd_hist(None if f1 is None else _t(f1), None if f2 is None else _t(f2), *ins, d_ctx, dh, di)
            assert _pad_is_nan(dh_b, D) and _pad_is_nan(di_b, D)
            return dh, di
        dh, di = _twice(run)
        r64, r32 = (G.dmr_tail_bwd_hist(f1, f2, p["d_sum"], p["d_prod"], p["item_eb"], hsum, p["d_item_direct"],
                                        p["d_ctx"][:, :D + 1], p["d_hist0"], dt) for dt in (F64, F32))
        what = "tail bwd_hist %s f1=%d f2=%d " % ((B, T, E), f1 is not None, f2 is not None)
        _close(dh, r64[0], r32[0], what + "d_hist")
        _close(di, r64[1], r32[1], what + "d_item")


def test_wrappers_refuse_what_their_kernels_cannot_address(engine_lib):
    """The kernels take one row stride per operand (or none): a view they cannot walk is refused in Python, before any launch —
    every output still holds its NaN fill afterwards and the status stays 0."""
    from paddlerec_amd import ops
    from paddlerec_amd._lib import RecError
    B, T, E = 3, 4, 2
    D = 2 * E
    p = _tail_problem(B, 2, E)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    uv, V, cid, mm = _t(p["uv"]), _t(p["V"]), _t(p["clean_id"]), _t(p["match_mask"])
    status = ops.new_status(DEV)
    bad_hist = {"last stride 2": z(B, T, 2 * D)[:, :, ::2], "batch stride (T + 1) rows": z(B, T + 1, D)[:, :T]}
    for why, hist in bad_hist.items():
        assert tuple(hist.shape) == (B, T, D)
        (hs, hs_b), (pr, pr_b), (rel, rel_b) = _out(B, D, 1), _out(B, D, 1), _out(B, 1, 1)
        with pytest.raises(RecError, match="hist must be"):
            ops.dmr_tail_fwd(hist, z(B, D), uv, mm, V, cid, hs, pr, rel, status)
        assert all(bool(torch.isnan(b).all()) for b in (hs_b, pr_b, rel_b)), why
    ops.dmr_tail_fwd(z(1, T, 2 * D)[:, :, :D], z(1, D), uv[:1], mm[:1], V, cid[:1], z(1, D), z(1, D), z(1, 1), status)   # B = 1: any
    dvr, dvr_b = _out(B, E, 1)
    with pytest.raises(RecError, match="V"):                                      # a V narrower than uv's rows
        ops.dmr_tail_bwd_match(None, z(B, 1), uv, mm, z(TAIL_C, E + 1)[:, :E - 1], cid, dvr)
    with pytest.raises(RecError, match="uv"):
        ops.dmr_tail_bwd_match(None, z(B, 1), z(B, 3, E), mm, V, cid, dvr)
    assert bool(torch.isnan(dvr_b).all())
    ws = ops.Workspace(DEV)
    with pytest.raises(RecError, match="labels"):                                 # fewer labels than logits
        ops.bce_with_logits(z(8, 1), z(7, 1), ws)
    with pytest.raises(RecError, match="gradients"):
        ops.sgd_dense(z(8), z(7), 0.1)
    rec, rows = z(5, 12), torch.zeros(4, dtype=torch.int64, device=DEV)
    ow, ow_b = _out(4, 8, 4)
    with pytest.raises(RecError, match="out_w"):                                  # out_w is written at i * D: no row stride
        ops.record_gather(rows, rec, 8, ow, z(4), status)
    with pytest.raises(RecError, match="out_w"):
        ops.record_gather(rows, rec, 8, z(3, 8), z(4), status)
    with pytest.raises(RecError, match="out_w1"):
        ops.record_gather(rows, rec, 8, z(4, 8), z(4, 2)[:, 0], status)
    assert bool(torch.isnan(ow_b).all()) and int(status.item()) == 0


# ---------------------------------------------------------------------------------------------------- DIEN attention pieces
@pytest.mark.parametrize("n,E", [(1, 1), (7, 3), (65, 4), (3, 128), (257, 12)])
def test_dien_att_feat(engine_lib, n, E):
    """n E from one thread to 13 blocks, ragged last blocks; the forward is four copies / single operations: bit for bit."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(n * 1000 + E)
    h, q, df, d0 = (rng.standard_normal(s).astype(F32) for s in ((n, E), (n, E), (n, 4 * E), (n, E)))
    feat, = _twice(lambda: (ops.dien_att_feat_fwd(_t(h), _t(q)),))
    assert tuple(feat.shape) == (n, 4 * E)
    for k, want in enumerate((h, q, h - q, h * q)):
        _exact(_n(feat)[:, k * E:(k + 1) * E], want, "att_feat fwd block %d" % k)
    b64, b32 = (G.att_feat_bwd(h, q, df, dt) for dt in (F64, F32))
    for acc in (True, False):
        def run():
            dh = _t(d0) if acc else torch.full((n, E), NAN, dtype=torch.float32, device=DEV)     # not read unless it accumulates
            return dh, ops.dien_att_feat_bwd(_t(h), _t(q), _t(df), dh, accumulate=acc)
        dh, dq = _twice(run)
        what = "att_feat bwd %s acc=%d " % ((n, E), acc)
        _close(dh, b64[0] + (d0 if acc else 0), (b32[0] + d0) if acc else b32[0], what + "d_hist")
        _close(dq, b64[1], b32[1], what + "d_q")


SOFTMAX = [(1, 1, 1), (3, 257, 4), (2, 513, 3), (2, 5, 128), (4, 513, 3)]
# T past one and two strides of the 256 threads, T E past the weighting loop's first pass; (4, 513, 3): an ordinary ragged row
# over three strides as well (with B = 2 the two special rows are all there is), and a row of moderate scores whose weights
# are all of one order (the wide rows are nearly one-hot: their sum hardly matters)


@functools.lru_cache(maxsize=None)
def _softmax_problem(B, T, E):
    """Row 0: fully masked, one constant score (both precisions then see T equal logits).  Row 1: one open position, the LAST,
    with (score + mask) * scale = +150 — exp(150) overflows float32 unless the maximum is subtracted.  Row 2 (and the one row
    of B = 1): ragged length T - 3, scores 300 N(0,1) sqrt(E), i.e. logits spread over hundreds.  Row 3: every position open,
    scores 2 N(0,1) sqrt(E)."""
    rng = np.random.default_rng(B * 10000 + T * 10 + E)
    scale = float(E) ** -0.5
    score = (300.0 * np.sqrt(E) * rng.standard_normal((B, T))).astype(F32)
    length = np.full(B, max(T - 3, 1))
    mask = np.where(np.arange(T)[None, :] < length[:, None], 0.0, -1e9).astype(F32)
    if B >= 2:
        mask[0], score[0] = -1e9, 5.0
        mask[1], mask[1, T - 1] = -1e9, 0.0
        score[1, T - 1] = 150.0 * np.sqrt(E)
    if B >= 4:
        mask[3], score[3] = 0.0, (2.0 * np.sqrt(E) * rng.standard_normal(T)).astype(F32)
    hist, dx, d0 = (rng.standard_normal((B, T, E)).astype(F32) for _ in range(3))
    for b in range(2 if B >= 2 else 0, min(B, 3)):
        x = (score[b].astype(F64) + mask[b]) * scale
        open_x = x[mask[b] == 0]
        assert T < 8 or (open_x.max() - open_x.min() > 200 and open_x.max() > 89)      # exp overflows without the maximum
    fw = [G.softmax_weight_fwd(score, mask, hist, scale, dt) for dt in (F64, F32)]
    w32 = fw[0][0].astype(F32)                     # the backward starts from the reference's own w: its error is its own
    bw = [G.softmax_weight_bwd(w32, hist, dx, scale, dt) for dt in (F64, F32)]
    out = dict(scale=scale, score=score, mask=mask, hist=hist, dx=dx, d0=d0, fw=fw, w32=w32, bw=bw)
    for v in (score, mask, hist, dx, d0, w32):
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("B,T,E", SOFTMAX)
def test_dien_softmax_weight_fwd(engine_lib, B, T, E):
    from paddlerec_amd import ops
    p = _softmax_problem(B, T, E)
    w, x_att = _twice(lambda: ops.dien_softmax_weight_fwd(_t(p["score"]), _t(p["mask"]), _t(p["hist"]), p["scale"]))
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(x_att).all())
    what = "softmax_weight fwd %s " % ((B, T, E),)
    _close(w, p["fw"][0][0], p["fw"][1][0], what + "w")
    _close(x_att, p["fw"][0][1], p["fw"][1][1], what + "x_att")
    wn = _n(w)
    assert np.abs(wn.astype(F64).sum(1) - 1).max() <= 2e-6 * max(1, T // 64)
    if B >= 2:
        assert (wn[0] == wn[0, 0]).all() and abs(float(wn[0, 0]) - 1.0 / T) <= 1e-6           # fully masked: uniform
        assert wn[1, T - 1] == 1.0 and not wn[1, :T - 1].any()                                 # one open position
    else:
        assert wn[0, 0] == 1.0


@pytest.mark.parametrize("B,T,E", SOFTMAX)
def test_dien_softmax_weight_bwd(engine_lib, B, T, E):
    from paddlerec_amd import ops
    p = _softmax_problem(B, T, E)
    for acc in (True, False):
        def run():
            dh = _t(p["d0"]) if acc else torch.full((B, T, E), NAN, dtype=torch.float32, device=DEV)
            return ops.dien_softmax_weight_bwd(_t(p["w32"]), _t(p["hist"]), _t(p["dx"]), p["scale"], dh, accumulate=acc), dh
        ds, dh = _twice(run)
        what = "softmax_weight bwd %s acc=%d " % ((B, T, E), acc)
        (s64, h64), (s32, h32) = p["bw"]
        _close(ds, s64, s32, what + "dscore")
        _close(dh, h64 + (p["d0"] if acc else 0), (h32 + p["d0"]) if acc else h32, what + "d_hist")


# ---------------------------------------------------------------------------------------------------- record_gather
GATHER = [(1, 4), (8, 12), (9, 12), (9, 13), (8, 13), (16, 20), (64, 68), (256, 260)]
# one float per lane because of D (1, 9) or because of the stride alone (8, 13); float4 per lane on 2, 4, 16 and 64 lanes
GATHER_N = 37


def _init_value(lib):
    return lambda seed, row, d, r: F32(lib.rec_ps_init_value_host(seed, row, d, r))


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("D,stride", GATHER)
def test_record_gather(engine_lib, D, stride, n):
    """Duplicate rows, one row -1 and one row N (n = 1: a second call on row N), a NaN payload in a record.  Where the float4
    route applies and the scalar one can take D (D <= 64) the same lookup runs again into an out_w that starts 4 bytes into
    its buffer: the scalar fallback, the same bits."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(D * 1000 + stride + n)
    N = GATHER_N
    rec = rng.standard_normal((N, stride)).astype(F32)
    rec.view(np.uint32)[3, 0], rec.view(np.uint32)[3, D] = 0x7FC00123, 0xFFC00456
    rows = rng.integers(0, N, n).astype(np.int64)
    rows[0] = 3
    clean = rows.copy()
    if n > 1:
        rows[5], rows[100], rows[200], rows[256] = -1, N, rows[7], rows[7]
        clean[200], clean[256] = rows[7], rows[7]
    bad = rows != clean
    want_w, want_w1, flag = G.record_gather(rows, rec, D)
    rec_d = _t(rec)

    def run(r, status, misaligned=False):
        flat = torch.full((n * D + 8,), NAN, dtype=torch.float32, device=DEV)
        off = 1 if misaligned else 0
        ow, ow1 = flat[off:off + n * D].view(n, D), torch.full((n,), NAN, dtype=torch.float32, device=DEV)
        assert ow.data_ptr() % 16 == 4 * off
        ops.record_gather(_t(r), rec_d, D, ow, ow1, status)
        assert bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(flat[off + n * D:]).all())
        return ow, ow1

    status, clean_status = ops.new_status(DEV), ops.new_status(DEV)
    ow, ow1 = _twice(lambda: run(rows, status))
    _exact(ow, want_w, "record_gather W %s" % ((D, stride, n),))
    _exact(ow1, want_w1, "record_gather W1")
    assert int(status.item()) == flag == (G.REC_FLAG_INDEX_OOB if bad.any() else 0)
    assert not _n(ow)[bad].any() and not _n(ow1)[bad].any()
    cw, cw1 = run(clean, clean_status)
    assert int(clean_status.item()) == 0
    _exact(cw, rec[clean, :D], "born rows")
    _exact(cw1, rec[clean, D], "born rows W1")
    if n == 1:
        s = ops.new_status(DEV)
        zw, zw1 = run(np.array([N], np.int64), s)
        assert int(s.item()) == G.REC_FLAG_INDEX_OOB and not zw.any() and not zw1.any()
    if D % 4 == 0 and stride % 4 == 0 and D <= 64:
        s = ops.new_status(DEV)
        mw, mw1 = run(rows, s, misaligned=True)
        _exact(mw, want_w, "misaligned out_w")
        _exact(mw1, want_w1, "misaligned out_w1")
        assert int(s.item()) == flag
    assert torch.equal(rec_d.view(torch.int32), _t(rec).view(torch.int32))


@pytest.mark.parametrize("D", [8, 9])
def test_record_gather_reads_unborn_rows_as_their_creation_values(engine_lib, D):
    """A table as paddlerec_amd/sharded.py builds its PsTable (kind 'deepfm', lazy creation on, the rank's row_mul / row_add).
    A third of the record lines are zero memory (the state float with them): their W1 is creation value element 0 of the
    GLOBAL row, bit for bit as rec_ps_init_value_host gives it (tests/test_slot_dnn.py pins that function to the oracle);
    W stays zero through ops.record_gather (init_dims 1) and is elements 1 + d when the lookup asks for init_embedx, which
    only the C entry point can.  The gather gives birth to nothing: the record lines are unchanged."""
    from paddlerec_amd import _lib, ops
    rng = np.random.default_rng(D)
    N, n, rngv, seed, mul, add = 41, 257, 0.05, 2 ** 63 + 77, 8, 5
    tab = ops.PsTable(N, D, torch.device(DEV), kind="deepfm", initial_range=rngv, embed_zero_init=False, seed=seed, row_mul=mul,
                      row_add=add)
    rec = rng.standard_normal(tuple(tab.rec.shape)).astype(F32)
    rec[:, tab.state_col] = 1.0
    rec[::3] = 0.0
    tab.rec.copy_(_t(rec))
    rows = rng.integers(0, N, n).astype(np.int64)
    rows[:3] = [0, 1, 3]
    unborn = rows % 3 == 0
    kw = dict(init_value=_init_value(engine_lib), state_col=tab.state_col, initial_range=rngv, seed=seed, row_mul=mul, row_add=add)
    status = ops.new_status(DEV)

    def run():
        ow, ow1 = (torch.full(s, NAN, dtype=torch.float32, device=DEV) for s in ((n, D), (n, 1)))
        ops.record_gather(_t(rows), tab.rec, D, ow, ow1, status, table=tab)
        return ow, ow1
    ow, ow1 = _twice(run)
    W, W1, _ = G.record_gather(rows, rec, D, **kw)
    _exact(ow, W, "lazy W")
    _exact(_n(ow1).reshape(-1), W1, "lazy W1")
    assert W1[unborn].all() and not W[unborn].any()                             # the reference itself: creation values, zeros
    assert W1[0] == engine_lib.rec_ps_init_value_host(seed, 0 * mul + add, 0, rngv) != \
        engine_lib.rec_ps_init_value_host(seed, 0, 0, rngv)                     # keyed by the global row
    # init_embedx: through the C entry point (ops.record_gather never asks for it)
    lz = _lib.LazyInit(tab.state_col, D + 1, rngv, seed, mul, add)
    ow, ow1 = (torch.full(s, NAN, dtype=torch.float32, device=DEV) for s in ((n, D), (n,)))
    rows_d = _t(rows)
    _lib.check(engine_lib.rec_record_gather(n, D, tab.rec.stride(0), N, ops._p(rows_d), ops._p(tab.rec), ops._p(ow), ops._p(ow1),
                                            C.byref(lz), ops._p(status), ops._stream()), "rec_record_gather")
    Wx, W1x, _ = G.record_gather(rows, rec, D, init_embedx=True, **kw)
    _exact(ow, Wx, "lazy W with init_embedx")
    _exact(ow1, W1x, "lazy W1 with init_embedx")
    assert Wx[unborn].all()
    # embed_zero_init (Paddle's default): no lazy values, the memory itself
    tab0 = ops.PsTable(N, D, torch.device(DEV), kind="deepfm", initial_range=rngv, row_mul=mul, row_add=add)
    tab0.rec.copy_(_t(rec))
    ow, ow1 = (torch.full(s, NAN, dtype=torch.float32, device=DEV) for s in ((n, D), (n,)))
    ops.record_gather(_t(rows), tab0.rec, D, ow, ow1, status, table=tab0)
    _exact(ow, rec[rows, :D], "zero-init W")
    _exact(ow1, rec[rows, D], "zero-init W1")
    assert int(status.item()) == 0
    assert torch.equal(tab.rec.view(torch.int32), _t(rec).view(torch.int32))


# ---------------------------------------------------------------------------------------------------- dense glue
SIZES = [1, 255, 257, 100003, 2048 * 256 + 513]       # sgd_dense and fill_uniform cap their grids at 2048 blocks: the last
#                                                       size makes the grid-stride loop take a second, ragged pass


@pytest.mark.parametrize("lr", [0.85, -1.0, 0.0])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_dense(engine_lib, n, lr):
    from paddlerec_amd import ops
    rng = np.random.default_rng(n)
    p, g = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)

    def run():
        buf = torch.full((n + 2,), NAN, dtype=torch.float32, device=DEV)
        buf[1:n + 1] = _t(p)
        ops.sgd_dense(buf[1:n + 1], _t(g), lr)
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[n + 1]))
        return (buf[1:n + 1],)
    got, = _twice(run)
    if lr == 0.0:
        _exact(got, p, "sgd_dense lr=0")                                         # p - 0 * g: unchanged, bit for bit
    else:
        _close(got, G.sgd_dense(p, g, lr), G.sgd_dense(p, g, lr, F32), "sgd_dense n=%d lr=%g" % (n, lr))
    if lr == -1.0:
        _exact(got, p + g, "sgd_dense lr=-1")                                    # -(-1 g) is exact: one float32 addition


@pytest.mark.parametrize("n", SIZES)
def test_copy_f32(engine_lib, n):
    from paddlerec_amd import ops
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)        # every bit pattern: NaN payloads, denormals
    bits[0] = 0x7FC00001
    src = _t(bits.view(np.int32)).view(torch.float32)
    buf = torch.zeros(n + 2, dtype=torch.float32, device=DEV)
    out = ops.copy_f32(buf[1:n + 1], src)
    assert out.data_ptr() == buf[1:].data_ptr()
    assert np.array_equal(_n(buf.view(torch.int32)).view(np.uint32), np.concatenate([[0], bits, [0]]).astype(np.uint32))
    out2 = ops.copy_f32(torch.zeros(n, dtype=torch.float32, device=DEV), src)
    assert torch.equal(out2.view(torch.int32), buf[1:n + 1].view(torch.int32))


@pytest.mark.parametrize("n", SIZES)
def test_fill_uniform(engine_lib, n):
    from paddlerec_amd import ops
    lo, hi, seed = -0.1, 0.3, 2 ** 63 + 12345

    def fill(m, s=seed, a=lo, b=hi):
        buf = torch.full((m + 2,), NAN, dtype=torch.float32, device=DEV)
        ops.fill_uniform(buf[1:m + 1], a, b, s)
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[m + 1]))
        return buf[1:m + 1]
    got, = _twice(lambda: (fill(n),))
    v = _n(got)
    assert v.min() >= F32(lo) and v.max() <= F32(hi)
    _close(got, G.splitmix_uniform(n, lo, hi, seed), G.splitmix_uniform(n, lo, hi, seed, F32), "fill_uniform n=%d" % n)
    other = _n(fill(n, seed + 1))
    assert n < 100 or (other != v).mean() > 0.99
    assert n > 100 or not np.array_equal(other, v)
    assert np.array_equal(_n(fill(n, seed, 0.25, 0.25)), np.full(n, 0.25, F32))                # lo == hi: the constant
    for m in (257, 100003):                                                       # value i depends on (seed, i) alone
        k = min(n, m)
        assert torch.equal(fill(m)[:k], got[:k])
    if n >= 100003:
        # uniform on [lo, hi): mean (lo + hi) / 2, deviation (hi - lo) / sqrt(12), each within 6 standard errors
        assert abs(float(v.astype(F64).mean()) - 0.1) < 2e-3 and abs(float(v.astype(F64).std()) - 0.4 / 12 ** 0.5) < 2e-3
