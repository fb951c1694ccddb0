"""Every dispatch_row_shape call site on every <VEC, LANES> leaf it can reach, and the three hand-rolled routers of the
sparse side (the lane-per-row lazy Adam, the multi-slot pool, the PS push) on every kernel they can launch.

A case runs ONE public entry point at a width D and a `how` (everything aligned, or one condition of the call site that
pushes a float4-eligible width onto the scalar leaf), and asserts
  * the route log (ops.route_log) holds exactly the note the Python restatement of the router predicts (_row_leaf_cases),
  * gathers and pools bit for bit against NumPy; updates and sums against float64 at the bar of the entry point's own test,
  * every float outside the D columns the call owns — wider rows, the bytes in front of an offset buffer, untouched rows —
    is still the sentinel / the old value, and the status word is what the reference says.
Shapes: 37 rows, ~70 lookups with duplicates (one row owns a third), a padding id and, where the entry point has a status
word, one id outside the table.  rec_segment_partials only acts on a row that owns >= REC_SEG_LONG = 128 lookups, so its
case (and only its) uses 230 lookups, 150 of them on one row.  The two completeness tests are plain CPU tests."""
import collections
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import _row_leaf_cases as RC
from helpers import assert_close_scaled

DEV = "cuda"
SENT = np.float32(-7777.25)
N, HOT = 37, 5
REL = 2e-5          # helpers.assert_close_scaled at 2e-5: the bar of the flen / gate / autofis kernel tests


# ------------------------------------------------------------------------------------------------ completeness (CPU)
def test_every_call_site_has_an_adapter():
    found = collections.Counter(f for f, _ in RC.call_sites())
    have = collections.Counter(s.file for s in RC.SITES)
    assert sum(found.values()) >= 20 and found == have, "call sites %r, adapters %r" % (dict(found), dict(have))
    assert sorted(RUNNERS) == sorted(s.name for s in RC.SITES)                  # ... and every adapter has its runner
    for s in RC.SITES:                                                          # the entry point is in that file
        src = open(RC.os.path.join(RC.REPO, "paddlerec_amd", "csrc", s.file)).read()
        assert ('extern "C" int %s(' % s.entry) in src or ("int %s_impl(" % s.entry[4:]) in src, s.name


@pytest.mark.parametrize("site", RC.SITES, ids=lambda s: s.name)
def test_case_table_reaches_every_leaf_of_the_rule(site):
    cases = site.cases()
    assert {site.predict(D, how) for D, how in cases} == site.reachable()
    assert {how for _, how in cases} == set(site.hows())                        # every condition of the site is used
    for c in site.conds:                                                        # ... on a width that float4 could take
        assert any(how == c and D % 4 == 0 for D, how in cases)
    full = {"rows<%d,%d>" % (v, l) for v in (1, 4) for l in (1, 2, 4, 8, 16, 32, 64)}
    assert RC.leaf(1024, 4, True) == "rows<4,256>" and RC.leaf(260, 4, True) == "rows<4,128>"
    assert RC.leaf(260, 1, True) is None and RC.leaf(65, 4) is None and RC.leaf(260, 4) is None
    if site.name == "emb_gather":
        assert site.reachable() == full
    if site.wide:
        assert {"rows<4,128>", "rows<4,256>"} <= site.reachable()


_PROBE = r"""
#include <stdarg.h>
#include <stdio.h>
#include "rec_common.h"
namespace rec {
void set_error(const char*, ...) {}
void route_note(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); }
}
int main() {
  for (int wide = 0; wide < 2; ++wide)
    for (int D = 1; D <= 1024; ++D)
      for (int stride : {4, 1}) {
        printf("%d %d %d|", wide, D, stride);
        int v = 0, l = 0;
        auto f = [&](auto v_, auto l_) -> int { v = decltype(v_)::value; l = decltype(l_)::value; return 0; };
        const int rc = wide ? rec::dispatch_row_shape_wide(D, stride, f) : rec::dispatch_row_shape(D, stride, f);
        printf("|%d %d %d\n", rc, v, l);
      }
  return 0;
}
"""


def test_python_rule_equals_the_router_of_rec_common_h(tmp_path):
    """The two dispatchers are host code: compiled into a stand-alone program they are walked over every width 1..1024 at
    an aligned and an odd stride (route_note replaced by one that prints).  The note, the instantiation the lambda
    receives and the refusals are what leaf() says."""
    import subprocess
    from paddlerec_amd import build
    src = tmp_path / "probe.cpp"
    src.write_text(_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call([build._hipcc(), "-std=c++17", "-O0", "--offload-arch=" + build.ARCH, "-I" + build.CSRC,
                           "-I" + RC.os.path.join(RC.REPO, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe]).decode().splitlines()
    assert len(lines) == 2 * 1024 * 2
    for line in lines:
        head, note, tail = line.split("|")
        wide, D, stride = (int(x) for x in head.split())
        rc, v, l = (int(x) for x in tail.split())
        want = RC.leaf(D, stride, bool(wide))
        assert note == (want or ""), line
        assert (rc, "rows<%d,%d>" % (v, l)) == (0, want) if want else (rc, v, l) == (-2, 0, 0), line


def test_restated_hand_rolled_routers():
    assert len({RC.adam_narrow_note(*c) for c in RC.ADAM_NARROW_CASES}) == 16
    notes = {RC.ms_note(S, D, 16 if D <= 16 else 68, al) for S, D, al in RC.MS_CASES}
    assert {"ms_lane<%d>" % d for d in (8, 9, 10, 11)} <= notes
    rows = {n for n in notes if n.startswith("ms_rows")}
    # every ms_rows kernel of the default environment: float4 lanes 1, 2, 4 and scalar lanes 1 .. 16 on all three
    # (NSW, WAVES) bands, the wider lane counts on <1, 4>.  ms_rows<4,4,2,8> is the one leaf the lane-per-id kernel takes
    # over whenever it is eligible (D 9 / 10, S > 8): test_multislot_pool_leaf reaches it under REC_MS_LANE=0
    assert len(RC.MS_LEAVES) == 28 and rows == RC.MS_LEAVES - {"ms_rows<4,4,2,8>"}
    off = {RC.ms_note(S, D, 16 if D <= 16 else 68, al, lane_on=False) for S, D, al in RC.MS_CASES}
    assert off == RC.MS_LEAVES


# ------------------------------------------------------------------------------------------------ device helpers
def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def al4(x):
    return (x + 3) // 4 * 4


def odd_above(x):
    return x + 1 if x % 2 == 0 else x + 2


def not4_above(x):
    return x + 1 if (x + 1) % 4 else x + 2


class Rows:
    """host [R, D] inside a sentinel-filled device buffer: row r at `off + r * stride` floats.  off 1 = the rows start 4
    bytes into the buffer; torch aligns the buffer itself far beyond 16 bytes."""

    def __init__(self, host, stride, off=0):
        host = np.asarray(host, np.float32)
        self.R, self.D, self.stride, self.off = host.shape[0], host.shape[1], stride, off
        assert stride >= self.D
        self.buf = torch.full((off + self.R * stride + 5,), float(SENT), dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[off:off + self.R * stride].view(self.R, stride)[:, :self.D]
        self.view.copy_(T(host))
        self.before = H(self.buf).copy()

    def got(self):
        return H(self.view).copy()

    def assert_rest_untouched(self, rows=None, what=""):
        """Everything but the D columns (of `rows`, default all rows) holds the bits it held after construction."""
        now, keep = H(self.buf), np.ones(self.buf.numel(), bool)
        r = np.arange(self.R) if rows is None else np.asarray(rows, np.int64).reshape(-1)
        keep[(self.off + r[:, None] * self.stride + np.arange(self.D)[None]).reshape(-1)] = False
        assert np.array_equal(now[keep], self.before[keep]), what + ": wrote outside its columns"


@contextlib.contextmanager
def lenient_tables(monkeypatch):
    """The Python wrappers refuse a float4-shaped table that is not 16-byte aligned before the library sees it; the C ABI
    takes it and routes to the scalar leaf.  That route is what a `*_off4` case of a table is about."""
    from paddlerec_amd import ops

    def chk(t, name):
        if t.dim() == 1:
            return 1, (t.stride(0) if t.numel() > 1 else 1)
        return t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])
    monkeypatch.setattr(ops, "_chk_table", chk)
    yield
    monkeypatch.undo()


def flat_ids(rng, n=70, oob=False, hot=None):
    ids = rng.integers(1, N, n).astype(np.int64)
    ids[rng.random(n) < (1 / 3 if hot is None else 0)] = HOT
    if hot:
        ids[rng.choice(n, hot, replace=False)] = HOT
    ids[3] = 0                                          # the padding id
    if oob:
        ids[11] = N + 2
    return ids


def table(rng, D, how, key="odd_stride", off_key=None, extra=4, scale=1.0):
    stride = odd_above(D) if how == key else al4(D) + extra
    return Rows(rng.uniform(-1, 1, (N, D)) * scale, stride, 1 if off_key and how == off_key else 0)


def rows_only(notes):
    return [n for n in notes if n.startswith("rows<")]


# ------------------------------------------------------------------------------------------------ gathers and pools
def run_emb_gather(ops, D, how, mp):
    rng = np.random.default_rng(D)
    ids = flat_ids(rng, oob=True)
    W = table(rng, D, how)
    gs = 2 * D + 1 if how == "out_pitch" else 2 * D + 4
    off = 1 if how == "out_off4" else 0
    out = torch.full((off + 35 * gs + 3,), float(SENT), dtype=torch.float32, device=DEV)
    with ops.route_log() as notes:
        _, status = ops.emb_gather(T(ids), W.view, padding_idx=0, out=out[off:], out_group=2, out_group_stride=gs)
    want = np.full(out.numel(), SENT, np.float32)
    Wh = W.got()
    for i, r in enumerate(ids):
        o = off + (i // 2) * gs + (i % 2) * D
        want[o:o + D] = Wh[r] if 0 < r < N else 0
    assert np.array_equal(H(out), want) and int(status.item()) == 1
    W.assert_rest_untouched([], "W")
    return notes


def _lod(rng, n=70, B=10):
    cut = np.sort(rng.integers(0, n + 1, B - 1))
    cut[4] = cut[3]                                     # an empty sample
    return np.concatenate([[0], np.sort(cut), [n]]).astype(np.int64)


def run_emb_gather_sumpool(ops, D, how, mp):
    rng = np.random.default_rng(100 + D)
    ids, lod, W = flat_ids(rng, oob=True), _lod(rng), table(rng, D, how)
    B = lod.size - 1
    out, counts, status = Rows(np.zeros((B, D)), D), torch.full((B + 2,), -9, dtype=torch.int32, device=DEV), ops.new_status(DEV)
    tid, tl = T(ids), T(lod)
    with ops.route_log() as notes:
        ops.check(ops.lib().rec_emb_gather_sumpool(B, D, W.stride, N, 0, ops._p(tid), ops._p(tl), ops._p(W.view),
                                                   ops._p(out.view), ops._p(counts), ops._p(status), ops._stream()))
    Wh, want, cnt = W.got(), np.zeros((B, D), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        for k in range(lod[b], lod[b + 1]):             # ascending k in float32, as the kernel adds
            if 0 < ids[k] < N:
                want[b] += Wh[ids[k]]
                cnt[b] += 1
    assert np.array_equal(out.got(), want) and np.array_equal(H(counts), np.concatenate([cnt, [-9, -9]]))
    assert int(status.item()) == 1
    out.assert_rest_untouched(None, "out tail")           # (every row of out is written; the tail is not)
    return notes


def run_emb_sumpool_bwd(ops, D, how, mp):
    rng = np.random.default_rng(200 + D)
    lod = _lod(rng)
    B = lod.size - 1
    d_out = rng.standard_normal((B, D)).astype(np.float32)
    rg = Rows(np.zeros((70, D)), D)
    td, tl = T(d_out), T(lod)
    with ops.route_log() as notes:
        ops.check(ops.lib().rec_emb_sumpool_bwd(B, D, ops._p(tl), ops._p(td), ops._p(rg.view), ops._stream()))
    assert np.array_equal(rg.got(), np.repeat(d_out, np.diff(lod), axis=0))
    rg.assert_rest_untouched(None, "row_grad tail")
    return notes


def run_record_gather(ops, D, how, mp):
    rng = np.random.default_rng(300 + D)
    rows = flat_ids(rng, oob=True)                      # row 0 is a row like any other here
    stride = odd_above(D + 1) if how == "odd_stride" else al4(D + 1) + 4
    rec = Rows(rng.uniform(-1, 1, (N, D + 1)), stride, 1 if how == "rec_off4" else 0)
    ow = Rows(np.zeros((70, D)), D, 1 if how == "out_off4" else 0)
    ow1 = torch.full((72,), float(SENT), dtype=torch.float32, device=DEV)
    status = ops.new_status(DEV)
    recv = rec.buf[rec.off:rec.off + N * stride].view(N, stride)
    with ops.route_log() as notes:
        ops.record_gather(T(rows), recv, D, ow.buf[ow.off:ow.off + 70 * D].view(70, D), ow1[:70], status)
    Rh = rec.got()
    ok = (rows >= 0) & (rows < N)
    want = np.where(ok[:, None], Rh[np.where(ok, rows, 0)], 0).astype(np.float32)
    assert np.array_equal(ow.got(), want[:, :D]) and np.array_equal(H(ow1)[:70], want[:, D])
    assert np.all(H(ow1)[70:] == SENT) and int(status.item()) == 1
    ow.assert_rest_untouched(None, "out_w")
    rec.assert_rest_untouched([], "rec")
    return notes


# ------------------------------------------------------------------------------------------------ merged-gradient sites
class Merge:
    """~70 lookups grouped by row, their gradient rows in a sentinel-filled buffer at the pitch / offset of `how`, and the
    float64 merged gradient of every row."""

    def __init__(self, ops, D, how, seed, grouped=True, hot=None, n=70):
        rng = self.rng = np.random.default_rng(seed)
        self.ids = flat_ids(rng, n, hot=hot)
        self.g = (rng.standard_normal((n, D)) * 1e-2).astype(np.float32)
        if grouped:
            pitch = not4_above(D) if how == "grad_pitch" else al4(D) + 4
            self.grad = Rows(self.g, pitch, 1 if how == "grad_off4" else 0)
            self.kw = dict(grad_group=1, grad_group_stride=pitch)
        else:                                           # an entry point whose gradient rows are contiguous [n, D]
            self.grad = Rows(self.g, D, 1 if how == "grad_off4" else 0)
            self.kw = {}
        self.tensor = self.grad.buf[self.grad.off:]
        self.ws = ops.Workspace(DEV)
        self.groups, self.status = ops.ids_group(T(self.ids), N, 0, self.ws)
        live = self.ids != 0
        self.merged = np.zeros((N, D), np.float64)
        np.add.at(self.merged, self.ids[live], self.g[live].astype(np.float64))
        self.rows = np.unique(self.ids[live])

    def done(self):
        assert int(self.status.item()) == 0
        self.grad.assert_rest_untouched([], "grad")


def assert_rows_close(got, want, rows, rtol=2e-5):
    """test_row_update_shapes_gpu.py: rtol 2e-5 with atol 2e-5 * max|ref| over the touched rows."""
    w = np.asarray(want, np.float64)[rows]
    np.testing.assert_allclose(np.asarray(got, np.float64)[rows], w, rtol=rtol, atol=rtol * float(np.abs(w).max()))


def adam_ref(P, M, V, g, t, lr, l2=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """_adam_ref of test_row_update_shapes_gpu.py on whole float64 arrays, with the L2Decay term g + l2 * w."""
    from test_row_update_shapes_gpu import _adam_ref
    g = torch.as_tensor(g + l2 * np.asarray(P, np.float64))
    rows = torch.arange(P.shape[0])
    p, m, v = _adam_ref(torch.as_tensor(P), torch.as_tensor(M), torch.as_tensor(V), rows, g, t, lr, b1, b2, eps)
    return p.numpy(), m.numpy(), v.numpy()


def run_segment_partials(ops, D, how, mp):
    m = Merge(ops, D, how, 400 + D, hot=150, n=230)
    spos, uniq, offs = m.groups.host()
    tiles = (230 + 63) // 64
    pp = torch.full((tiles * 2 * D,), float(SENT), dtype=torch.float32, device=DEV)
    with ops.route_log() as notes:
        got = ops.segment_partials(m.groups, m.tensor, D, out=pp, **m.kw)
    assert got is pp
    got, want = H(pp).reshape(tiles, 2, D), {}
    g64, nvalid = m.g.astype(np.float64), int(offs[-1])
    seg_of = lambda x: int(np.searchsorted(offs, x, side="right") - 1)
    for t in range(tiles):
        s, e = t * 64, min(t * 64 + 64, nvalid)
        if s >= nvalid:
            continue
        u0 = seg_of(s)
        b0, e0 = int(offs[u0]), int(offs[u0 + 1])
        if e0 - b0 >= 128:
            want[t, 0] = g64[spos[s:min(e, e0)]].sum(0)
        if e0 < e:
            u1 = seg_of(e - 1)
            if offs[u1 + 1] - offs[u1] >= 128:
                want[t, 1] = g64[spos[int(offs[u1]):e]].sum(0)
    assert len(want) >= 3 and {0, 1} == {slot for _, slot in want}, "the hot row must enter, span and leave tiles"
    scale = max(float(np.abs(w).max()) for w in want.values())
    for t in range(tiles):
        for slot in (0, 1):
            if (t, slot) in want:
                np.testing.assert_allclose(got[t, slot], want[t, slot], rtol=2e-5, atol=2e-5 * scale)
            else:
                assert np.all(got[t, slot] == SENT), "slot (%d, %d) is not a piece of a long segment" % (t, slot)
    m.done()
    return notes


def _state(rng, D, how, a_off_key=None):
    sstride = not4_above(D) if how == "state_pitch" else al4(D) + 4
    off = 1 if a_off_key and how == a_off_key else 0
    return (Rows(rng.standard_normal((N, D)) * 1e-2, sstride, off), Rows(rng.random((N, D)) * 1e-3, sstride, off))


def _adam_rows(ops, D, how, mp, every_row, l2=None, seed=500):
    m = Merge(ops, D, how, seed + D)
    P = table(m.rng, D, how)
    M, V = _state(m.rng, D, how)
    P0, M0, V0 = P.got(), M.got(), V.got()
    fn = ops.adam_rows_all if every_row else ops.sparse_adam_rows
    with ops.route_log() as notes:
        fn(m.groups, m.tensor, 1, P.view, M.view, V.view, 7, lr=1e-2, l2=l2, **m.kw)
    p, mm, v = adam_ref(P0, M0, V0, m.merged, 7, 1e-2, l2 or 0.0)
    rows = np.arange(N) if every_row else m.rows
    for got, want, r in ((P, p, "P"), (M, mm, "M"), (V, v, "V")):
        assert_rows_close(got.got(), want, rows)
        got.assert_rest_untouched(rows, r)
    m.done()
    return notes


def run_sparse_adam_rows(ops, D, how, mp):
    return _adam_rows(ops, D, how, mp, False)


def run_adam_rows_all(ops, D, how, mp):
    return _adam_rows(ops, D, how, mp, True)


def _adam_record(ops, D, how, mp, every_row):
    m = Merge(ops, D, how, 600 + D, grouped=False)
    rng = m.rng
    Dp = al4(D)
    voff = Dp + 1 if how == "v_off" else Dp
    stride = odd_above(D + 3) if how == "odd_stride" else al4(D + 3) + 4
    sstride = not4_above(voff + D) if how == "state_pitch" else al4(voff + D) + 4
    rec_h = rng.uniform(-1, 1, (N, D + 3)) * 0.1
    rec_h[:, D + 2] = np.abs(rec_h[:, D + 2]) * 1e-2
    mv_h = np.concatenate([rng.standard_normal((N, D)) * 1e-2, np.zeros((N, voff - D)), rng.random((N, D)) * 1e-3], 1)
    rec, mv = Rows(rec_h, stride, 1 if how == "rec_off4" else 0), Rows(mv_h, sstride, 1 if how == "mv_off4" else 0)
    rec0, mv0 = rec.got().astype(np.float64), mv.got().astype(np.float64)
    dz = (rng.standard_normal(70) * 1e-2).astype(np.float32)
    full = lambda r: r.buf[r.off:r.off + N * r.stride].view(N, r.stride)
    fn = ops.adam_record_all if every_row else ops.sparse_adam_record
    grad = m.tensor[:70 * D].view(70, D)
    with ops.route_log() as notes:
        fn(m.groups, grad, T(dz), 1, full(rec), full(mv), D, 5, lr=1e-2, v_offset=voff)
    g1 = np.zeros((N, 1), np.float64)
    live = m.ids != 0
    np.add.at(g1, m.ids[live], dz[live].astype(np.float64)[:, None])
    p, mm, v = adam_ref(rec0[:, :D], mv0[:, :D], mv0[:, voff:voff + D], m.merged, 5, 1e-2)
    p1, m1, v1 = adam_ref(rec0[:, D:D + 1], rec0[:, D + 1:D + 2], rec0[:, D + 2:D + 3], g1, 5, 1e-2)
    rows = np.arange(N) if every_row else m.rows
    rg, mg = rec.got(), mv.got()
    for got, want in ((rg[:, :D], p), (mg[:, :D], mm), (mg[:, voff:voff + D], v), (rg[:, D:D + 1], p1),
                      (rg[:, D + 1:D + 2], m1), (rg[:, D + 2:D + 3], v1)):
        assert_rows_close(got, want, rows)
    assert np.array_equal(mg[:, D:voff], mv0[:, D:voff].astype(np.float32))          # the gap in front of v
    rec.assert_rest_untouched(rows, "rec")
    mv.assert_rest_untouched(rows, "mv")
    m.done()
    return notes


def run_sparse_adam_record(ops, D, how, mp):
    return _adam_record(ops, D, how, mp, False)


def run_adam_record_all(ops, D, how, mp):
    return _adam_record(ops, D, how, mp, True)


def run_sparse_rows_sumsq(ops, D, how, mp):
    m = Merge(ops, D, how, 700 + D)
    out = T(np.array([0.25, SENT], np.float32))
    with ops.route_log() as notes:
        ops.sparse_rows_sumsq(m.groups, m.tensor, D, out, m.ws, accumulate=True, **m.kw)
    np.testing.assert_allclose(float(H(out)[0]), 0.25 + float((m.merged ** 2).sum()), rtol=1e-5)   # test_deepfm_gpu.py
    assert H(out)[1] == SENT
    m.done()
    return notes


def run_sparse_sgd_rows(ops, D, how, mp):
    m = Merge(ops, D, how, 800 + D)
    P = table(m.rng, D, how, off_key="p_off4")
    P0 = P.got()
    with lenient_tables(mp), ops.route_log() as notes:
        ops.sparse_sgd_rows(m.groups, m.tensor, P.view, 0.25, **m.kw)
    assert_rows_close(P.got(), P0 - 0.25 * m.merged, m.rows, rtol=1e-5)              # test_small_merge_shape_sweep
    P.assert_rest_untouched(m.rows, "P")
    m.done()
    return notes


def run_adagrad_rows(ops, D, how, mp):
    import flen_ref as FR
    m = Merge(ops, D, how, 900 + D)
    P = table(m.rng, D, how, off_key="p_off4")
    A = _state(m.rng, D, how, "a_off4")[1]
    P64, A64 = P.got().astype(np.float64), A.got().astype(np.float64)
    with lenient_tables(mp), ops.route_log() as notes:
        ops.adagrad_rows(m.groups, m.tensor, 1, P.view, A.view, 0.05, **m.kw)
    live = m.ids != 0
    FR.adagrad_rows(P64, A64, m.ids[live], m.g[live].astype(np.float64), 0.05)
    assert_close_scaled(P.got()[m.rows], P64[m.rows], REL, "P")
    assert_close_scaled(A.got()[m.rows], A64[m.rows], REL, "acc")
    P.assert_rest_untouched(m.rows, "P")
    A.assert_rest_untouched(m.rows, "A")
    m.done()
    return notes


# ------------------------------------------------------------------------------------------------ whole-layer lookups
B, S = 10, 7


def bs_ids(rng, oob=True, pad=True):
    ids = rng.integers(1, N, (B, S)).astype(np.int64)
    ids[rng.random((B, S)) < 1 / 3] = HOT
    if pad:
        ids[0, 3] = 0
    if oob:
        ids[1, 4] = N + 2
    return ids


def out_rows(cols, how, off_key, pitch_key, fill=None):
    ld = not4_above(cols) if how == pitch_key else al4(cols) + 4
    return Rows(np.zeros((B, cols)) if fill is None else fill, ld, 1 if how == off_key else 0)


def run_deepfm_fm_fwd(ops, D, how, mp):
    from oracle import deepfm_ref as R
    rng = np.random.default_rng(1000 + D)
    Dn = 3
    ids = bs_ids(rng)
    dense = rng.standard_normal((B, Dn)).astype(np.float32)
    W = table(rng, D, how, scale=0.3)
    W1 = (rng.uniform(-1, 1, (N, 1)) * 0.3).astype(np.float32)
    dw, dw1 = (rng.standard_normal((1, Dn, D)) * 0.1).astype(np.float32), (rng.standard_normal(Dn) * 0.1).astype(np.float32)
    F = S + Dn
    feat = Rows(np.zeros((B, F * D)), F * D, 1 if how == "feat_off4" else 0)
    y1, y2, se = (torch.empty(B, 1, device=DEV), torch.empty(B, 1, device=DEV), torch.empty(B, D, device=DEV))
    fv = feat.buf[feat.off:feat.off + B * F * D].view(B, F, D)
    with ops.route_log() as notes:
        _, _, _, _, status = ops.deepfm_fm_fwd(T(ids), T(dense), W.view, T(W1), T(dw), T(dw1), 0, out=(y1, y2, fv, se))
    ref_ids = np.where(ids >= N, 0, ids)                                    # outside the table: a zero row, as padding
    ry1, ry2, rfeat = R.fm_forward(ref_ids, dense, W1, W.got(), dw1, dw, 0)
    assert np.array_equal(feat.got().reshape(B, F, D), rfeat) and int(status.item()) == 1
    np.testing.assert_allclose(H(y1), ry1, rtol=1e-5, atol=2e-7)            # RTOL / ATOL of test_deepfm_gpu.py
    np.testing.assert_allclose(H(y2), ry2, rtol=1e-5, atol=2e-7 * D)
    np.testing.assert_allclose(H(se), rfeat.sum(1), rtol=1e-5, atol=2e-7)
    feat.assert_rest_untouched(None, "feat")
    W.assert_rest_untouched([], "W")
    return notes


def run_deepfm_fm_bwd(ops, D, how, mp):
    from oracle import deepfm_ref as R
    rng = np.random.default_rng(1100 + D)
    Dn = 3
    ids = bs_ids(rng, oob=False)
    dense = rng.standard_normal((B, Dn)).astype(np.float32)
    W = (rng.uniform(-1, 1, (N, D)) * 0.3).astype(np.float32)
    W1, dw = np.zeros((N, 1), np.float32), (rng.standard_normal((1, Dn, D)) * 0.1).astype(np.float32)
    _, _, feat = R.fm_forward(ids, dense, W1, W, np.zeros(Dn, np.float32), dw, 0)
    sum_emb = feat.sum(1, dtype=np.float32)
    dfeat = (rng.standard_normal(feat.shape) * 1e-3).astype(np.float32)
    dz = (rng.standard_normal((B, 1)) * 1e-3).astype(np.float32)
    rg = Rows(np.zeros((B * S, D)), D, 1 if how == "rg_off4" else 0)
    ddw, ddw1 = torch.empty(Dn, D, device=DEV), torch.empty(Dn, device=DEV)
    with ops.route_log() as notes:
        ops.deepfm_fm_bwd(T(dense), T(feat), T(sum_emb), T(dfeat), T(dz), T(dz), S, ops.Workspace(DEV),
                          out=(rg.buf[rg.off:rg.off + B * S * D].view(B * S, D), ddw, ddw1))
    ref = R.fm_backward(ids, dense, feat, dfeat, dz, dz, 0)
    np.testing.assert_allclose(rg.got(), ref["row_grad"], rtol=1e-5, atol=1e-9)          # test_fm_bwd_vs_oracle
    r64 = R.fm_backward(ids, dense.astype(np.float64), feat.astype(np.float64), dfeat.astype(np.float64),
                        dz.astype(np.float64), dz.astype(np.float64))
    np.testing.assert_allclose(H(ddw), r64["d_dense_w"][0], rtol=1e-5, atol=1e-5 * np.abs(r64["d_dense_w"]).max())
    np.testing.assert_allclose(H(ddw1), r64["d_dense_w_one"], rtol=1e-5, atol=1e-5 * np.abs(r64["d_dense_w_one"]).max())
    rg.assert_rest_untouched(None, "row_grad")
    return notes


GB = [0, 2, 3, S]


def run_flen_fwd(ops, D, how, mp):
    import flen_ref as FR
    rng = np.random.default_rng(1200 + D)
    ids = bs_ids(rng, pad=False)
    W = table(rng, D, how, off_key="w_off4")
    kmf = rng.uniform(0.5, 1.5, 3).astype(np.float32)
    X0, Hm = out_rows(S * D, how, "x0_off4", "x0_pitch"), out_rows(D, how, None, None)
    FW = torch.empty(B, 3 * D, device=DEV)
    with lenient_tables(mp), ops.route_log() as notes:
        _, _, _, status = ops.flen_fwd(T(ids), W.view, GB, T(kmf), out=(X0.view, Hm.view, FW))
    E, _ = FR.lookup(ids, W.got())
    fw, h = FR.flen_forward(E, GB, kmf)
    assert np.array_equal(X0.got(), E.reshape(B, -1).astype(np.float32)) and int(status.item()) == 1
    assert_close_scaled(H(FW), fw.reshape(B, -1), REL, "FW")
    assert_close_scaled(Hm.got(), h, REL, "h_mf")
    X0.assert_rest_untouched(None, "X0")
    Hm.assert_rest_untouched(None, "h_mf")
    W.assert_rest_untouched([], "W")
    return notes


def run_flen_bwd(ops, D, how, mp):
    import flen_ref as FR
    rng = np.random.default_rng(1300 + D)
    ids = bs_ids(rng, pad=False)
    kmf = rng.uniform(0.5, 1.5, 3).astype(np.float32)
    FW = rng.uniform(-1, 1, (B, 3, D)).astype(np.float32)
    dH = rng.standard_normal((B, D)).astype(np.float32)
    dX0 = rng.standard_normal((B, S, D)).astype(np.float32)
    g = out_rows(S * D, how, "g_off4", "g_pitch", dX0.reshape(B, -1))
    with ops.route_log() as notes:
        _, dk, status = ops.flen_bwd(T(ids), N, GB, T(kmf), T(FW.reshape(B, -1)), T(dH), g.view, ops.Workspace(DEV))
    live = (ids >= 0) & (ids < N)
    rg, wdk = FR.flen_backward(FW, GB, kmf, dH, dX0, live)
    assert_close_scaled(g.got(), rg.reshape(B, -1), REL, "row gradient")
    assert np.all(g.got().reshape(B, S, D)[~live] == 0)
    assert_close_scaled(H(dk), wdk, REL, "d kernel_mf")
    assert int(status.item()) == 1
    g.assert_rest_untouched(None, "g")
    return notes


def _gate_lookup(ids, Wh):
    live = (ids > 0) & (ids < N)
    return Wh[np.where(live, ids, 0)].astype(np.float64) * live[..., None], live


def run_gate_emb_fwd(ops, D, how, mp):
    import gatenet_ref as GR
    rng = np.random.default_rng(1400 + D)
    ids = bs_ids(rng)
    W = table(rng, D, how, off_key="w_off4")
    gw = rng.uniform(-1, 1, S).astype(np.float32)
    out = out_rows(S * D, how, "out_off4", "out_pitch")
    with lenient_tables(mp), ops.route_log() as notes:
        _, status = ops.gate_emb_fwd(T(ids), W.view, T(gw), padding_idx=0, out=out.view)
    e, live = _gate_lookup(ids, W.got())
    want, _, _ = GR.gate_emb_forward(e, gw)
    assert_close_scaled(out.got(), want.reshape(B, -1), REL, "out")
    assert np.all(out.got().reshape(B, S, D)[~live] == 0) and int(status.item()) == 1
    out.assert_rest_untouched(None, "out")
    W.assert_rest_untouched([], "W")
    return notes


def run_gate_emb_bwd(ops, D, how, mp):
    import gatenet_ref as GR
    rng = np.random.default_rng(1500 + D)
    ids = bs_ids(rng)
    W = table(rng, D, how, off_key="w_off4")
    gw = rng.uniform(-1, 1, S).astype(np.float32)
    g0 = rng.standard_normal((B, S, D)).astype(np.float32)
    g = out_rows(S * D, how, "g_off4", "g_pitch", g0.reshape(B, -1))
    with lenient_tables(mp), ops.route_log() as notes:
        _, dwt, status = ops.gate_emb_bwd(T(ids), W.view, T(gw), g.view, ops.Workspace(DEV), padding_idx=0)
    e, live = _gate_lookup(ids, W.got())
    de, dw = GR.gate_emb_backward(e, gw, g0 * live[..., None])
    assert_close_scaled(g.got(), (de * live[..., None]).reshape(B, -1), REL, "d e")
    assert np.all(g.got().reshape(B, S, D)[~live] == 0)
    assert_close_scaled(H(dwt), dw, REL, "d w_s")
    assert int(status.item()) == 1
    g.assert_rest_untouched(None, "g")
    W.assert_rest_untouched([], "W")
    return notes


def _autofis(ops, D, how, mp, training):
    import autofis_ref as AR
    rng = np.random.default_rng(1600 + D)
    ids = bs_ids(rng, pad=False)
    V = table(rng, D, how, off_key="v_off4")
    W1 = rng.uniform(-1, 1, (N, 1)).astype(np.float32)
    cols, rows = AR.generate_pairs(S)
    P = len(cols)
    gamma = (1.0 + 0.2 * rng.standard_normal(P)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(P)).astype(np.float32)
    mask = rng.uniform(0.3, 0.9, P).astype(np.float32)
    mask[::5] = 0.0
    rm0, rv0 = (0.3 * rng.standard_normal(P)).astype(np.float32), (0.5 + rng.random(P)).astype(np.float32)
    rm, rv = T(rm0), T(rv0)
    X0 = out_rows(S * D, how, "x0_off4", "x0_pitch")
    L = Rows(np.zeros((B, P)), P + 3, 1)
    pairs = ops.AutofisPairs(cols, rows, S, DEV)
    with lenient_tables(mp), ops.route_log() as notes:
        _, s, Lr, sm, si, status = ops.autofis_fwd(T(ids), V.view, T(W1), pairs, T(gamma), T(beta), T(mask), rm, rv,
                                                   ops.Workspace(DEV), training, out=(X0.view, L.view))
    xv, _ = AR.lookup(ids, V.got())
    xw, _ = AR.lookup(ids, W1)
    assert np.array_equal(X0.got(), xv.reshape(B, -1).astype(np.float32)) and int(status.item()) == 1
    if training:
        ws, L64, mean, var, invstd = AR.pair_forward(xv, xw[..., 0], cols, rows, gamma, beta, mask)
        assert_close_scaled(L.got(), L64, REL, "L")
        assert_close_scaled(H(sm), mean, REL, "mean")
        assert_close_scaled(H(si), invstd, REL, "invstd")
        assert_close_scaled(H(rm), 0.9 * rm0 + 0.1 * mean, REL, "running mean")
        assert_close_scaled(H(rv), 0.9 * rv0 + 0.1 * var, REL, "running var")
        L.assert_rest_untouched(None, "L")
    else:
        ws = AR.pair_forward(xv, xw[..., 0], cols, rows, gamma, beta, mask, rm0, rv0)[0]
        assert Lr is None and np.all(H(L.buf) == L.before)                       # eval without want_L: L is not written
        assert np.array_equal(H(rm), rm0) and np.array_equal(H(rv), rv0)
    assert_close_scaled(H(s), ws, REL, "s")
    X0.assert_rest_untouched(None, "X0")
    V.assert_rest_untouched([], "V")
    return notes


def run_autofis_fwd_eval(ops, D, how, mp):
    return _autofis(ops, D, how, mp, False)


def run_autofis_fwd_train(ops, D, how, mp):
    return _autofis(ops, D, how, mp, True)


RUNNERS = {n[4:]: f for n, f in list(globals().items()) if n.startswith("run_") and callable(f)}
CASES = [pytest.param(s.name, D, how, id="%s-D%d-%s" % (s.name, D, how), marks=pytest.mark.gpu)
         for s in RC.SITES for D, how in s.cases()]


@pytest.fixture(scope="module")
def ops(engine_lib):
    from paddlerec_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.mark.parametrize("site,D,how", CASES)
def test_row_leaf(ops, monkeypatch, site, D, how):
    notes = RUNNERS[site](ops, D, how, monkeypatch)
    assert rows_only(notes) == [RC.BY_NAME[site].predict(D, how)], (site, D, how, notes)


# ------------------------------------------------------------------------------------------------ lane-per-row lazy Adam
V4_OFF = ("p_stride", "state_stride", "p_off4", "m_off4", "v_off4")     # each host condition that clears V4 (sparse_update.hip)


def _narrow_adam(ops, mp, D, unaligned, l2):
    """One lane-per-row Adam call; unaligned: None (float4 row access) or the one V4_OFF condition that forbids it."""
    how = "vec" if D % 4 else "grad_pitch"
    m = Merge(ops, D, how, 2000 + D)
    rng = m.rng
    stride = odd_above(D) if unaligned == "p_stride" else al4(D) + 4
    sstride = not4_above(D) if unaligned == "state_stride" else al4(D) + 8
    off = lambda k: 1 if unaligned == k else 0
    P, M, V = (Rows(rng.uniform(-1, 1, (N, D)), stride, off("p_off4")),
               Rows(rng.standard_normal((N, D)) * 1e-2, sstride, off("m_off4")),
               Rows(rng.random((N, D)) * 1e-3, sstride, off("v_off4")))
    P0, M0, V0 = P.got(), M.got(), V.got()
    with lenient_tables(mp), ops.route_log() as notes:
        ops.sparse_adam_rows(m.groups, m.tensor, 1, P.view, M.view, V.view, 3, lr=1e-2, l2=0.01 if l2 else None, **m.kw)
    assert notes == [RC.adam_narrow_note(D, unaligned is None, l2)]
    p, mm, v = adam_ref(P0, M0, V0, m.merged, 3, 1e-2, 0.01 if l2 else 0.0)
    for got, want, name in ((P, p, "P"), (M, mm, "M"), (V, v, "V")):
        assert_rows_close(got.got(), want, m.rows)
        got.assert_rest_untouched(m.rows, name)
    m.done()


@pytest.mark.gpu
@pytest.mark.parametrize("D,v4,l2", RC.ADAM_NARROW_CASES)
def test_narrow_adam_leaf(ops, monkeypatch, D, v4, l2):
    """rec_sparse_adam_rows / rec_sparse_adam_rows_l2 on rows without float4 groups, D 1..16: NV = ceil(D / 4) x float4
    row access (strides multiples of 4 and P / M / V 16-byte aligned) or not x with / without the decay term.  A width that
    is a multiple of 4 only gets here when its gradient rows cannot be read as float4: their pitch is then no multiple of 4.
    The V4 = 0 cases walk the five conditions that clear it, one per width."""
    _narrow_adam(ops, monkeypatch, D, None if v4 else V4_OFF[D % len(V4_OFF)], l2)


@pytest.mark.gpu
@pytest.mark.parametrize("unaligned", V4_OFF)
@pytest.mark.parametrize("D", [5, 12])
def test_narrow_adam_every_condition_clears_v4(ops, monkeypatch, D, unaligned):
    """Aligned and unaligned P / M / V: an odd P row stride, a state stride that is no multiple of 4, and P, M or V starting
    4 bytes into its buffer each send the call to the scalar-access kernel, at a ragged width and at a multiple of 4."""
    _narrow_adam(ops, monkeypatch, D, unaligned, False)


# ------------------------------------------------------------------------------------------------ multi-slot pool
def _ms_problem(rng, S, nb=6):
    """nb samples x S slots, 0..4 values per (slot, sample) with duplicates, a padding id and one id outside the table."""
    lens = rng.integers(0, 5, (S, nb))
    lod = np.concatenate([np.zeros((S, 1), np.int64), np.cumsum(lens, 1)], 1)
    base = np.concatenate([[0], np.cumsum(lod[:, -1])]).astype(np.int64)
    vals = rng.integers(1, N, int(base[-1])).astype(np.int64)
    vals[rng.random(vals.size) < 1 / 3] = HOT
    vals[1] = 0
    vals[vals.size // 2] = N + 2
    return vals, lod.astype(np.int64), base


def _ms_run(ops, S, D, aligned, seed):
    from oracle import slot_dnn_ref as M
    rng = np.random.default_rng(seed)
    vals, lod, base = _ms_problem(rng, S)
    nb = lod.shape[1] - 1
    stride = (16 if D <= 16 else al4(D) + 4) if aligned else odd_above(D)
    W = Rows(rng.uniform(-1, 1, (N, D)), stride)
    mb = ops.MultislotBatch(T(vals), T(lod), T(base))
    ld = S * D + 5
    out = torch.full((nb, ld), float(SENT), dtype=torch.float32, device=DEV)
    with ops.route_log() as notes:
        _, counts, seg, rows, status = ops.multislot_sumpool(mb, W.view, padding_idx=0, out=out)
    # the statement has no ids outside the table: the kernels flag such an id and then treat it as the padding id (no
    # row added, not counted, rows_out = padding_idx), so the statement gets it as one
    want, cnt, wseg, wrows = M.multislot_sumpool(np.where(vals >= N, 0, vals), lod, base, W.got(), 0, 0)
    got = H(out)
    np.testing.assert_allclose(got[:, :S * D], want, rtol=1e-5, atol=1e-6)     # test_multislot_sumpool_vs_oracle
    assert np.all(got[:, S * D:] == SENT)
    assert np.array_equal(H(counts), cnt) and int(status.item()) == 1
    assert np.array_equal(H(seg)[:vals.size], wseg) and np.array_equal(H(rows)[:vals.size], wrows)
    W.assert_rest_untouched([], "W")
    return notes, stride


@pytest.mark.gpu
@pytest.mark.parametrize("S,D,aligned", RC.MS_CASES)
def test_multislot_pool_leaf(ops, monkeypatch, S, D, aligned):
    """Against the pool statement of tests/test_slot_dnn.py (oracle/slot_dnn_ref.py) at that test's bar — the kernels sum
    a segment by a scan, not left to right — with counts, segments and rows exact, on the kernel the restated router
    names; the lane-per-id widths again with REC_MS_LANE=0 (read per call), which must land on the row kernels."""
    monkeypatch.delenv("REC_MS_LANE", raising=False)
    notes, stride = _ms_run(ops, S, D, aligned, 3000 + 31 * S + D)
    assert notes == [RC.ms_note(S, D, stride)]
    if notes[0].startswith("ms_lane"):
        monkeypatch.setenv("REC_MS_LANE", "0")
        notes, stride = _ms_run(ops, S, D, aligned, 3000 + 31 * S + D)
        assert notes == [RC.ms_note(S, D, stride, lane_on=False)] and notes[0].startswith("ms_rows<4,")


# ------------------------------------------------------------------------------------------------ PS push
PS_CASES = [  # name, kind, looked-up width D, layout override (embed_off, embedx_off, embedx_dim, stat_off) | None, grad pitch, note
    ("narrow4", "slot", 4, None, None, "ps_narrow<4>"), ("narrow8", "slot", 8, None, None, "ps_narrow<8>"),
    ("narrow12", "slot", 12, None, None, "ps_narrow<12>"), ("narrow16", "slot", 17, None, None, "ps_narrow<16>"),
    ("whole_row9", "slot", 9, None, None, "ps_narrow_whole<1>"), ("whole", "slot", 9, None, 10, "ps_narrow_whole<0>"),
    ("rows_vec_statv", "deepfm", 20, None, None, "ps_rows<4,8,1>"),
    ("rows_vec", "deepfm", 20, (21, 0, 20, 22), None, "ps_rows<4,8,0>"),
    ("rows_scalar_statv", "deepfm", 17, (20, 0, 17, 21), None, "ps_rows<1,32,1>"),
    ("rows_scalar", "deepfm", 17, None, None, "ps_rows<1,32,0>"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,D,layout,pitch,note", PS_CASES, ids=[c[0] for c in PS_CASES])
def test_ps_push_leaf(ops, name, kind, D, layout, pitch, note):
    """rec_ps_push_rows against oracle/ps_ref.py at the bars of test_ps_push_narrow_shape_sweep, one case per kernel: the
    four lane-per-feature widths, the whole-record form with both gradients from one 9-float row and from a 10-float one,
    and the row-group kernel on float4 / scalar lanes with the statistics read as one float4 or not."""
    from oracle import deepfm_ref as R
    from oracle import ps_ref
    from paddlerec_amd import _lib
    rng = np.random.default_rng(4000 + D + len(name))
    kw = dict(embedx_threshold=1.5, initial_range=1e-2, seed=77, lr=0.05, embedx_lr=0.02, initial_g2sum=3.0,
              embedx_initial_g2sum=1.0, bounds=(-10.0, 10.0), embedx_bounds=(-0.25, 0.25), embedx_initial_range=2e-2,
              grad_scale=8.0, show_scale=True, embed_zero_init=False)
    tab = ops.PsTable(N, D, DEV, kind=kind, row_stride=64 if layout else None, **kw)
    if layout:
        tab.layout = _lib.PsLayout(64, *layout)
    Ly = tab.layout
    lay = dict(embed_off=Ly.embed_off, embedx_off=Ly.embedx_off, embedx_dim=Ly.embedx_dim, stat_off=Ly.stat_off)
    Dx, so = Ly.embedx_dim, Ly.stat_off
    rec = np.zeros((N, Ly.row_stride), np.float32)
    for r in range(1, N):                               # a third unborn, a third embed-only, a third full
        k = r % 3
        if k == 0:
            continue
        rec[r, Ly.embed_off] = rng.standard_normal() * 0.1
        rec[r, so:so + 4] = [rng.integers(1, 30), rng.integers(0, 2), rng.random() * 0.5, rng.random() * 0.5]
        rec[r, so + 4], rec[r, so + 5], rec[r, so + 6] = k, rng.random(), rng.integers(0, 9)
        if k == 2:
            rec[r, Ly.embedx_off:Ly.embedx_off + Dx] = rng.standard_normal(Dx) * 0.1
    tab.rec.copy_(T(rec))
    ids = bs_ids(rng)                                   # one id outside the table: the grouping flags and drops it
    show, click = rng.integers(1, 4, B).astype(np.int64), (rng.random(B) < 0.4).astype(np.int64)
    groups, status = ops.ids_group(T(ids), N, 0, ops.Workspace(DEV))
    n = B * S
    if kind == "slot":
        pitch = pitch or D
        gbuf = Rows((rng.standard_normal((n, D)) * 0.05), pitch)
        g_w, g_x = gbuf.got()[:, 0], gbuf.got()[:, 1:]
        with ops.route_log() as notes:
            ops.ps_push_rows(tab, groups, gbuf.buf, S, grad_pitch=pitch, show=T(show), click=T(click))
    else:
        gbuf = Rows((rng.standard_normal((n, D)) * 0.05), D)
        dz = (rng.standard_normal(B) * 0.05).astype(np.float32)
        g_w, g_x = np.repeat(dz, S), gbuf.got()
        with ops.route_log() as notes:
            ops.ps_push_rows(tab, groups, gbuf.buf, S, grad1=T(dz), grad1_div=S, show=T(show), click=T(click))
    assert notes == [note]
    rows = ids.reshape(-1)
    valid = (rows != 0) & (rows < N)
    uniq, merged, _ = R.merge_rows(rows, valid, np.concatenate([g_w[:, None], g_x], 1).astype(np.float32))
    dshow = np.array([np.repeat(show, S)[(rows == u) & valid].sum() for u in uniq], np.float64)
    dclick = np.array([np.repeat(click, S)[(rows == u) & valid].sum() for u in uniq], np.float64)
    want = rec.copy()
    ps_ref.push_rows(want, lay, uniq, merged[:, 0], merged[:, 1:], dshow, dclick, dict(kw, nonclk_coeff=0.1, click_coeff=1.0))
    got = H(tab.rec)
    assert np.array_equal(got[:, so:so + 2], want[:, so:so + 2]) and np.array_equal(got[:, so + 4], want[:, so + 4])
    assert np.array_equal(got[:, so + 6], want[:, so + 6])
    np.testing.assert_allclose(got[:, so + 5], want[:, so + 5], rtol=1e-6)
    wcols = np.r_[Ly.embed_off, Ly.embedx_off:Ly.embedx_off + Dx]
    np.testing.assert_allclose(got[:, wcols], want[:, wcols], rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(got[:, so + 2:so + 4], want[:, so + 2:so + 4], rtol=2e-6, atol=1e-12)
    other = np.setdiff1d(np.arange(Ly.row_stride), np.r_[wcols, so:so + 7])
    assert np.array_equal(got[:, other], rec[:, other])                               # padding columns of every record
    assert np.array_equal(got[np.setdiff1d(np.arange(N), uniq)], rec[np.setdiff1d(np.arange(N), uniq)])
    assert int(status.item()) == 1
