"""Every rec_gemm_f32 epilogue on every kernel route that instantiates it — and the route ASSERTED, not assumed.

One call of rec_gemm_f32 lands on one of nine kernel families by rules over the shape, the alignment and the leading
dimensions (csrc/gemm_f32.hip, csrc/gemm_direct.h).  A test that only picks a shape silently changes its subject when a
rule moves.  Here a case names its route (ROUTES below: family, tile config, K slices, loader / kernel flags), reads
ops.gemm_last_route() back and FAILS if the shape no longer reaches it; then C (and the second output of "cross") is held
against float64 inside the bound of tests/gemm_ref.py — the bars of an exact-f32 accumulate, nothing tuned here.

Layouts: "contiguous", and "windows" — out, aux0, aux1, out2 are column windows of wider buffers, each with its own
(odd, unaligned) leading dimension, row_scale is a column of an [M, 3] tensor: the same kernel doing the same arithmetic,
so C must be BIT-identical to the contiguous call (any difference is a wrong stride) and nothing outside the windows may
change.  Every call runs twice and must repeat its bits.
"""
import collections
import math
import zlib

import numpy as np
import pytest

import gemm_ref
from gemm_ref import EPILOGUES

DEV = "cuda"
PIPE_EPILOGUES = ("none", "bias", "bias_relu", "relu_mask")     # the instantiations of gemm_f32_pipe_kernel
LAYOUTS = ("contiguous", "windows")
# epilogue variants: name -> (epilogue, operands left out).  "cross" itself stores its second output.
VARIANTS = collections.OrderedDict((e, (e, ())) for e in EPILOGUES)
VARIANTS.update(add_no_bias=("add", ("bias",)), add_no_aux0=("add", ("aux0",)), bias_tanh_no_bias=("bias_tanh", ("bias",)),
                cross_no_out2=("cross", ("out2",)))

Route = collections.namedtuple("Route", "name M N K split_k family cfg splits flags forms view_a")


def _route(name, M, N, K, family, forms, split_k=0, cfg=None, splits=1, flags=(), view_a=False):
    """forms: {"nn" | "nt" | "tn" | "tt" (trans_a, trans_b): flags this form adds to `flags`}; the variants of a route take
    its forms in turn.  view_a: A is a column window at an unaligned start of a wider buffer."""
    return Route(name, M, N, K, split_k, family, cfg, splits, frozenset(flags), collections.OrderedDict(forms), view_a)


_ALL = ("nn", "nt", "tn", "tt")
_plain = lambda forms: [(f, ()) for f in forms]
# `fast` (branch-free tile loaders) needs both operands 16-byte aligned with leading dimension and contiguous extent
# multiples of 4: at N = 150 / 90 only the forms whose B is stored [N, K] have it
_fast_nt = [("nn", ()), ("nt", ("fast",)), ("tn", ()), ("tt", ())]
_fast_tb = [("nn", ()), ("nt", ("fast",)), ("tn", ()), ("tt", ("fast",))]
ROUTE_LIST = [
    # ---- direct (gemm_direct.h): M N K < 1.5e8, K <= 1024, N > 4; ragged 16-row and 64-column strips
    _route("direct_vec", 37, 70, 36, "direct", _plain(("nn", "nt", "tt")), flags=("vec",)),     # (tn has no float4 form)
    _route("direct_scalar", 37, 70, 37, "direct", _plain(_ALL)),                                 # ld % 4 != 0
    _route("direct_scalar_view", 37, 70, 36, "direct", _plain(("nn",)), view_a=True),            # unaligned start
    # <= 256 tiles and K >= 128: four waves per tile, folded in LDS
    _route("direct_ks4", 37, 70, 132, "direct", [("nn", ("vec",)), ("nt", ("vec",)), ("tn", ()), ("tt", ("vec",))],
           flags=("ks4",)),
    # (second shapes: with the rotation below every epilogue meets all four forms on the direct kernel; three 64-column
    # strips with a ragged last one, K % 16 != 0 / a single row tile)
    _route("direct_scalar_b", 21, 133, 53, "direct", _plain(_ALL)),
    _route("direct_ks4_b", 19, 40, 200, "direct", [("nn", ("vec",)), ("nt", ("vec",)), ("tn", ()), ("tt", ("vec",))],
           flags=("ks4",)),
    # ---- tiled (gemm_f32.hip); K > 1024 leaves the direct kernel, split_k = 1 keeps the automatic K split off
    # N % 4 != 0: element-wise checked loader (MODE 2) on every tile, a K tail tile, ragged epilogue stores
    _route("tiled_checked", 130, 90, 1042, "tiled", _plain(_ALL), split_k=1, cfg="80x80"),
    # aligned, multiples of 4, no whole tile: branch-free edge loader (MODE 1)
    _route("tiled_fast_edge", 132, 92, 1040, "tiled", _plain(_ALL), split_k=1, cfg="80x80", flags=("fast",)),
    # whole tiles: the pipe kernel for its four epilogues, the plain kernel (MODE 0) for the other seven
    _route("tiled_whole", 160, 160, 1040, "tiled", _plain(("nn", "nt", "tn")), split_k=1, cfg="80x80", flags=("fast",)),
    # plan_gemm, m < 2048: 64x80 for a short row-major A, 128x128 for its trans_a form
    _route("tiled_64x80", 120, 120, 1040, "tiled", _plain(("nn", "nt")), split_k=1, cfg="64x80", flags=("fast",)),
    _route("tiled_128x128_short", 120, 120, 1040, "tiled", _plain(("tn", "tt")), split_k=1, cfg="128x128", flags=("fast",)),
    # 2048 <= M < 8192: the tile width that wastes fewer columns
    _route("tiled_128x80", 2050, 150, 1040, "tiled", _fast_nt, split_k=1, cfg="128x80"),
    _route("tiled_128x128", 2050, 90, 1040, "tiled", _fast_nt, split_k=1, cfg="128x128"),
    # M >= 8192: N % 4 != 0 and M % 128 != 0 keep bf16x3 and the ring out, M N K >= 1.5e8 the direct kernel
    _route("tiled_256x80", 8200, 150, 208, "tiled", _fast_tb, split_k=1, cfg="256x80"),
    _route("tiled_256x128", 8200, 90, 208, "tiled", _fast_tb, split_k=1, cfg="256x128"),
] + [
    # ---- tiled partial tiles + splitk_reduce_kernel<E>: 128 K tiles (the last one ragged) in 2 / 7 slices on a 2-D
    # grid, 8 / 16 folded into a 1-D grid
    _route("splitk_%d" % s, 130, 90, 2042, "tiled", _plain(_ALL), split_k=s, cfg="80x80", splits=s,
           flags=("fold",) if s % 8 == 0 else ())
    for s in (2, 7, 8, 16)
] + [
    # ---- skinny rows (gemv_rows_kernel): N <= 4, A row-major; K % 4 == 0: float4 loads of A
    _route("skinny_n%d_k%d" % (n, k), 300, n, k, "skinny_rows", _plain(("nn", "nt")), flags=("vec_a",) if k % 4 == 0 else ())
    for k in (400, 401) for n in (1, 3, 4)
] + [
    _route("skinny_grid_stride", 9000, 1, 64, "skinny_rows", _plain(("nn", "nt")), flags=("vec_a",)),   # > 8192 rows
]
ROUTES = collections.OrderedDict((r.name, r) for r in ROUTE_LIST)
_ROTATION = {r.name: i for i, r in enumerate(ROUTE_LIST)}
_ROTATION.update(direct_scalar=0, direct_ks4=1, direct_scalar_b=2, direct_ks4_b=3)
# what the suite must keep covering: every row of the route table, each with every epilogue variant in both layouts
REQUIRED_ROUTES = ("direct_vec", "direct_scalar", "direct_scalar_view", "direct_ks4", "direct_scalar_b", "direct_ks4_b",
                   "tiled_checked", "tiled_fast_edge",
                   "tiled_whole", "tiled_64x80", "tiled_128x128_short", "tiled_128x80", "tiled_128x128", "tiled_256x80",
                   "tiled_256x128", "splitk_2", "splitk_7", "splitk_8", "splitk_16", "skinny_n1_k400", "skinny_n3_k400",
                   "skinny_n4_k400", "skinny_n1_k401", "skinny_n3_k401", "skinny_n4_k401", "skinny_grid_stride")

CASES = [(r, v, l) for r in ROUTES for v in VARIANTS for l in LAYOUTS]
# out aliasing aux1 (xdeepfm.py: gemm(..., epilogue="add", aux1=dxk_c, out=dxk_c)); "x3" is the bf16 x 3 kernel
INPLACE_ROUTES = ("direct_vec", "direct_ks4", "tiled_checked", "splitk_7", "splitk_8", "skinny_n3_k400", "x3")
INPLACE_EPILOGUES = ("add", "cross", "moe")
# (the bf16 x 3 kernel demands aligned epilogue operands: windows leave its route)
INPLACE_CASES = [(r, e, l) for r in INPLACE_ROUTES for e in INPLACE_EPILOGUES for l in LAYOUTS if (r, l) != ("x3", "windows")]
X3_ROUTE = _route("x3", 8192, 400, 72, "x3", _plain(("nn", "nt")))


def form_of(route, variant):
    """(form, expected flags) of one case: the variants of a route take its forms in turn."""
    forms = list(route.forms.items())
    turn = list(VARIANTS).index(variant) + _ROTATION.get(route.name, 0)     # (routes start at different forms)
    form, extra = forms[turn % len(forms)]
    flags = set(route.flags) | set(extra)
    if route.name == "tiled_whole" and VARIANTS[variant][0] in PIPE_EPILOGUES:
        flags.add("pipe")
    return form, frozenset(flags)


def expected_route(route, variant):
    """What ops.gemm_last_route() must report for this case."""
    from paddlerec_amd import ops
    return ops.GemmRouteInfo(route.family, route.cfg, route.splits, form_of(route, variant)[1])


# ------------------------------------------------------------------------------------------ no GPU needed
def test_route_table_covers_every_route_epilogue_and_layout():
    """Pure bookkeeping over the parametrization: taking a row out of the table fails here."""
    have = set(CASES)
    assert len(have) == len(CASES)
    assert set(EPILOGUES) == {"none", "bias", "bias_relu", "relu_mask", "cross", "bias_sigmoid", "bias_tanh", "add", "moe",
                              "dsigmoid", "dtanh"}
    assert {VARIANTS[v][0] for v in VARIANTS} == set(EPILOGUES) and len(VARIANTS) == 15
    assert VARIANTS["add_no_bias"] == ("add", ("bias",)) and VARIANTS["add_no_aux0"] == ("add", ("aux0",))
    assert VARIANTS["bias_tanh_no_bias"] == ("bias_tanh", ("bias",)) and VARIANTS["cross_no_out2"] == ("cross", ("out2",))
    assert VARIANTS["cross"] == ("cross", ())                                    # "cross" itself checks out2
    missing = [(r, v, l) for r in REQUIRED_ROUTES for v in VARIANTS for l in LAYOUTS if (r, v, l) not in have]
    assert not missing, missing[:5]
    fam = lambda prefix: {ROUTES[r].family for r in REQUIRED_ROUTES if r.startswith(prefix)}
    assert fam("direct") == {"direct"} and fam("tiled") == {"tiled"} and fam("splitk") == {"tiled"}
    assert fam("skinny") == {"skinny_rows"}
    # the four direct forms: VEC / scalar x KS 1 / 4
    direct = {form_of(ROUTES[r], v)[1] for r in REQUIRED_ROUTES if r.startswith("direct") for v in VARIANTS}
    assert direct == {frozenset(), frozenset({"vec"}), frozenset({"ks4"}), frozenset({"vec", "ks4"})}
    # all six tile configs of the planner, the three loader modes' selectors, the pipe kernel and its plain twin
    assert {ROUTES[r].cfg for r in REQUIRED_ROUTES if ROUTES[r].family == "tiled"} == {
        "80x80", "64x80", "128x128", "128x80", "256x80", "256x128"}
    whole = {VARIANTS[v][0]: "pipe" in form_of(ROUTES["tiled_whole"], v)[1] for v in VARIANTS}
    assert {e for e, p in whole.items() if p} == set(PIPE_EPILOGUES) and len(whole) == 11
    assert "fast" not in ROUTES["tiled_checked"].flags and "fast" in ROUTES["tiled_fast_edge"].flags
    # split-K: both grid forms, every epilogue through the reduce
    assert {ROUTES["splitk_%d" % s].splits for s in (2, 7, 8, 16)} == {2, 7, 8, 16}
    assert ["fold" in ROUTES["splitk_%d" % s].flags for s in (2, 7, 8, 16)] == [False, False, True, True]
    # every (trans_a, trans_b) form appears with every epilogue on the direct and on the tiled routes
    for prefix in ("direct", "tiled"):
        seen = {(VARIANTS[v][0], form_of(ROUTES[r], v)[0]) for r in REQUIRED_ROUTES if r.startswith(prefix) for v in VARIANTS}
        assert seen == {(e, f) for e in EPILOGUES for f in _ALL}, prefix
    # skinny rows: N 1 / 3 / 4, float4 and scalar loads of A, both B forms, the grid-stride loop
    sk = [ROUTES[r] for r in REQUIRED_ROUTES if r.startswith("skinny")]
    assert {(r.N, "vec_a" in r.flags) for r in sk if r.M == 300} == {(n, v) for n in (1, 3, 4) for v in (True, False)}
    assert any(r.M > 8192 for r in sk) and all(set(r.forms) == {"nn", "nt"} for r in sk)
    # in place: direct KS 1 and KS 4, tiled without and with the reduce (both grid forms), skinny rows, bf16 x 3
    assert set(INPLACE_EPILOGUES) == {"add", "cross", "moe"}
    assert set(INPLACE_ROUTES) == {"direct_vec", "direct_ks4", "tiled_checked", "splitk_7", "splitk_8", "skinny_n3_k400", "x3"}
    assert {(r, e) for r, e, _ in INPLACE_CASES} == {(r, e) for r in INPLACE_ROUTES for e in INPLACE_EPILOGUES}
    for r in ROUTES.values():                               # the largest case stays under 0.7 GFLOP
        assert 2.0 * r.M * r.N * r.K < 0.7e9, r.name


# ------------------------------------------------------------------------------------------ operands
@pytest.fixture(scope="module")
def ops(engine_lib):
    from paddlerec_amd import ops as o
    return o


_state_cache, _contiguous_results = {}, {}
SENTINEL = -777.25


class _State:
    """The operands of one route, made once: float32 NumPy (logical A [M,K], B [K,N]), their float64 product, and the
    device copies (never written)."""

    def __init__(self, route):
        import torch
        rng = np.random.default_rng(zlib.crc32(route.name.encode()))
        M, N, K = route.M, route.N, route.K
        u = lambda *shape: rng.uniform(-1, 1, size=shape).astype(np.float32)
        self.A = u(M, K)
        self.B = (u(K, N) * (1.5 / math.sqrt(K))).astype(np.float32)     # |acc| ~ 0.5: tanh / sigmoid off their plateaus
        self.bias, self.X0, self.X1, self.prob = u(N), u(M, N), u(M, N), u(M, 3)
        self.X0[::7, ::5] = 0.0                                         # relu_mask: aux0 == 0 masks
        # sigmoid / tanh arguments that saturate, and overflow expf: +-60, +-100 (as many as N holds)
        self.bias_sat = self.bias.copy()
        for j, v in zip(range(N - 1, -1, -1), (-100.0, 100.0, -60.0, 60.0)):
            self.bias_sat[j] = v
        self.rs = np.ascontiguousarray(self.prob[:, 1])
        self.prod = gemm_ref.product(self.A, self.B)
        self.t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
        self.dev = {k: self.t(getattr(self, k)) for k in ("bias", "bias_sat", "X0", "X1", "prob", "rs")}
        self._ab = {}
        self.route = route

    def operands(self, form):
        import torch
        if form not in self._ab:
            At = self.t(self.A.T if form[0] == "t" else self.A)
            if self.route.view_a:                            # a window at column 1: rows 16-byte aligned apart, start not
                wide = torch.zeros(At.shape[0], At.shape[1] + 4, device=DEV)
                wide[:, 1:1 + At.shape[1]] = At
                At = wide[:, 1:1 + At.shape[1]]
            self._ab[form] = (At, self.t(self.B.T if form[1] == "t" else self.B))
        return self._ab[form]


def _state(route):
    if route.name not in _state_cache:
        _state_cache[route.name] = _State(route)
    return _state_cache[route.name]


def _window(M, N, ld, col, fill):
    import torch
    wide = torch.full((M, ld), SENTINEL, device=DEV)
    view = wide[:, col:col + N]
    if fill is not None:
        view.copy_(fill)
    return wide, view


def _call(ops, ws, route, variant, layout, inplace=False):
    """One ops.gemm call of the case -> (C, out2 or None, route report, [(wide buffer, window column, values the window
    must hold afterwards or None for an output)])."""
    st = _state(route)
    epi, drop = VARIANTS[variant]
    form = form_of(route, variant)[0]
    At, Bt = st.operands(form)
    M, N = route.M, route.N
    sat = epi in ("bias_sigmoid", "bias_tanh")
    use = lambda name, needs: epi in needs and name not in drop
    kw = dict(trans_a=form[0] == "t", trans_b=form[1] == "t", epilogue=epi, split_k=route.split_k)
    wides = []
    if use("bias", gemm_ref.NEEDS_BIAS):
        kw["bias"] = st.dev["bias_sat" if sat else "bias"]
    want_out2 = epi == "cross" and "out2" not in drop
    import torch
    if layout == "contiguous":
        if use("aux0", gemm_ref.NEEDS_AUX0):
            kw["aux0"] = st.dev["X0"]
        if use("aux1", gemm_ref.NEEDS_AUX1):
            kw["aux1"] = st.dev["X1"].clone() if inplace else st.dev["X1"]
        if epi == "moe":
            kw["row_scale"] = st.dev["rs"]
        if want_out2:
            kw["out2"] = torch.full((M, N), SENTINEL, device=DEV)
        kw["out"] = kw["aux1"] if inplace else torch.full((M, N), SENTINEL, device=DEV)
    else:
        # every operand in a buffer of its own width: a kernel that took one leading dimension for another cannot pass
        ld1 = N + 5 if N % 2 == 0 else N + 6                 # odd, and not aux0's
        if use("aux0", gemm_ref.NEEDS_AUX0):
            w, kw["aux0"] = _window(M, N, N + 3, 1, st.dev["X0"])         # unaligned start
            wides.append((w, 1, st.dev["X0"]))
        if use("aux1", gemm_ref.NEEDS_AUX1):
            w, kw["aux1"] = _window(M, N, ld1, 2, st.dev["X1"])
            wides.append((w, 2, None if inplace else st.dev["X1"]))
        if epi == "moe":
            kw["row_scale"] = st.dev["prob"][:, 1]           # the gate of expert 1 of 3: stride 3
        if want_out2:
            w, kw["out2"] = _window(M, N, N + 7, 3, None)
            wides.append((w, 3, None))
        if inplace:
            kw["out"] = kw["aux1"]
        else:
            w, kw["out"] = _window(M, N, N + 9, 4, None)
            wides.append((w, 4, None))
    C = ops.gemm(At, Bt, ws, **kw)
    report = ops.gemm_last_route()
    assert C.data_ptr() == kw["out"].data_ptr()
    return C, kw.get("out2"), report, wides


def _reference(route, variant):
    st = _state(route)
    epi, drop = VARIANTS[variant]
    sat = epi in ("bias_sigmoid", "bias_tanh")
    bias = (st.bias_sat if sat else st.bias) if epi in gemm_ref.NEEDS_BIAS and "bias" not in drop else None
    X0 = st.X0 if epi in gemm_ref.NEEDS_AUX0 and "aux0" not in drop else None
    X1 = st.X1 if epi in gemm_ref.NEEDS_AUX1 else None
    want, bound = gemm_ref.epi_reference(epi, st.A, st.B, bias, X0, X1, st.rs if epi == "moe" else None, prod=st.prod)
    u = gemm_ref.cross_out2_reference(st.A, st.B, bias, prod=st.prod) if epi == "cross" and "out2" not in drop else None
    return want, bound, u


def _outside_untouched(wides, N):
    for wide, col, inside in wides:
        w = wide.cpu().numpy()
        assert np.all(w[:, :col] == SENTINEL) and np.all(w[:, col + N:] == SENTINEL), "wrote outside a window"
        if inside is not None:                               # an input: the call must not have written it
            assert np.array_equal(w[:, col:col + N], inside.cpu().numpy())


def _run_checked(ops, ws, route, variant, layout, inplace=False):
    """The case, twice: the named route both times, identical bits, nothing outside the windows -> (C, out2) as NumPy."""
    want_route = expected_route(route, variant)
    got = []
    for _ in range(2):
        C, U, report, wides = _call(ops, ws, route, variant, layout, inplace)
        assert report == want_route, "%s / %s: the call took %r, the case means %r" % (route.name, variant, report, want_route)
        got.append((C.cpu().numpy(), None if U is None else U.cpu().numpy()))
        _outside_untouched(wides, route.N)
    assert np.array_equal(got[0][0], got[1][0]), "two runs differ"
    if got[0][1] is not None:
        assert np.array_equal(got[0][1], got[1][1]), "two runs differ (out2)"
    return got[0]


# ------------------------------------------------------------------------------------------ the matrix
@pytest.fixture(scope="module")
def ws(ops):
    return ops.Workspace(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant,layout", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_gemm_route_epilogue(ops, ws, name, variant, layout):
    route = ROUTES[name]
    C, U = _run_checked(ops, ws, route, variant, layout)
    want, bound, u = _reference(route, variant)
    assert np.all(np.isfinite(C))
    gemm_ref.check(C, want, bound, "C")
    if u is not None:
        gemm_ref.check(U, u[0], u[1], "out2")
    else:
        assert U is None
    if layout == "contiguous":
        _contiguous_results[name, variant] = (C, U)
        return
    # same A and B, same kernel, same arithmetic: the windows change addresses only
    if (name, variant) not in _contiguous_results:
        _contiguous_results[name, variant] = _run_checked(ops, ws, route, variant, "contiguous")
    C0, U0 = _contiguous_results[name, variant]
    assert np.array_equal(C, C0), "C differs from the contiguous call: %d elements" % int((C != C0).sum())
    if U is not None:
        assert np.array_equal(U, U0), "out2 differs from the contiguous call: %d elements" % int((U != U0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name,epi,layout", INPLACE_CASES, ids=["%s-%s-%s" % c for c in INPLACE_CASES])
def test_gemm_out_aliases_aux1(ops, ws, monkeypatch, name, epi, layout):
    """out IS aux1 (C is __restrict__ in every kernel; an element's aux1 is read by the thread that then stores it):
    bit-identical to the out-of-place call on the same route, and right against float64."""
    route = ROUTES.get(name, X3_ROUTE)
    if name == "x3":
        monkeypatch.setenv("REC_GEMM_BF16X3", "1")           # (read per call; the route is asserted like every other)
    C0, U0 = _run_checked(ops, ws, route, epi, layout)
    C1, U1 = _run_checked(ops, ws, route, epi, layout, inplace=True)
    want, bound, u = _reference(route, epi)
    gemm_ref.check(C1, want, bound, "C")
    assert np.array_equal(C0, C1), "in place differs from out of place: %d elements" % int((C0 != C1).sum())
    if u is not None:
        gemm_ref.check(U1, u[0], u[1], "out2")
        assert np.array_equal(U0, U1)
