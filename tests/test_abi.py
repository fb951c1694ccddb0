"""The C-ABI shared library loads without a GPU and exports every symbol include/recengine.h declares."""
import os
import re

from conftest import REPO


def _declared():
    src = open(os.path.join(REPO, "include", "recengine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(rec_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_symbols_exported(engine_lib):
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(engine_lib, n), "missing export: " + n


def test_python_signature_table_covers_header(engine_lib):
    from paddlerec_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_error_reporting_without_gpu(engine_lib):
    """Argument validation happens before any launch: callable on a GPU-less host."""
    import ctypes as C
    from paddlerec_amd import _lib
    n = C.c_size_t(0)
    rc = engine_lib.rec_ids_group_workspace_bytes(-5, 10, C.byref(n))
    assert rc == -1 and b"bad" in engine_lib.rec_last_error()
    d = _lib.DeepFMDesc(4, 26, 99, 16, 16, 10, 0)        # num_dense too large
    rc = engine_lib.rec_deepfm_fm_bwd_workspace_bytes(C.byref(d), C.byref(n))
    assert rc == -2
    assert engine_lib.rec_version() >= 100


def test_product_never_imports_oracle():
    """The product path must not route through the oracle (or any CPU fallback)."""
    pkg = os.path.join(REPO, "paddlerec_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "liboracle" not in txt, f


def test_host_planning_queries(engine_lib):
    """Pure host logic behind the boundary: split-K planning for a CU budget, partial-sum buffer sizing."""
    import ctypes as C
    from paddlerec_amd import _lib
    sp = C.c_int32(0)
    # dW of the 400x400 MLP layers at batch 65536: 5 x 5 tiles of 80x80 (no padding rows), 4 blocks per CU
    d = _lib.GemmDesc(400, 400, 65536, 400, 400, 400, 1, 0, 0, 0)
    assert engine_lib.rec_gemm_plan_splits(C.byref(d), 0, C.byref(sp)) == 0
    full = sp.value
    assert full == 40 and full % 8 == 0                      # 256 CUs * 4 / 25 tiles = one resident round
    assert engine_lib.rec_gemm_plan_splits(C.byref(d), 192, C.byref(sp)) == 0
    assert sp.value == 24                                    # 192 CUs * 4 / 25 = 30 -> multiple of 8
    assert engine_lib.rec_gemm_plan_splits(C.byref(d), 8, C.byref(sp)) == 0 and sp.value == 1
    # forward GEMM [65536 x 400] = 2560 tiles: fills the chip without splitting K
    f = _lib.GemmDesc(65536, 400, 432, 432, 400, 400, 0, 0, 0, 0)
    assert engine_lib.rec_gemm_plan_splits(C.byref(f), 0, C.byref(sp)) == 0 and sp.value == 1
    # an explicit split_k in the descriptor is ignored by the query
    d.split_k = 7
    assert engine_lib.rec_gemm_plan_splits(C.byref(d), 0, C.byref(sp)) == 0 and sp.value == full
    assert engine_lib.rec_gemm_plan_splits(C.byref(d), 100000, C.byref(sp)) == -1
    bad = _lib.GemmDesc(4, 0, 4, 4, 4, 4, 0, 0, 0, 0)
    assert engine_lib.rec_gemm_plan_splits(C.byref(bad), 0, C.byref(sp)) == -1
    n = C.c_size_t(0)
    assert engine_lib.rec_segment_partials_bytes(65536 * 26, 16, C.byref(n)) == 0
    assert n.value == (65536 * 26 // 64) * 2 * 16 * 4          # [tiles, 2, D] floats, REC_SEG_TILE = 64
    assert engine_lib.rec_segment_partials_bytes(65, 1, C.byref(n)) == 0 and n.value == 2 * 2 * 4
    assert engine_lib.rec_segment_partials_bytes(-1, 16, C.byref(n)) == -1


def test_gemm_route_report_without_gpu(engine_lib):
    """rec_gemm_last_route is host bookkeeping: it answers on a GPU-less host, and a call that is refused before it
    chooses a kernel leaves the report as it was."""
    import ctypes as C
    from paddlerec_amd import _lib
    L = engine_lib
    assert L.rec_gemm_last_route(None) == -1
    r0, r1 = _lib.GemmRoute(), _lib.GemmRoute()
    assert L.rec_gemm_last_route(C.byref(r0)) == 0
    assert -1 <= r0.family < len(_lib.GEMM_ROUTE_FAMILIES) and -1 <= r0.cfg < len(_lib.GEMM_CFGS)
    d = _lib.GemmDesc(4, 4, 4, 4, 4, 4, 0, 0, 99, 0)                      # unknown epilogue: refused
    assert L.rec_gemm_f32(C.byref(d), None, None, None, None, None, 0, None) == -1
    assert L.rec_gemm_last_route(C.byref(r1)) == 0
    assert (r1.family, r1.cfg, r1.splits, r1.flags) == (r0.family, r0.cfg, r0.splits, r0.flags)
    # the Python names are the header's enumerators
    src = open(os.path.join(REPO, "include", "recengine.h")).read()
    enums = {n.lower(): int(v) for n, v in re.findall(r"\bREC_GEMM_ROUTE_([A-Z0-9_]+) = (\d+)", src)}
    assert enums == dict({n: i for i, n in enumerate(_lib.GEMM_ROUTE_FAMILIES)}, **_lib.GEMM_ROUTE_FLAGS)
    # ... and the tile config names are the planner's, in its order
    hip = open(os.path.join(REPO, "paddlerec_amd", "csrc", "gemm_f32.hip")).read()
    cfgs = re.search(r"enum GemmCfg \{([^}]*)\}", hip).group(1)
    names = [c.split("=")[0].strip()[4:].lower() for c in cfgs.split(",") if c.strip() and "COUNT" not in c]
    assert tuple(names) == _lib.GEMM_CFGS


def test_more_argument_validation_without_gpu(engine_lib):
    """Every entry point rejects null pointers / bad sizes before it touches the device."""
    import ctypes as C
    from paddlerec_amd import _lib
    L = engine_lib
    gl = _lib.GradLayout(1, 0, 0, None, None)
    h = _lib.AdamHyper(1e-3, 0.9, 0.999, 1e-8, 1)
    assert L.rec_segment_partials(10, 16, None, None, None, None, C.byref(gl), None, None) == -1
    assert L.rec_segment_partials(0, 0, None, None, None, None, None, None, None) == -1
    assert L.rec_sparse_adam_rows(10, 16, 8, 0, None, None, None, None, None, None, None, None, None, None,
                                  C.byref(h), None) == -1              # row_stride < emb_dim
    assert b"bad sizes" in L.rec_last_error()
    assert L.rec_sparse_sgd_rows(10, 16, 16, None, None, None, None, None, None, None, 0.1, None) == -1
    assert L.rec_stream_spin(-1, None) == -1
    out = C.c_void_p()
    assert L.rec_stream_create_cu_range(5, 5, C.byref(out)) == -1
    assert L.rec_stream_create_cu_range(0, 64, None) == -1
    assert L.rec_stream_destroy(None) == 0
    d = _lib.GemmDesc(4, 4, 4, 4, 4, 4, 0, 0, 99, 0)
    assert L.rec_gemm_f32(C.byref(d), None, None, None, None, None, 0, None) == -1
    assert b"epilogue" in L.rec_last_error()
    nl = C.c_int64(0)
    assert L.rec_count_lines(None, 10, 1, C.byref(nl)) == -1
    assert L.rec_count_lines(b"a\nb\nc", 5, 4, C.byref(nl)) == 0 and nl.value == 3


def test_cross_entry_points_reject_bad_arguments_without_gpu(engine_lib):
    """Host checks of the CrossNet glue kernels and layer entry points: they return before any launch, so they can be
    called on a GPU-less host with dummy non-null pointer values (tests/test_cross_layers_gpu.py runs the kernels)."""
    import ctypes as C
    from paddlerec_amd import _lib
    L = engine_lib
    p = C.c_void_p(4096)                                     # never dereferenced: every call below is refused first
    # softmax over the experts: 1 <= E <= 64, leading dimensions >= E
    assert L.rec_softmax_rows(4, 65, p, 65, p, 65, None) == -1
    assert L.rec_softmax_rows(4, 0, p, 4, p, 4, None) == -1
    assert L.rec_softmax_rows(4, 5, p, 4, p, 5, None) == -1
    assert L.rec_softmax_rows(4, 5, p, 5, p, 4, None) == -1
    assert L.rec_softmax_rows_bwd(4, 65, p, 65, p, 65, p, 65, None) == -1
    for bad in range(3):
        lds = [5, 5, 5]
        lds[bad] = 4
        assert L.rec_softmax_rows_bwd(4, 5, p, lds[0], p, lds[1], p, lds[2], None) == -1
    # the streaming glue: every leading dimension >= n
    for bad in range(5):
        lds = [8] * 5
        lds[bad] = 7
        assert L.rec_cross_bwd_prep(3, 8, p, lds[0], p, lds[1], p, lds[2], p, lds[3], p, lds[4], 0, None) == -1
        assert L.rec_moe_bwd_prep(3, 8, p, lds[0], p, lds[1], p, lds[2], p, 1, p, lds[3], p, lds[4], 0, p, 1, None) == -1
    assert L.rec_moe_bwd_prep(3, 8, p, 8, p, 8, p, 8, p, 0, p, 8, p, 8, 0, p, 1, None) == -1      # prob_stride < 1
    assert L.rec_cross_bwd_prep(0, 8, None, 8, None, 8, None, 8, None, 8, None, 8, 0, None) == 0  # m = 0: nothing to do
    # global-norm clip
    assert L.rec_clip_scale(p, 0.0, p, None) == -1
    assert L.rec_clip_scale(p, -1.0, p, None) == -1
    assert L.rec_clip_scale(None, 1.0, p, None) == -1
    # CrossNetMix: experts <= 64, rank > 0, dXl must not alias dXnext (batch > 0: batch == 0 returns success first)
    n = C.c_size_t(0)
    assert L.rec_crossnet_mix_layer_workspace_bytes(C.byref(_lib.CrossMixDesc(8, 12, 4, 65, 0, 0, 0)), C.byref(n), None) == -1
    assert L.rec_crossnet_mix_layer_workspace_bytes(C.byref(_lib.CrossMixDesc(8, 12, 0, 4, 0, 0, 0)), C.byref(n), None) == -1
    ok = _lib.CrossMixDesc(8, 12, 4, 3, 0, 0, 0)

    def mix_bwd(desc, dxnext, dxl, ld_dxnext=0, ld_acc=0, ld_dxl=0):
        return L.rec_crossnet_mix_layer_bwd(C.byref(desc), *[p] * 10, dxnext, ld_dxnext, p, ld_acc, 0, 0, dxl, ld_dxl,
                                            *[p] * 6, 0, p, C.c_size_t(1 << 30), None)
    q = C.c_void_p(8192)
    assert mix_bwd(ok, p, p) == -1 and b"alias" in L.rec_last_error()
    assert mix_bwd(_lib.CrossMixDesc(8, 12, 4, 65, 0, 0, 0), p, q) == -1
    assert mix_bwd(_lib.CrossMixDesc(8, 12, 0, 3, 0, 0, 0), p, q) == -1
    assert mix_bwd(_lib.CrossMixDesc(0, 12, 4, 3, 0, 0, 0), p, p) == 0
    # row strides below d — descriptor fields and the gradient strides of the call — are refused before anything runs
    assert mix_bwd(_lib.CrossMixDesc(8, 12, 4, 3, 11, 0, 0), p, q) == -1
    for k in range(3):
        lds = [0, 0, 0]
        lds[k] = 11
        assert mix_bwd(ok, p, q, *lds) == -1 and b"stride" in L.rec_last_error()

    def v2_bwd(desc, ld_dxnext=0, ld_acc=0, ld_dxl=0, ws_bytes=1 << 30):
        return L.rec_crossnet_v2_layer_bwd(C.byref(desc), p, p, p, p, p, ld_dxnext, p, ld_acc, 0, 0, q, ld_dxl, p, p, p,
                                           C.c_size_t(ws_bytes), None)
    assert v2_bwd(_lib.CrossV2Desc(8, 12, 0, 11, 0, 0)) == -1
    for k in range(3):
        lds = [0, 0, 0]
        lds[k] = 11
        assert v2_bwd(_lib.CrossV2Desc(8, 12, 0, 0, 0, 0), *lds) == -1 and b"stride" in L.rec_last_error()
    assert v2_bwd(_lib.CrossV2Desc(0, 12, 0, 0, 0, 0)) == 0


def test_cross_layer_workspace_covers_the_strides_of_the_call(engine_lib):
    """include/recengine.h, gradient strides: at B 64, d 156 the dXl GEMM splits K and its partials are
    [splits][B][ld_dxl].  A dXl of row stride 176 needs more than the bwd_bytes of a descriptor that names no stride
    above 156: the call is refused with REC_EWORKSPACE BEFORE its first launch (host arithmetic only — this runs without
    a GPU), and a descriptor whose ld_out names 176 reports a bwd_bytes that covers it."""
    import ctypes as C
    from paddlerec_amd import _lib
    L = engine_lib
    B, d, wide = 64, 156, 176
    sp = C.c_int32(0)
    assert L.rec_gemm_plan_splits(C.byref(_lib.GemmDesc(B, d, d, d, d, wide, 0, 1, 7, 0)), 0, C.byref(sp)) == 0
    need_gemm = {}
    for ldc in (d, wide):
        n = C.c_size_t(0)
        assert L.rec_gemm_f32_workspace_bytes(C.byref(_lib.GemmDesc(B, d, d, d, d, ldc, 0, 1, 7, 0)), C.byref(n)) == 0
        need_gemm[ldc] = n.value
    plain, named = C.c_size_t(0), C.c_size_t(0)
    assert L.rec_crossnet_v2_layer_workspace_bytes(C.byref(_lib.CrossV2Desc(B, d, 0, 0, 0, 0)), None, C.byref(plain)) == 0
    assert L.rec_crossnet_v2_layer_workspace_bytes(C.byref(_lib.CrossV2Desc(B, d, 0, 0, wide, 0)), None,
                                                   C.byref(named)) == 0
    du = (B * d * 4 + 255) // 256 * 256
    assert named.value >= du + need_gemm[wide] and named.value >= plain.value
    if sp.value > 1:
        assert need_gemm[wide] > need_gemm[d]
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    if du + need_gemm[wide] > plain.value:
        rc = L.rec_crossnet_v2_layer_bwd(C.byref(_lib.CrossV2Desc(B, d, 0, 0, 0, 0)), p, p, p, p, p, 0, p, 0, 0, 1, q, wide,
                                         p, p, p, C.c_size_t(plain.value), None)
        assert rc == -3 and b"ld_out" in L.rec_last_error()
