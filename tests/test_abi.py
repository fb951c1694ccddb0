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


def test_route_log_without_gpu(engine_lib):
    """rec_route_log_begin / rec_route_log_end are host bookkeeping: they answer on a GPU-less host.  An empty log is one
    NUL byte; a buffer that cannot hold the notes is refused and named; a call refused before it chooses a kernel
    leaves no note; ops.route_log() yields the notes as a list."""
    import ctypes as C
    from paddlerec_amd import ops
    L = engine_lib
    buf, need = C.create_string_buffer(b"x" * 8, 8), C.c_size_t(99)
    assert L.rec_route_log_begin() == 0
    assert L.rec_sparse_adam_rows(10, 16, 8, 0, None, None, None, None, None, None, None, None, None, None, None,
                                  None) == -1                                       # row_stride < emb_dim: refused
    assert L.rec_route_log_end(None, 0, C.byref(need)) == -1 and need.value == 1 and b"route log" in L.rec_last_error()
    assert L.rec_route_log_end(buf, 0, None) == -1
    assert L.rec_route_log_end(buf, 1, C.byref(need)) == 0 and buf.raw[:1] == b"\0" and need.value == 1
    assert L.rec_route_log_end(buf, 8, None) == 0 and buf.value == b""                # end without begin: the last log
    with ops.route_log() as notes:
        assert notes == []
    assert notes == []


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


# ------------------------------------------------------------------------------------------------ the parsed binding
# paddlerec_amd/_lib.py derives constants, structs and signatures from include/recengine.h.  A comparison of the binding
# with the header is therefore header against header; what follows pins the PARSER: against literals written out by
# hand, against the host compiler's layout of every struct, and on text it has to refuse.
def test_parsed_signatures_match_literals():
    import ctypes as C
    from paddlerec_amd import _lib
    P, I64, I32, F, SZ = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
    S = _lib.SIGNATURES
    assert S["rec_last_error"] == (C.c_char_p, [])
    assert S["rec_ps_init_value_host"] == (C.c_float, [C.c_uint64, I64, I32, F])
    assert S["rec_xxh32"] == (C.c_uint32, [P, SZ, C.c_uint32])
    assert S["rec_gemm_f32"] == (C.c_int, [C.POINTER(_lib.GemmDesc), P, P, P, C.POINTER(_lib.GemmEpilogueArgs), P, SZ, P])
    assert S["rec_w2v_sgns_fwd_bwd"] == (C.c_int, [I64, I32, I32, I64, P, P, P, I64, P, I64, P, I64, F, P, P, P, P, I64, P,
                                                   P, P])
    assert S["rec_bst_embed_fwd"] == (C.c_int, [I64, I32, P, P, P, P, P, P, I64, P, I64, P, P])       # T* const* is a pointer
    assert S["rec_autofis_fwd"] == (C.c_int, [I64, I32, I32, I32, I32, I64, P, P, P, I32, P, P, P, P, P, P, P, P, F, F, I32,
                                              I32, P, I64, P, I64, P, P, P, P, P, SZ, P])
    assert len(S["rec_autofis_fwd"][1]) == 33 == max(len(a) for _, a in S.values())


def test_parsed_structs_and_constants_match_literals():
    import ctypes as C
    from paddlerec_amd import _lib
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    assert _lib.GemmDesc is _lib.STRUCTS["rec_gemm_desc"] and _lib.GemmDesc.__name__ == "GemmDesc"
    assert _lib.GemmDesc._fields_ == [("m", I64)] + [(n, I32) for n in (
        "n", "k", "lda", "ldb", "ldc", "trans_a", "trans_b", "epilogue", "split_k", "num_cus")]
    assert _lib.SmallSgdJob._fields_ == [("n", I64), ("emb_dim", I32), ("row_stride", I32), ("num_rows", I64),
                                         ("padding_idx", I64), ("ids", P), ("grad", P),
                                         ("grad_layout", _lib.GradLayout), ("P", P)]              # nested by value
    assert _lib.GradLayout._fields_ == [("div", I32), ("group", I32), ("group_stride", I64), ("partials", P),
                                        ("index", P), ("sorted", I32)]
    assert _lib.MtlMixDesc._fields_ == (
        [("batch", I64), ("expert_size", I32), ("n_slots", I32), ("n_gates", I32)] +
        [(n, I64) for n in ("ld_h", "ld_logit", "ld_prob", "ld_out", "ld_dh", "ld_dlogit")] +
        [(n, I32 * 16) for n in ("first0", "count0", "first1", "count1")])                        # [REC_MTL_MAX_GATES]
    assert _lib.REC_AUC_WIDE_MAX_THRESHOLDS == 16777216 and _lib.REC_EHIP == -4 and _lib.REC_GEMM_ROUTE_PAIR == 64
    assert _lib.EPI == dict(none=0, bias=1, bias_relu=2, relu_mask=3, cross=4, bias_sigmoid=5, bias_tanh=6, add=7, moe=8,
                            dsigmoid=9, dtanh=10)
    assert len(_lib.STRUCTS) == 29 == len(_lib._STRUCT_NAMES) and set(_lib.STRUCTS) == set(_lib._STRUCT_NAMES)


def test_struct_layouts_match_the_host_compiler(tmp_path):
    """sizeof and every offsetof of all structs, as the C compiler lays out include/recengine.h."""
    import ctypes as C
    import shutil
    import subprocess
    import pytest
    from paddlerec_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ['#include <stdio.h>', '#include "recengine.h"', "int main(void) {"]
    want = []
    for cname, cls in sorted(_lib.STRUCTS.items()):
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        want.append("%s %d" % (cname, C.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (cname, field, cname, field, cname, field))
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    got = subprocess.check_output([exe]).decode().split("\n")
    assert len(want) > 29 + 300 and got[:-1] == want


def test_parser_refuses_what_it_does_not_recognise(monkeypatch):
    import pytest
    from paddlerec_amd import _lib
    from paddlerec_amd._lib import RecError, parse_header
    assert _lib.HEADER_PATH == os.path.join(REPO, "include", "recengine.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(REPO, "include", "no_such.h"))
    with pytest.raises(RecError, match="no_such.h"):                                   # a missing header names the path tried
        _lib._read_header()
    ok = "typedef struct { int32_t a, *b; } rec_s;\nint rec_f(const rec_s* s, float x); /* rec_g( */\n"
    consts, structs, sigs = parse_header("#define REC_N (1 << 3)\nenum { REC_A = REC_N + 1 };\n" + ok)
    assert consts == dict(REC_N=8, REC_A=9) and list(structs) == ["rec_s"] and list(sigs) == ["rec_f"]
    for bad, word in (("int rec_f(double x);", "double"),                               # unknown type in a prototype
                      ("int rec_f(double* x);", "double"),                              # ... also behind a pointer
                      ("typedef struct { long a; } rec_s;", "long"),
                      ("typedef struct { int32_t a[REC_NOPE]; } rec_s;", "REC_NOPE"),
                      ("typedef enum { REC_A = 0, REC_B } rec_e;", "REC_B"),            # valueless enumerator
                      ("struct rec_fwd;", "struct rec_fwd"),                            # declarations it cannot place
                      ("int rec_f(int32_t (*cb)(void));", "rec_f"),
                      ("static int rec_x = 3;", "rec_x"),
                      ("int rec_f(void)", "rec_f"),                                     # no terminating ';'
                      ("int rec_f(void);\nint rec_f(void);", "rec_f"),
                      ("#define REC_X 1.5", "REC_X"),
                      ("#if 0\n#endif", "#if 0")):
        with pytest.raises(RecError) as e:
            parse_header(bad)
        assert word in str(e.value), (bad, str(e.value))
