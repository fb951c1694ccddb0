"""Host checks of the word2vec entry points (csrc/w2v_ops.hip): they return before any launch, so they are called here without a
GPU, with dummy non-null pointer values that nothing may dereference."""
import ctypes as C
import os

NEW = ["rec_w2v_analogy_topk", "rec_w2v_sgns_fwd_bwd", "rec_w2v_target_update"]
FWD_PTRS = ("in_ids", "target_ids", "emb", "emb_w", "emb_b", "true_logits", "neg_logits", "g", "d_in", "loss")
UPD_PTRS = ("n_uniq", "uniq_rows", "seg_offset", "sorted_pos", "g", "in_ids", "emb", "emb_w", "emb_b")
TOPK_PTRS = ("a", "b", "c", "W", "cand_values", "cand_ids", "values", "ids")
MB = 1 << 20                                                    # dummy tables sit a megabyte apart: no two overlap


def _p(v):
    return None if v is None else C.c_void_p(v)


def _ptrs(names, given):
    return {n: given.get(n, MB * (i + 1)) for i, n in enumerate(names)}


def _fwd(L, batch=4, D=12, neg=3, V=50, ld_emb=0, ld_w=0, ld_b=0, ld_din=0, status=64 * MB, **ptr):
    v = _ptrs(FWD_PTRS, ptr)
    return L.rec_w2v_sgns_fwd_bwd(batch, D, neg, V, _p(v["in_ids"]), _p(v["target_ids"]), _p(v["emb"]), ld_emb, _p(v["emb_w"]),
                                  ld_w, _p(v["emb_b"]), ld_b, 1.0, _p(v["true_logits"]), _p(v["neg_logits"]), _p(v["g"]),
                                  _p(v["d_in"]), ld_din, _p(v["loss"]), _p(status), None)


def _upd(L, batch=4, D=12, neg=3, V=50, ld_emb=0, ld_w=0, ld_b=0, ld_dw=0, d_w_rows=32 * MB, d_b_rows=33 * MB, **ptr):
    v = _ptrs(UPD_PTRS, ptr)
    return L.rec_w2v_target_update(batch, D, neg, V, _p(v["n_uniq"]), _p(v["uniq_rows"]), _p(v["seg_offset"]), _p(v["sorted_pos"]),
                                   _p(v["g"]), _p(v["in_ids"]), _p(v["emb"]), ld_emb, _p(v["emb_w"]), ld_w, _p(v["emb_b"]), ld_b,
                                   0.25, _p(d_w_rows), ld_dw, _p(d_b_rows), None)


def _topk(L, Q=5, D=12, ld=0, V=300, k=4, tiles=None, status=64 * MB, **ptr):
    from paddlerec_amd import _lib
    v = _ptrs(TOPK_PTRS, ptr)
    if tiles is None:
        tiles = (V + _lib.REC_W2V_TOPK_TILE_ROWS - 1) // _lib.REC_W2V_TOPK_TILE_ROWS
    return L.rec_w2v_analogy_topk(Q, D, ld, V, k, _p(v["a"]), _p(v["b"]), _p(v["c"]), _p(v["W"]), _p(v["cand_values"]),
                                  _p(v["cand_ids"]), tiles, _p(v["values"]), _p(v["ids"]), _p(status), None)


def _refused(L, fn, cases, name):
    for kw, word in cases:
        assert fn(L, **kw) == -1, kw
        assert word in L.rec_last_error() and name in L.rec_last_error(), (kw, L.rec_last_error())


SIZES = [(dict(D=0), b"emb_dim"), (dict(D=1025), b"emb_dim"), (dict(neg=0), b"neg"), (dict(neg=33), b"neg"),
         (dict(batch=-1), b"batch"), (dict(ld_emb=11), b"ld_emb"), (dict(ld_w=11), b"ld_w"), (dict(ld_b=-1), b"ld_b")]


def test_sgns_fwd_bwd_refusals_without_gpu(engine_lib):
    L = engine_lib
    cases = SIZES + [(dict(ld_din=11), b"ld_din")] + [({n: None}, b"null") for n in FWD_PTRS]
    _refused(L, _fwd, cases, b"rec_w2v_sgns_fwd_bwd")
    for kw, _ in cases[5:9]:
        assert b"below the packed width" in (_fwd(L, **kw), L.rec_last_error())[1]
    assert _fwd(L, batch=0, status=None, **dict.fromkeys(FWD_PTRS)) == 0                 # no launch, nothing dereferenced
    assert _fwd(L, batch=0, D=1025) == -1 and _fwd(L, batch=0, neg=33) == -1 and _fwd(L, batch=0, ld_din=11) == -1
    assert _fwd(L, batch=0, D=1024, neg=32) == 0 and _fwd(L, batch=0, D=1, neg=1) == 0   # the limits
    assert _fwd(L, batch=0, ld_emb=12, ld_w=16, ld_b=1, ld_din=13) == 0


def test_target_update_refusals_without_gpu(engine_lib):
    L = engine_lib
    cases = SIZES + [(dict(ld_dw=11), b"ld_dw")] + [({n: None}, b"null") for n in UPD_PTRS]
    _refused(L, _upd, cases, b"rec_w2v_target_update")
    # emb may not share a float with emb_w: the same pointer, and a table that starts inside the other
    _refused(L, _upd, [(dict(emb=8 * MB, emb_w=8 * MB), b"aliases"), (dict(emb=8 * MB, emb_w=8 * MB + 48 * 10), b"aliases"),
                       (dict(emb=8 * MB + 48, emb_w=8 * MB, batch=0), b"aliases")], b"rec_w2v_target_update")
    assert _upd(L, emb=8 * MB, emb_w=8 * MB + 48 * 50, batch=0) == 0                     # back to back is no overlap
    assert _upd(L, batch=0, d_w_rows=None, d_b_rows=None, **dict.fromkeys(UPD_PTRS)) == 0
    assert _upd(L, batch=0, D=1025) == -1 and _upd(L, batch=0, ld_dw=11) == -1
    assert _upd(L, batch=0, D=1024, neg=32) == 0 and _upd(L, batch=0, D=1, neg=1) == 0   # the limits


def test_analogy_topk_refusals_without_gpu(engine_lib):
    from paddlerec_amd import _lib
    L, T = engine_lib, _lib.REC_W2V_TOPK_TILE_ROWS
    cases = [(dict(D=0), b"emb_dim"), (dict(D=1025), b"emb_dim"), (dict(k=0), b"bad k"), (dict(k=9), b"bad k"),
             (dict(Q=-1), b"batch"), (dict(ld=11), b"below the packed width"), (dict(tiles=2), b"n_tiles"),
             (dict(tiles=4), b"n_tiles"), (dict(V=T, tiles=2), b"n_tiles"), (dict(V=T + 1, tiles=1), b"n_tiles"),
             (dict(V=3), b"num_rows")]
    cases += [({n: None}, b"null") for n in TOPK_PTRS]
    _refused(L, _topk, cases, b"rec_w2v_analogy_topk")
    assert _topk(L, Q=0, status=None, **dict.fromkeys(TOPK_PTRS)) == 0
    assert _topk(L, Q=0, k=9) == -1 and _topk(L, Q=0, tiles=2) == -1
    assert _topk(L, Q=0, D=1024, k=8) == 0 and _topk(L, Q=0, D=1, k=1, V=1) == 0 and _topk(L, Q=0, V=T, tiles=1) == 0


def test_the_new_exports_take_no_workspace():
    from paddlerec_amd import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("rec_w2v_"))
    assert names == NEW and not any(n.endswith("_bytes") for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recengine.h")).read()
    for n in NEW:
        decl = header[header.index("int %s(" % n):]
        decl = decl[:decl.index(";")]
        assert "workspace" not in decl and decl.rstrip().endswith("void* stream)"), n            # no workspace; the stream is last
        assert "int %s_workspace_bytes" % n not in header and "int %s_bytes" % n not in header
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[n][1]), n                               # one ctypes entry per argument
        kinds = [C.c_void_p if "*" in a else {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}[a.split()[0]]
                 for a in decl[decl.index("(") + 1:-1].split(",")]
        assert kinds == list(_lib.SIGNATURES[n][1]), n                                            # and of the same kind
    limits = dict(REC_W2V_MAX_DIM=1024, REC_W2V_MAX_NEG=32, REC_W2V_MAX_TOPK=8, REC_W2V_TOPK_TILE_ROWS=_lib.REC_W2V_TOPK_TILE_ROWS)
    for name, value in limits.items():
        assert getattr(_lib, name) == value and "#define %s %d\n" % (name, value) in header
