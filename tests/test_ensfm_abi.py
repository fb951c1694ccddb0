"""Host checks of the ENSFM entry points (csrc/ensfm_ops.hip): they return before any launch, so they are called here without
a GPU, with dummy non-null pointer values that nothing may dereference.  None of them takes a workspace (the last test pins
that): the buffers a call needs beyond its results are named arguments whose sizes follow from the shapes."""
import ctypes as C
import os

NEW = ["rec_ensfm_gram", "rec_ensfm_loss", "rec_ensfm_pos_item", "rec_ensfm_pos_user", "rec_ensfm_score", "rec_ensfm_tower_bwd",
       "rec_ensfm_tower_fwd"]
MB = 1 << 20
INF, NAN = float("inf"), float("nan")


def _p(v):
    return None if v is None else C.c_void_p(v)


def _refused(L, fn, cases, name, **fixed):
    for kw in cases:
        assert fn(L, **fixed, **kw) == -1, kw
        assert name in L.rec_last_error(), (kw, L.rec_last_error())


def _ptrs(names, kw, base=1):
    return {n: kw.pop(n, MB * (i + base)) for i, n in enumerate(names)}


def _tower_fwd(L, n=4, F=3, D=6, rows=9, brows=9, ldt=6, item=0, ldo=8, **kw):
    v = _ptrs(("ids", "table", "bias_table", "H_s", "bias", "out"), kw)
    assert not kw, kw
    return L.rec_ensfm_tower_fwd(n, F, D, rows, brows, _p(v["ids"]), _p(v["table"]), ldt, _p(v["bias_table"]), _p(v["H_s"]),
                                 _p(v["bias"]), item, _p(v["out"]), ldo, None, None)


def _tower_bwd(L, n=4, F=3, D=6, rows=9, ldt=6, ldd=8, item=0, ldr=6, acc=0, **kw):
    v = _ptrs(("ids", "table", "H_s", "d_out", "rows_", "dscore", "partials", "dH_s", "dbias"), kw)
    assert not kw, kw
    return L.rec_ensfm_tower_bwd(n, F, D, rows, _p(v["ids"]), _p(v["table"]), ldt, _p(v["H_s"]), _p(v["d_out"]), ldd, item,
                                 _p(v["rows_"]), ldr, _p(v["dscore"]), _p(v["partials"]), _p(v["dH_s"]), _p(v["dbias"]), acc, None)


def _gram(L, n=5, cols=8, ldx=8, **kw):
    v = _ptrs(("X", "partials", "G"), kw)
    assert not kw, kw
    return L.rec_ensfm_gram(n, cols, _p(v["X"]), ldx, _p(v["partials"]), _p(v["G"]), None)


def _pos_user(L, B=3, P=7, D=6, I=6, w=0.5, ldp=8, ldq=8, lddp=8, **kw):
    v = _ptrs(("ur", "p", "q", "H_i", "G_q", "g", "pos_r", "dP", "loss_part", "dHi_part"), kw)
    assert not kw, kw
    return L.rec_ensfm_pos_user(B, P, D, I, w, _p(v["ur"]), _p(v["p"]), ldp, _p(v["q"]), ldq, _p(v["H_i"]), _p(v["G_q"]), _p(v["g"]),
                                _p(v["pos_r"]), _p(v["dP"]), lddp, _p(v["loss_part"]), _p(v["dHi_part"]), None, None)


def _pos_item(L, B=3, P=7, D=6, I=6, w=0.5, ldp=8, ldq=8, lddq=8, **kw):
    v = _ptrs(("n_uniq", "uniq_rows", "seg_offset", "sorted_pos", "g", "p", "q", "H_i", "G_p", "dQ"), kw)
    assert not kw, kw
    return L.rec_ensfm_pos_item(B, P, D, I, w, _p(v["n_uniq"]), _p(v["uniq_rows"]), _p(v["seg_offset"]), _p(v["sorted_pos"]),
                                _p(v["g"]), _p(v["p"]), ldp, _p(v["q"]), ldq, _p(v["H_i"]), _p(v["G_p"]), _p(v["dQ"]), lddq, None)


def _loss(L, B=3, D=6, w=0.5, **kw):
    v = _ptrs(("G_p", "G_q", "H_i", "loss_part", "dHi_part", "loss", "dH_i"), kw)
    assert not kw, kw
    return L.rec_ensfm_loss(B, D, w, _p(v["G_p"]), _p(v["G_q"]), _p(v["H_i"]), _p(v["loss_part"]), _p(v["dHi_part"]), _p(v["loss"]),
                            _p(v["dH_i"]), None)


def _score(L, B=3, rows=7, D=6, ldp=8, ldq=8, ldpre=7, **kw):
    v = _ptrs(("p", "q", "H_i", "pre"), kw)
    assert not kw, kw
    return L.rec_ensfm_score(B, rows, D, _p(v["p"]), ldp, _p(v["q"]), ldq, _p(v["H_i"]), _p(v["pre"]), ldpre, None)


def test_tower_refusals_without_gpu(engine_lib):
    from paddlerec_amd import _lib
    L = engine_lib
    assert (_lib.REC_ENSFM_MAX_DIM, _lib.REC_ENSFM_MAX_PARTIALS, _lib.REC_ENSFM_GRAM_MAX_BLOCKS) == (128, 1024, 256)
    _refused(L, _tower_fwd, [dict(n=-1), dict(F=0), dict(D=0), dict(D=129, ldt=129, ldo=131), dict(rows=0), dict(brows=0),
                             dict(ldt=5), dict(ldo=7), dict(ids=None), dict(table=None), dict(bias_table=None), dict(H_s=None),
                             dict(out=None), dict(out=2 * MB), dict(out=3 * MB), dict(out=4 * MB), dict(out=5 * MB),
                             dict(n=1 << 30, F=4)], b"rec_ensfm_tower_fwd")
    for ok in (dict(F=4, D=64, rows=6069, brows=6069, ldt=64, ldo=66), dict(F=2, D=64, rows=3954, brows=3953, ldt=64, ldo=66, item=1),
               dict(F=1, D=1, rows=1, brows=1, ldt=1, ldo=3), dict(D=128, ldt=128, ldo=130)):
        assert _tower_fwd(L, n=0, **ok) == 0, (ok, L.rec_last_error())
    assert _tower_fwd(L, n=0, ids=None, table=None, bias_table=None, H_s=None, bias=None, out=None) == 0
    assert _tower_fwd(L, n=0, D=129, ldt=129, ldo=131) == -1 and _tower_fwd(L, n=0, ldo=7) == -1
    _refused(L, _tower_bwd, [dict(n=-1), dict(F=0), dict(D=0), dict(D=129, ldt=129, ldd=131, ldr=129), dict(rows=0), dict(ldt=5),
                             dict(ldd=7), dict(ldr=5), dict(ids=None), dict(table=None), dict(H_s=None), dict(d_out=None),
                             dict(rows_=None), dict(dscore=None), dict(partials=None), dict(dH_s=None), dict(dH_s=3 * MB),
                             dict(dH_s=9 * MB), dict(rows_=2 * MB), dict(rows_=4 * MB), dict(dscore=5 * MB), dict(partials=6 * MB),
                             dict(dbias=5 * MB), dict(dscore=2 * MB), dict(n=1 << 30, F=4)], b"rec_ensfm_tower_bwd",)
    for ok in (dict(F=4, D=64, rows=6069, ldt=64, ldd=66, ldr=64), dict(F=2, D=64, rows=3954, ldt=64, ldd=66, ldr=64, item=1, acc=1),
               dict(F=1, D=1, rows=1, ldt=1, ldd=3, ldr=1), dict(D=128, ldt=128, ldd=130, ldr=128)):
        assert _tower_bwd(L, n=0, **ok) == 0, (ok, L.rec_last_error())
    assert _tower_bwd(L, n=0, ids=None, table=None, H_s=None, d_out=None, rows_=None, dscore=None, partials=None, dbias=None) == 0
    assert _tower_bwd(L, n=0, dH_s=None) == -1 and _tower_bwd(L, n=0, D=0) == -1


def test_gram_and_loss_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _gram, [dict(n=-1), dict(cols=0), dict(cols=131, ldx=131), dict(ldx=7), dict(X=None), dict(G=None), dict(partials=None),
                        dict(G=2 * MB), dict(X=3 * MB), dict(X=2 * MB)], b"rec_ensfm_gram")
    assert _gram(L, n=0, G=None) == -1 and _gram(L, n=0, cols=131, ldx=131) == -1
    for ok in (dict(cols=66, ldx=66), dict(cols=1, ldx=1), dict(cols=130, ldx=130), dict(X=None)):
        assert _gram(L, n=0, **ok) == 0, (ok, L.rec_last_error())
    _refused(L, _loss, [dict(B=-1), dict(D=0), dict(D=129), dict(w=INF), dict(w=NAN), dict(G_p=None), dict(G_q=None), dict(H_i=None),
                        dict(loss=None), dict(dH_i=None), dict(loss_part=None), dict(dHi_part=None), dict(dH_i=6 * MB),
                        dict(dH_i=3 * MB), dict(loss=MB), dict(loss=4 * MB), dict(dH_i=5 * MB)], b"rec_ensfm_loss")
    assert _loss(L, B=0, D=129) == -1 and _loss(L, B=0, w=NAN) == -1
    for ok in (dict(D=64), dict(D=1), dict(D=128), dict(loss_part=None, dHi_part=None)):
        assert _loss(L, B=0, **ok) == 0, (ok, L.rec_last_error())


def test_positives_refusals_without_gpu(engine_lib):
    L = engine_lib
    common = [dict(B=-1), dict(P=0), dict(D=0), dict(D=129, ldp=131, ldq=131), dict(I=0), dict(w=INF), dict(w=NAN), dict(ldp=7),
              dict(ldq=7), dict(B=1 << 20, P=1 << 11)]
    _refused(L, _pos_user, common + [dict(lddp=7), dict(ur=None), dict(p=None), dict(q=None), dict(H_i=None), dict(G_q=None),
                                     dict(g=None), dict(dP=None), dict(loss_part=None), dict(dHi_part=None), dict(g=2 * MB),
                                     dict(dP=3 * MB), dict(pos_r=5 * MB), dict(dP=6 * MB), dict(loss_part=8 * MB),
                                     dict(dHi_part=9 * MB), dict(pos_r=6 * MB)], b"rec_ensfm_pos_user")
    assert _pos_user(L, pos_r=None, B=0) == 0
    for ok in (dict(B=0, P=2048, D=64, I=3706, ldp=66, ldq=66, lddp=66), dict(B=0, P=1, D=1, I=1, ldp=3, ldq=3, lddp=3),
               dict(B=0, D=128, ldp=130, ldq=130, lddp=130)):
        assert _pos_user(L, **ok) == 0, (ok, L.rec_last_error())
    assert _pos_user(L, B=0, ur=None, p=None, q=None, H_i=None, G_q=None, g=None, pos_r=None, dP=None, loss_part=None,
                     dHi_part=None) == 0
    assert _pos_user(L, B=0, D=129, ldp=131, ldq=131, lddp=131) == -1 and _pos_user(L, B=0, w=INF) == -1
    _refused(L, _pos_item, common + [dict(lddq=7), dict(n_uniq=None), dict(uniq_rows=None), dict(seg_offset=None),
                                     dict(sorted_pos=None), dict(g=None), dict(p=None), dict(q=None), dict(H_i=None),
                                     dict(G_p=None), dict(dQ=None), dict(dQ=7 * MB), dict(dQ=6 * MB), dict(dQ=5 * MB),
                                     dict(dQ=9 * MB)], b"rec_ensfm_pos_item")
    assert _pos_item(L, B=0, D=129, ldp=131, ldq=131, lddq=131) == -1 and _pos_item(L, B=0, w=NAN) == -1 \
        and _pos_item(L, B=0, dQ=None) == -1
    for ok in (dict(P=2048, D=64, I=3706, ldp=66, ldq=66, lddq=66), dict(P=1, D=1, I=1, ldp=3, ldq=3, lddq=3),
               dict(D=128, ldp=130, ldq=130, lddq=130), dict(n_uniq=None, uniq_rows=None, seg_offset=None, sorted_pos=None, g=None, p=None)):
        assert _pos_item(L, B=0, **ok) == 0, (ok, L.rec_last_error())


def test_score_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _score, [dict(B=-1), dict(rows=0), dict(D=0), dict(D=129, ldp=131, ldq=131), dict(ldp=7), dict(ldq=7), dict(ldpre=6),
                         dict(p=None), dict(q=None), dict(H_i=None), dict(pre=None), dict(pre=MB), dict(pre=2 * MB), dict(pre=3 * MB),
                         dict(B=1 << 21)], b"rec_ensfm_score")
    for ok in (dict(rows=3707, D=64, ldp=66, ldq=66, ldpre=3707), dict(rows=1, D=1, ldp=3, ldq=3, ldpre=1),
               dict(D=128, ldp=130, ldq=130)):
        assert _score(L, B=0, **ok) == 0, (ok, L.rec_last_error())
    assert _score(L, B=0, p=None, q=None, H_i=None, pre=None) == 0 and _score(L, B=0, D=129, ldp=131, ldq=131) == -1


def test_the_new_exports_take_no_workspace():
    from paddlerec_amd import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("rec_ensfm_"))
    assert names == NEW and not any(n.endswith("_bytes") for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recengine.h")).read()
    kinds_of = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "uint64_t": C.c_uint64}
    for n in NEW:
        decl = header[header.index("int %s(" % n):]
        decl = decl[:decl.index(";")]
        assert "workspace" not in decl and decl.rstrip().endswith("void* stream)"), n            # no workspace; the stream is last
        assert "int %s_workspace_bytes" % n not in header and "int %s_bytes" % n not in header
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[n][1]) <= 33, n                         # one ctypes entry per argument
        kinds = [C.c_void_p if "*" in a else kinds_of[a.split()[0]] for a in decl[decl.index("(") + 1:-1].split(",")]
        assert kinds == list(_lib.SIGNATURES[n][1]), n                                            # and of the same kind
    for name, value in dict(REC_ENSFM_MAX_DIM=128, REC_ENSFM_MAX_PARTIALS=1024, REC_ENSFM_GRAM_MAX_BLOCKS=256).items():
        assert getattr(_lib, name) == value and "#define %s %d\n" % (name, value) in header
