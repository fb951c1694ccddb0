"""Host checks of the TiSASRec entry points (csrc/tisas_ops.hip): they return before any launch, so they are called here
without a GPU, with dummy non-null pointer values that nothing may dereference.  None of them takes a workspace (the last test
pins that): the buffers a call needs beyond its results are named arguments whose sizes follow from the shapes."""
import ctypes as C
import os

NEW = ["rec_affine_layer_norm_bwd", "rec_affine_layer_norm_fwd", "rec_tisas_attn_bwd", "rec_tisas_attn_fwd", "rec_tisas_embed_bwd",
       "rec_tisas_embed_fwd", "rec_tisas_head"]
MB = 1 << 20
ATT_PTRS = ("q", "k", "v", "tm", "log_seqs", "out", "lse", "d_out", "gs", "ga", "dq", "dk", "dv", "partials")


def _p(v):
    return None if v is None else C.c_void_p(v)


def _arr(ctype, vals):
    return None if vals is None else (ctype * len(vals))(*vals)


def _att(L, bwd=False, batch=2, seq=5, H=2, D=6, T=4, ld=(6, 6, 6), ldo=6, probs=(0.0, 0.0, 0.0), scale=0.5,
         tables=(100 * MB, 101 * MB, 102 * MB, 103 * MB), d_tables=(110 * MB, 111 * MB, 112 * MB, 113 * MB), streams=(1, 2, 3, 4, 5),
         ldg=(6, 6, 6), **ptr):
    v = {n: ptr.get(n, MB * (i + 1)) for i, n in enumerate(ATT_PTRS)}
    common = (batch, seq, H, D, T, _p(v["q"]), ld[0], _p(v["k"]), ld[1], _p(v["v"]), ld[2], _arr(C.c_void_p, tables), _p(v["tm"]),
              _p(v["log_seqs"]), scale, _arr(C.c_float, probs), 7, _arr(C.c_uint64, streams))
    if not bwd:
        return L.rec_tisas_attn_fwd(*common, _p(v["out"]), ldo, _p(v["lse"]), None, None)
    return L.rec_tisas_attn_bwd(*common, _p(v["d_out"]), ldo, _p(v["lse"]), _p(v["gs"]), _p(v["ga"]), _p(v["dq"]), ldg[0],
                                _p(v["dk"]), ldg[1], _p(v["dv"]), ldg[2], _arr(C.c_void_p, d_tables), _p(v["partials"]), 0, None)


def _refused(L, fn, cases, name, **fixed):
    for kw in cases:
        assert fn(L, **fixed, **kw) == -1, kw
        assert name in L.rec_last_error(), (kw, L.rec_last_error())


def test_attention_refusals_without_gpu(engine_lib):
    from paddlerec_amd import _lib
    L = engine_lib
    assert (_lib.REC_TISAS_MAX_L, _lib.REC_TISAS_MAX_HEAD, _lib.REC_TISAS_MAX_TILE, _lib.REC_TISAS_MAX_TIME_TILE) == (128, 64, 7168, 16384)
    sizes = [dict(batch=-1), dict(seq=0), dict(seq=129), dict(H=0), dict(H=4), dict(D=0), dict(T=0), dict(D=65, H=1, ld=(65,) * 3, ldo=65),
             dict(seq=128, D=64, H=1, ld=(64,) * 3, ldo=64),                       # 128 * 65 > REC_TISAS_MAX_TILE
             dict(ld=(5, 6, 6)), dict(ld=(6, 5, 6)), dict(ld=(6, 6, 5)), dict(ldo=5), dict(probs=(1.0, 0.0, 0.0)),
             dict(probs=(0.0, -0.1, 0.0)), dict(probs=(0.0, 0.0, 1.5)), dict(scale=float("inf")), dict(tables=None),
             dict(probs=None), dict(streams=None), dict(tables=(100 * MB, 0, 102 * MB, 103 * MB))]
    for bwd, name, ptrs in ((False, b"rec_tisas_attn_fwd", ("q", "k", "v", "tm", "log_seqs", "out", "lse")),
                            (True, b"rec_tisas_attn_bwd", ("q", "k", "v", "tm", "log_seqs", "d_out", "lse", "gs", "ga", "dq", "dk",
                                                           "dv", "partials"))):
        _refused(L, _att, sizes + [{n: None} for n in ptrs], name, bwd=bwd)
        # the shipped shape, L 70 and the corners of the limits pass the host checks (batch 0: nothing is launched)
        for ok in (dict(seq=50, D=50, H=1, T=257, ld=(50,) * 3, ldo=50, ldg=(50,) * 3), dict(seq=70, D=50, H=1, T=257, ld=(50,) * 3, ldo=50),
                   dict(seq=128, D=55, H=1, ld=(55,) * 3, ldo=55), dict(seq=110, D=64, H=1, ld=(64,) * 3, ldo=64),
                   dict(seq=1, D=1, H=1, T=1, ld=(1,) * 3, ldo=1)):
            assert _att(L, bwd=bwd, batch=0, **ok) == 0, (name, ok, L.rec_last_error())
        assert _att(L, bwd=bwd, batch=0, **dict.fromkeys(ATT_PTRS)) == 0
        assert _att(L, bwd=bwd, batch=0, seq=129) == -1 and _att(L, bwd=bwd, batch=0, probs=(0.0, 1.0, 0.0)) == -1
    _refused(L, _att, [dict(out=1 * MB)], b"aliases", bwd=False)                    # out is q
    _refused(L, _att, [dict(ldg=(5, 6, 6)), dict(ldg=(6, 5, 6)), dict(ldg=(6, 6, 5)), dict(dq=1 * MB), dict(dk=11 * MB),
                       dict(gs=10 * MB), dict(d_tables=None), dict(d_tables=(110 * MB, 0, 112 * MB, 113 * MB)),
                       dict(d_tables=(100 * MB, 111 * MB, 112 * MB, 113 * MB)),
                       dict(T=257, D=64, H=1, ld=(64,) * 3, ldo=64, ldg=(64,) * 3)],      # 257 * 64 > REC_TISAS_MAX_TIME_TILE
             b"rec_tisas_attn_bwd", bwd=True)
    assert _att(L, bwd=False, batch=0, T=257, D=64, H=1, ld=(64,) * 3, ldo=64) == 0       # the forward keeps no time tile


def _ln_fwd(L, m=4, n=6, x=MB, ldx=6, r=2 * MB, ldr=6, gamma=3 * MB, beta=4 * MB, eps=1e-8, ids=5 * MB, s=6 * MB, lds=6, y=7 * MB,
            ldy=6, mean=8 * MB, rstd=9 * MB):
    return L.rec_affine_layer_norm_fwd(m, n, _p(x), ldx, _p(r), ldr, _p(gamma), _p(beta), eps, _p(ids), _p(s), lds, _p(y), ldy,
                                       _p(mean), _p(rstd), None)


def _ln_bwd(L, m=4, n=6, t=MB, ldt=6, mean=2 * MB, rstd=3 * MB, gamma=4 * MB, dy=5 * MB, lddy=6, dy2=6 * MB, lddy2=6, e1=7 * MB,
            lde1=6, e2=8 * MB, lde2=6, ids=9 * MB, dx=10 * MB, lddx=6, dgamma=11 * MB, dbeta=12 * MB):
    return L.rec_affine_layer_norm_bwd(m, n, _p(t), ldt, _p(mean), _p(rstd), _p(gamma), _p(dy), lddy, _p(dy2), lddy2, _p(e1), lde1,
                                       _p(e2), lde2, _p(ids), _p(dx), lddx, _p(dgamma), _p(dbeta), None)


def test_affine_layer_norm_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _ln_fwd, [dict(m=-1), dict(n=0), dict(eps=-1.0), dict(ldx=5), dict(ldr=5), dict(lds=5), dict(ldy=5), dict(x=None),
                          dict(y=None), dict(mean=None), dict(rstd=None), dict(gamma=None), dict(beta=None), dict(y=MB),
                          dict(y=2 * MB), dict(y=6 * MB), dict(s=2 * MB)], b"rec_affine_layer_norm_fwd")
    assert _ln_fwd(L, m=0, x=None, y=None, mean=None, rstd=None, r=None, s=None, ids=None) == 0
    assert _ln_fwd(L, m=0, gamma=None) == -1 and _ln_fwd(L, m=0, n=0) == -1
    _refused(L, _ln_bwd, [dict(m=-1), dict(n=0), dict(ldt=5), dict(lddy=5), dict(lddy2=5), dict(lde1=5), dict(lde2=5), dict(lddx=5),
                          dict(t=None), dict(mean=None), dict(rstd=None), dict(gamma=None), dict(dy=None), dict(dx=None),
                          dict(dgamma=None), dict(dbeta=None), dict(dbeta=11 * MB), dict(dx=MB), dict(dx=6 * MB), dict(dx=7 * MB),
                          dict(dx=8 * MB)], b"rec_affine_layer_norm_bwd")
    assert _ln_bwd(L, m=-1, dgamma=None) == -1


def _embed(L, bwd=False, n=4, dim=6, rows=9, ids=MB, src=2 * MB, ld_src=6, scale=2.0, p=0.0, out=3 * MB, ldo=6):
    if bwd:
        return L.rec_tisas_embed_bwd(n, dim, rows, _p(ids), _p(src), ld_src, scale, p, 7, 3, _p(out), ldo, None)
    return L.rec_tisas_embed_fwd(n, dim, rows, _p(ids), _p(src), ld_src, scale, p, 7, 3, _p(out), ldo, None, None)


def test_embed_refusals_without_gpu(engine_lib):
    L = engine_lib
    cases = [dict(n=-1), dict(dim=0), dict(rows=0), dict(p=1.0), dict(p=-0.5), dict(scale=float("nan")), dict(ids=None), dict(src=None),
             dict(out=None), dict(out=2 * MB), dict(ld_src=5), dict(ldo=5)]
    for bwd, name in ((False, b"rec_tisas_embed_fwd"), (True, b"rec_tisas_embed_bwd")):
        _refused(L, _embed, cases, name, bwd=bwd)
        assert _embed(L, bwd=bwd, n=0, ids=None, src=None, out=None) == 0 and _embed(L, bwd=bwd, n=0, dim=0) == -1


def _head(L, n=4, dim=6, rows=9, feats=MB, ldf=6, pos=2 * MB, neg=3 * MB, table=4 * MB, ldt=6, loss2=5 * MB, row_loss=6 * MB,
          pl=7 * MB, nl=8 * MB, cp=9 * MB, cn=10 * MB, d_feats=11 * MB, lddf=6, dpr=12 * MB, ldp=6, dnr=13 * MB, ldn=6):
    return L.rec_tisas_head(n, dim, rows, _p(feats), ldf, _p(pos), _p(neg), _p(table), ldt, _p(loss2), _p(row_loss), _p(pl), _p(nl),
                            _p(cp), _p(cn), _p(d_feats), lddf, _p(dpr), ldp, _p(dnr), ldn, None, None)


def test_head_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _head, [dict(n=-1), dict(dim=0), dict(dim=1025), dict(rows=0), dict(ldf=5), dict(ldt=5), dict(lddf=5), dict(ldp=5),
                        dict(ldn=5), dict(feats=None), dict(pos=None), dict(neg=None), dict(table=None), dict(loss2=None),
                        dict(row_loss=None), dict(cp=None), dict(cn=None), dict(d_feats=None), dict(d_feats=MB), dict(dpr=MB),
                        dict(dnr=MB)], b"rec_tisas_head")
    assert _head(L, n=-1, loss2=None) == -1


def test_the_new_exports_take_no_workspace():
    from paddlerec_amd import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("rec_tisas_", "rec_affine_layer_norm")))
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
    for name, value in dict(REC_TISAS_MAX_L=128, REC_TISAS_MAX_HEAD=64, REC_TISAS_MAX_TILE=7168, REC_TISAS_MAX_TIME_TILE=16384,
                            REC_TISAS_MAX_PARTIALS=128, REC_TISAS_HEAD_MAX_DIM=1024).items():
        assert getattr(_lib, name) == value and "#define %s %d\n" % (name, value) in header
