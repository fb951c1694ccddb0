"""Host checks of the MatchPyramid entry points (csrc/match_pyramid_ops.hip): they return before any launch, so they are called
here without a GPU, with dummy non-null pointer values that nothing may dereference.  Every refusal is -1 with the entry named
in rec_last_error(); batch == 0 returns REC_OK after the checks of the sizes.  No call here passes the checks with a batch."""
import ctypes as C

NEW = ["rec_mpyr_bwd", "rec_mpyr_fwd", "rec_mpyr_hinge"]
MB = 1 << 20
SHIPPED = dict(Ll=20, Lr=500, E=50, K=8, kh=2, kw=10, ph=6, pw=50, sh=6, sw=50, relu=1)      # PH 3, PW 10: 240 features
ORDER = ("Ll", "Lr", "E", "K", "kh", "kw", "ph", "pw", "sh", "sw", "relu")


def _p(v):
    return None if v is None else C.c_void_p(v)


def _ptrs(names, kw, base=1):
    return {n: kw.pop(n, MB * (i + base)) for i, n in enumerate(names)}


def _shape(kw):
    s = dict(SHIPPED)
    for k in ORDER:
        if k in kw:
            s[k] = kw.pop(k)
    if kw.pop("no_shape", False):
        return None, s
    return (C.c_int32 * 11)(*[s[k] for k in ORDER]), s


def _features(s):
    return max(s["K"], 1) * max((s["Ll"] - s["ph"]) // max(s["sh"], 1) + 1, 1) * max((s["Lr"] - s["pw"]) // max(s["sw"], 1) + 1, 1)


def _fwd(L, B=0, V=193368, ldt=None, pad=193367, ldp=None, lda=None, **kw):
    arr, s = _shape(kw)
    v = _ptrs(("left", "right", "table", "conv_w", "conv_b", "pooled", "argmax"), kw)
    assert not kw, kw
    n = _features(s)
    return L.rec_mpyr_fwd(B, arr, V, s["E"] if ldt is None else ldt, pad, _p(v["left"]), _p(v["right"]), _p(v["table"]),
                          _p(v["conv_w"]), _p(v["conv_b"]), _p(v["pooled"]), n if ldp is None else ldp, _p(v["argmax"]),
                          n if lda is None else lda, None, None)


def _bwd(L, B=0, V=193368, ldt=None, pad=193367, lddp=None, lda=None, lddl=None, lddr=None, **kw):
    arr, s = _shape(kw)
    v = _ptrs(("left", "right", "table", "conv_w", "conv_b", "d_pooled", "argmax", "gated", "partials", "dL", "dR", "d_conv_w",
               "d_conv_b"), kw)
    assert not kw, kw
    n = _features(s)
    ld = lambda x, d: d if x is None else x
    return L.rec_mpyr_bwd(B, arr, V, ld(ldt, s["E"]), pad, _p(v["left"]), _p(v["right"]), _p(v["table"]), _p(v["conv_w"]),
                          _p(v["conv_b"]), _p(v["d_pooled"]), ld(lddp, n), _p(v["argmax"]), ld(lda, n), _p(v["gated"]),
                          _p(v["partials"]), _p(v["dL"]), ld(lddl, s["E"]), _p(v["dR"]), ld(lddr, s["E"]), _p(v["d_conv_w"]),
                          _p(v["d_conv_b"]), None)


def _hinge(L, B=0, pairs=64, **kw):
    v = _ptrs(("pred", "loss", "d_pred"), kw)
    assert not kw, kw
    return L.rec_mpyr_hinge(B, pairs, _p(v["pred"]), _p(v["loss"]), _p(v["d_pred"]), None)


def _refused(L, fn, cases, name, **fixed):
    for kw in cases:
        assert fn(L, **fixed, **kw) == -1, kw
        assert name in L.rec_last_error().decode(), (kw, L.rec_last_error())


def _limits():
    from paddlerec_amd import _lib
    return _lib


# a shape the sizes refuse, whatever the batch: checked ahead of the B == 0 return
def _bad_shapes():
    K = _limits()
    return [dict(Ll=0), dict(Lr=0), dict(E=0), dict(K=0), dict(kh=0), dict(kw=0), dict(ph=0), dict(pw=0), dict(sh=0), dict(sw=0),
            dict(kh=21), dict(kw=501), dict(ph=21), dict(pw=501),                       # filter or pool larger than the image
            dict(Ll=K.REC_MPYR_MAX_LEFT + 1), dict(Lr=K.REC_MPYR_MAX_RIGHT + 1), dict(E=K.REC_MPYR_MAX_EMB + 1),
            dict(K=K.REC_MPYR_MAX_WEIGHTS // 20 + 8),                                   # kh * kw * roundup(K, 8) past the weights' LDS
            dict(ph=14),                                                                # (14 + 1) * 509 = 7635 floats past the band
            dict(pw=5, sw=5, ph=2, sh=2),                                               # 8 * 10 * 100 pooled values
            dict(no_shape=True), dict(B=-1), dict(B=1 << 24), dict(V=0), dict(ldt=49)]


def test_fwd_refusals_without_gpu(engine_lib):
    L, K = engine_lib, _limits()
    assert (15 * 509 > K.REC_MPYR_MAX_BAND >= 7 * 509) and 8 * 10 * 100 > K.REC_MPYR_MAX_POOLED >= 240
    assert _fwd(L) == 0                                                        # B == 0: REC_OK after the checks
    assert _fwd(L, left=None, table=None, pooled=None) == 0                    # ... pointers are not looked at
    _refused(L, _fwd, _bad_shapes() + [dict(ldp=239), dict(lda=239)], "rec_mpyr_fwd")
    for name in ("left", "right", "table", "conv_w", "conv_b", "pooled", "argmax"):
        _refused(L, _fwd, [{name: None}], "rec_mpyr_fwd", B=3)
    _refused(L, _fwd, [dict(pooled=5 * MB, table=5 * MB)], "rec_mpyr_fwd", B=3)        # an output that aliases an input


def test_bwd_refusals_without_gpu(engine_lib):
    L = engine_lib
    assert _bwd(L) == 0
    assert _bwd(L, left=None, table=None, dL=None, gated=None) == 0
    _refused(L, _bwd, _bad_shapes() + [dict(lddp=239), dict(lda=239), dict(lddl=49), dict(lddr=49), dict(d_conv_w=None),
                                       dict(d_conv_b=None)], "rec_mpyr_bwd")
    for name in ("left", "right", "table", "conv_w", "conv_b", "d_pooled", "argmax", "gated", "partials", "dL", "dR"):
        _refused(L, _bwd, [{name: None}], "rec_mpyr_bwd", B=3)
    _refused(L, _bwd, [dict(dL=7 * MB, dR=7 * MB), dict(dL=3 * MB, table=3 * MB), dict(gated=6 * MB, d_pooled=6 * MB)],
             "rec_mpyr_bwd", B=3)


def test_hinge_refusals_without_gpu(engine_lib):
    L = engine_lib
    assert _hinge(L) == 0 and _hinge(L, pred=None, loss=None, d_pred=None) == 0
    _refused(L, _hinge, [dict(B=-1), dict(B=1 << 31), dict(pairs=0), dict(pairs=-3), dict(B=127), dict(B=128, pairs=65),
                         dict(B=128, pred=None), dict(B=128, loss=None), dict(B=128, d_pred=None),
                         dict(B=128, pred=4 * MB, d_pred=4 * MB), dict(B=128, pred=4 * MB, loss=4 * MB)], "rec_mpyr_hinge")


def test_signatures_and_constants():
    from paddlerec_amd import _lib, ops
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("rec_mpyr_")) == NEW
    assert _lib.SIGNATURES["rec_mpyr_fwd"] == (C.c_int, [I64, P, I64, I64, I64, P, P, P, P, P, P, I64, P, I64, P, P])
    assert _lib.SIGNATURES["rec_mpyr_bwd"] == (C.c_int, [I64, P, I64, I64, I64, P, P, P, P, P, P, I64, P, I64, P, P, P, I64, P, I64,
                                                         P, P, P])
    assert _lib.SIGNATURES["rec_mpyr_hinge"] == (C.c_int, [I64, I64, P, P, P, P])
    assert _lib.REC_MPYR_SHAPE_LEN == 11 == len(ops.MpyrShape._fields)
    s = ops.MpyrShape(20, 500, 50, 8, 2, 10, 6, 50, 6, 50, 1)
    assert ops.mpyr_pooled_shape(s) == (3, 10) and ops.mpyr_shape_error(s) is None
    assert "band" not in (ops.mpyr_shape_error(s._replace(pool_h=13)) or "") and ops.mpyr_shape_error(s._replace(pool_h=14))
    for bad in (s._replace(left_len=33), s._replace(right_len=1025), s._replace(emb_dim=129), s._replace(channels=60),
                s._replace(filter_h=21), s._replace(pool_w=501), s._replace(stride_h=0)):
        assert ops.mpyr_shape_error(bad), bad
