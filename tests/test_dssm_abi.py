"""Host checks of the DSSM entry points (csrc/dssm_ops.hip): they return before any launch, so they are called here without a
GPU, with dummy non-null pointer values that nothing may dereference.  Every refusal is -1 with the entry named in
rec_last_error(); a call with no rows returns REC_OK after the checks of the sizes."""
import ctypes as C

NEW = ["rec_dssm_cos", "rec_dssm_head_step", "rec_dssm_lod_rows", "rec_dssm_sparse_linear_bwd", "rec_dssm_sparse_linear_fwd"]
MB = 1 << 20


def _p(v):
    return None if v is None else C.c_void_p(v)


def _ptrs(names, kw, base=1):
    return {n: kw.pop(n, MB * (i + base)) for i, n in enumerate(names)}


def _refused(L, fn, cases, name, **fixed):
    for kw in cases:
        assert fn(L, **fixed, **kw) == -1, kw
        assert name in L.rec_last_error(), (kw, L.rec_last_error())


def _lod_rows(L, rows=5, nnz=40, **kw):
    v = _ptrs(("lod", "row_of"), kw)
    assert not kw, kw
    return L.rec_dssm_lod_rows(rows, nnz, _p(v["lod"]), _p(v["row_of"]), None)


def _fwd(L, rows=5, nnz=40, T=2900, n=300, relu=1, ldw=None, ldy=None, **kw):
    v = _ptrs(("cols", "vals", "lod", "W", "bias", "Y"), kw)
    assert not kw, kw
    return L.rec_dssm_sparse_linear_fwd(rows, nnz, T, n, relu, _p(v["cols"]), _p(v["vals"]), _p(v["lod"]), _p(v["W"]),
                                        n if ldw is None else ldw, _p(v["bias"]), _p(v["Y"]), n if ldy is None else ldy, None, None)


def _bwd(L, rows=5, nnz=40, T=2900, n=300, lddy=None, lddw=None, **kw):
    v = _ptrs(("vals", "row_of", "sorted_pos", "uniq_rows", "seg_offset", "n_uniq", "dY", "dW"), kw)
    assert not kw, kw
    return L.rec_dssm_sparse_linear_bwd(rows, nnz, T, n, _p(v["vals"]), _p(v["row_of"]), _p(v["sorted_pos"]), _p(v["uniq_rows"]),
                                        _p(v["seg_offset"]), _p(v["n_uniq"]), _p(v["dY"]), n if lddy is None else lddy,
                                        _p(v["dW"]), n if lddw is None else lddw, None)


def _head(L, B=5, neg=1, n=128, slice_end=8, relu=1, ldq=None, ldd=None, lddq=None, lddd=None, **kw):
    v = _ptrs(("q", "d", "cos", "hit_prob", "loss_terms", "loss", "dq", "dd"), kw)
    assert not kw, kw
    ld = lambda x: n if x is None else x
    return L.rec_dssm_head_step(B, neg, n, slice_end, relu, _p(v["q"]), ld(ldq), _p(v["d"]), ld(ldd), _p(v["cos"]),
                                _p(v["hit_prob"]), _p(v["loss_terms"]), _p(v["loss"]), _p(v["dq"]), ld(lddq), _p(v["dd"]),
                                ld(lddd), None)


def _cos(L, B=5, n=128, ldq=None, ldd=None, **kw):
    v = _ptrs(("q", "d", "cos"), kw)
    assert not kw, kw
    return L.rec_dssm_cos(B, n, _p(v["q"]), n if ldq is None else ldq, _p(v["d"]), n if ldd is None else ldd, _p(v["cos"]), None)


def test_lod_rows_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _lod_rows, [dict(rows=-1), dict(rows=1 << 31), dict(nnz=-1), dict(nnz=1 << 31), dict(lod=None), dict(row_of=None),
                            dict(row_of=MB)], b"rec_dssm_lod_rows")
    assert _lod_rows(L, rows=0, lod=None, row_of=None) == 0 and _lod_rows(L, nnz=0, lod=None, row_of=None) == 0
    assert _lod_rows(L, rows=0, nnz=-1) == -1


def test_sparse_linear_fwd_refusals_without_gpu(engine_lib):
    from paddlerec_amd import _lib
    L = engine_lib
    cases = [dict(rows=-1), dict(rows=1 << 31), dict(nnz=-1), dict(nnz=1 << 31), dict(T=0), dict(n=0), dict(n=_lib.REC_DSSM_MAX_WIDTH + 1),
             dict(ldw=299), dict(ldy=299), dict(cols=None), dict(vals=None), dict(lod=None), dict(W=None), dict(bias=None),
             dict(Y=None), dict(Y=2 * MB), dict(Y=4 * MB), dict(Y=5 * MB), dict(rows=(1 << 31) - 1, n=2047)]
    _refused(L, _fwd, cases, b"rec_dssm_sparse_linear_fwd")
    assert _fwd(L, rows=0) == 0 and _fwd(L, rows=0, cols=None, vals=None, lod=None, W=None, bias=None, Y=None) == 0
    assert _fwd(L, rows=0, ldw=304, ldy=512, n=_lib.REC_DSSM_MAX_WIDTH) == -1        # ld below n still refused
    assert _fwd(L, rows=0, ldw=299) == -1 and _fwd(L, rows=0, n=0) == -1 and _fwd(L, rows=0, T=0) == -1


def test_sparse_linear_bwd_refusals_without_gpu(engine_lib):
    from paddlerec_amd import _lib
    L = engine_lib
    cases = [dict(rows=-1), dict(rows=1 << 31), dict(nnz=-1), dict(nnz=1 << 31), dict(T=0), dict(T=1 << 31), dict(n=0),
             dict(n=_lib.REC_DSSM_MAX_WIDTH + 1), dict(lddy=299), dict(lddw=299), dict(vals=None), dict(row_of=None),
             dict(sorted_pos=None), dict(uniq_rows=None), dict(seg_offset=None), dict(n_uniq=None), dict(dY=None), dict(dW=None),
             dict(dW=7 * MB), dict(dW=MB)]
    _refused(L, _bwd, cases, b"rec_dssm_sparse_linear_bwd")
    # no early return: every row of dW is written even when the batch holds no entry, so dW and the grouping stay required
    assert _bwd(L, nnz=0, dW=None) == -1 and _bwd(L, rows=0, n_uniq=None) == -1


def test_head_step_refusals_without_gpu(engine_lib):
    from paddlerec_amd import _lib
    L = engine_lib
    cases = [dict(B=-1), dict(B=1 << 25), dict(neg=-1), dict(neg=_lib.REC_DSSM_MAX_DOCS), dict(n=0), dict(slice_end=0),
             dict(slice_end=-3), dict(ldq=127), dict(ldd=127), dict(lddq=127), dict(lddd=127), dict(q=None), dict(d=None),
             dict(cos=None), dict(hit_prob=None), dict(loss_terms=None), dict(loss=None), dict(dq=None), dict(dd=None),
             dict(dq=MB), dict(dd=2 * MB), dict(cos=MB), dict(loss=2 * MB), dict(dq=8 * MB)]
    _refused(L, _head, cases, b"rec_dssm_head_step")
    for neg in (0, 1, 4, _lib.REC_DSSM_MAX_DOCS - 1):
        assert _head(L, B=0, neg=neg) == 0, L.rec_last_error()
    assert _head(L, B=0, q=None, d=None, cos=None, hit_prob=None, loss_terms=None, dq=None, dd=None) == 0
    assert _head(L, B=0, loss=None) == -1 and _head(L, B=0, ldq=127) == -1 and _head(L, B=0, slice_end=0) == -1


def test_cos_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _cos, [dict(B=-1), dict(B=1 << 31), dict(n=0), dict(ldq=127), dict(ldd=127), dict(q=None), dict(d=None),
                       dict(cos=None), dict(cos=MB), dict(cos=2 * MB)], b"rec_dssm_cos")
    assert _cos(L, B=0) == 0 and _cos(L, B=0, q=None, d=None, cos=None) == 0 and _cos(L, B=0, ldd=127) == -1


def test_the_header_lists_exactly_these_entries():
    from paddlerec_amd import _lib
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("rec_dssm_")) == NEW
    assert (_lib.REC_DSSM_MAX_DOCS, _lib.REC_DSSM_MAX_WIDTH, _lib.REC_DSSM_BWD_WAVES) == (64, 2048, 8)
    assert 4 * _lib.REC_DSSM_BWD_WAVES * _lib.REC_DSSM_MAX_WIDTH == 64 << 10          # the backward's LDS at the widest layer
    for n in NEW:
        assert _lib.SIGNATURES[n][1][-1] is C.c_void_p                               # the stream is last
        assert C.c_size_t not in _lib.SIGNATURES[n][1]                               # no entry takes a workspace
    assert _lib.SIGNATURES["rec_dssm_sparse_linear_fwd"][1][-2] is C.c_void_p         # the status word
