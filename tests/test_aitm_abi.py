"""Host checks of the AITM entry points (csrc/aitm_ops.hip): they return before any launch, so they are called here without a
GPU, with dummy non-null pointer values that nothing may dereference."""
import ctypes as C
import os

NEW = ["rec_ait_bwd", "rec_ait_fwd", "rec_aitm_head", "rec_auc_histogram_wide", "rec_field_gather_fwd"]


def _p(v):
    return None if v is None else C.c_void_p(v)


def _gather(L, batch=4, F=3, D=4, stride=4, ld_out=0, begin=4096, ids=8192, W=12288, out=16384, rows=20480, status=24576):
    return L.rec_field_gather_fwd(batch, F, D, stride, _p(begin), _p(ids), _p(W), _p(out), ld_out, _p(rows), _p(status), None)


def _fwd(L, batch=4, T=2, d=32, ld_qkv=0, ld_out=0, qkv=4096, out=8192, prob=12288):
    return L.rec_ait_fwd(batch, T, d, _p(qkv), ld_qkv, _p(out), ld_out, _p(prob), None)


def _bwd(L, batch=4, T=2, d=32, ld_qkv=0, ld_dout=0, ld_dqkv=0, qkv=4096, prob=8192, dout=12288, dqkv=16384):
    return L.rec_ait_bwd(batch, T, d, _p(qkv), ld_qkv, _p(prob), _p(dout), ld_dout, _p(dqkv), ld_dqkv, None)


def _head(L, batch=4, d=32, ld_click=0, ld_ait=0, dz=49152, **ptr):
    from paddlerec_amd._lib import AitmHeadDesc
    names = ("tower_click", "ait", "w_click", "b_click", "w_conv", "b_conv", "click", "buy", "pred", "cost")
    vals = [ptr.get(n, 4096 * (i + 1)) for i, n in enumerate(names)]
    desc = AitmHeadDesc(batch, d, ld_click, ld_ait, 0.6, 0.25)
    return L.rec_aitm_head(C.byref(desc), *[_p(v) for v in vals], _p(dz), None)


def _auc(L, batch=4, ld=0, T=100000, pred=4096, label=8192, pos=12288, neg=16384):
    return L.rec_auc_histogram_wide(batch, _p(pred), ld, _p(label), T, _p(pos), _p(neg), None)


def _refused(L, fn, cases):
    for kw, word in cases:
        assert fn(L, **kw) == -1, kw
        assert word in L.rec_last_error(), (kw, L.rec_last_error())


def test_field_gather_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _gather, ((dict(D=0), b"emb_dim"), (dict(D=1025, stride=1028), b"emb_dim"), (dict(F=0), b"sizes"),
                          (dict(batch=-1), b"sizes"), (dict(stride=3), b"row_stride"), (dict(ld_out=11), b"below the packed width"),
                          (dict(begin=None), b"null"), (dict(ids=None), b"null"), (dict(W=None), b"null"), (dict(out=None), b"null")))
    assert _gather(L, batch=0, begin=None, ids=None, W=None, out=None, rows=None, status=None) == 0    # nothing to do: no launch
    assert _gather(L, batch=0, ld_out=11) == -1                                                      # ... but the arguments are still checked


def test_ait_refusals_without_gpu(engine_lib):
    L = engine_lib
    both = ((dict(T=0), b"tokens"), (dict(T=9), b"tokens"), (dict(d=0), b"dim"), (dict(d=257), b"dim"), (dict(batch=-1), b"batch"),
            (dict(ld_qkv=95), b"below the packed width"), (dict(qkv=None), b"null"), (dict(prob=None), b"null"))
    _refused(L, _fwd, both + ((dict(ld_out=31), b"below the packed width"), (dict(out=None), b"null")))
    _refused(L, _bwd, both + ((dict(ld_dout=31), b"below the packed width"), (dict(ld_dqkv=95), b"below the packed width"),
                              (dict(dout=None), b"null"), (dict(dqkv=None), b"null")))
    assert b"rec_ait_bwd" in L.rec_last_error()
    assert _fwd(L, batch=0, qkv=None, out=None, prob=None) == 0 and _bwd(L, batch=0, qkv=None, prob=None, dout=None, dqkv=None) == 0
    assert _fwd(L, batch=0, T=9) == -1 and _bwd(L, batch=0, ld_dqkv=95) == -1
    assert _fwd(L, batch=0, T=8, d=256) == 0 and _fwd(L, batch=0, T=1, d=1) == 0                       # the limits themselves


def test_aitm_head_refusals_without_gpu(engine_lib):
    L = engine_lib
    assert L.rec_aitm_head(None, *[C.c_void_p(4096)] * 11, None) == -1 and b"null descriptor" in L.rec_last_error()
    cases = [(dict(batch=-1), b"bad batch"), (dict(d=0), b"bad dim"), (dict(d=4097), b"bad dim"),
             (dict(ld_click=31), b"below the packed width"), (dict(ld_ait=31), b"below the packed width")]
    cases += [({n: None}, b"null") for n in ("tower_click", "ait", "w_click", "b_click", "w_conv", "b_conv", "click", "buy", "pred", "cost")]
    _refused(L, _head, cases)
    none = dict.fromkeys(("tower_click", "ait", "w_click", "b_click", "w_conv", "b_conv", "click", "buy", "pred", "cost"))
    assert _head(L, batch=0, dz=None, **none) == 0
    assert _head(L, batch=0, ld_ait=31) == -1


def test_auc_histogram_wide_refusals_without_gpu(engine_lib):
    L = engine_lib
    _refused(L, _auc, ((dict(T=0), b"num_thresholds"), (dict(T=(1 << 24) + 1), b"num_thresholds"), (dict(batch=-1), b"batch"),
                       (dict(ld=-1), b"below the packed width"), (dict(pred=None), b"null"), (dict(label=None), b"null"),
                       (dict(pos=None), b"null"), (dict(neg=None), b"null")))
    assert _auc(L, batch=0, pred=None, label=None, pos=None, neg=None) == 0 and _auc(L, batch=0, T=1 << 24) == 0
    assert _auc(L, batch=0, T=0) == -1
    # the LDS histogram keeps its limit
    p = C.c_void_p(4096)
    assert L.rec_auc_histogram(4, p, p, 16000, p, p, None) == -1


def test_the_new_exports_take_no_workspace():
    from paddlerec_amd import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("rec_ait", "rec_field_gather", "rec_auc_histogram_wide")))
    assert names == NEW and not any(n.endswith("_bytes") for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recengine.h")).read()
    for n in NEW:
        decl = header[header.index("int %s(" % n):]
        decl = decl[:decl.index(";")]
        assert "workspace" not in decl and decl.rstrip().endswith("void* stream)"), n            # no workspace; the stream is last
        assert "int %s_workspace_bytes" % n not in header and "int %s_bytes" % n not in header
    d = _lib.AitmHeadDesc(7, 32, 0, 0, 0.6, 0.25)
    F = _lib.AitmHeadDesc
    assert C.sizeof(d) == 40 and (F.batch.offset, F.dim.offset, F.ld_click.offset, F.ld_ait.offset, F.constraint_w.offset,
                                  F.grad_scale.offset) == (0, 8, 16, 24, 32, 36)
    assert (_lib.REC_AIT_MAX_TOKENS, _lib.REC_AIT_MAX_DIM, _lib.REC_AUC_WIDE_MAX_THRESHOLDS) == (8, 256, 1 << 24)
