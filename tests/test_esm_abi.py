"""Host checks of rec_field_sumpool_fwd and rec_esm_head (csrc/esm_ops.hip): they return before any launch, so they are called
here without a GPU, with dummy non-null pointer values that nothing may dereference."""
import ctypes as C


def _pool(L, batch=4, F=3, max_len=3, D=4, stride=4, rows=10, pad=0, ld_out=0, ids=4096, W=8192, out=12288, status=16384):
    p = lambda v: None if v is None else C.c_void_p(v)
    return L.rec_field_sumpool_fwd(batch, F, max_len, D, stride, rows, pad, p(ids), p(W), p(out), ld_out, p(status), None)


def _head(L, batch=4, mode=1, ld=0, logits=4096, click=8192, buy=12288, count=16384, pred=20480, cost=24576, dl=28672):
    from paddlerec_amd._lib import EsmHeadDesc
    p = lambda v: None if v is None else C.c_void_p(v)
    d = EsmHeadDesc(batch, mode, ld, 1.0, 0.5, 0.25)
    return L.rec_esm_head(C.byref(d), p(logits), p(click), p(buy), p(count), p(pred), p(cost), p(dl), None)


def test_field_sumpool_refusals_without_gpu(engine_lib):
    L = engine_lib
    for kw, word in ((dict(max_len=0), b"max_len"), (dict(max_len=65), b"max_len"), (dict(D=0), b"emb_dim"),
                     (dict(D=1025, stride=1028), b"emb_dim"), (dict(F=0), b"sizes"), (dict(batch=-1), b"sizes"),
                     (dict(stride=3), b"row_stride"), (dict(rows=0), b"num_rows"), (dict(ld_out=11), b"below the packed width"),
                     (dict(ids=None), b"null"), (dict(W=None), b"null"), (dict(out=None), b"null")):
        assert _pool(L, **kw) == -1, kw
        assert word in L.rec_last_error(), (kw, L.rec_last_error())
    assert _pool(L, batch=0, ids=None, W=None, out=None, status=None) == 0                # nothing to do: no launch
    assert _pool(L, batch=0, ld_out=11) == -1                                            # ... but the arguments are still checked


def test_esm_head_refusals_without_gpu(engine_lib):
    L = engine_lib
    assert L.rec_esm_head(None, *[C.c_void_p(4096)] * 7, None) == -1 and b"null descriptor" in L.rec_last_error()
    for kw, word in ((dict(mode=3), b"bad mode"), (dict(mode=-1), b"bad mode"), (dict(batch=-1), b"bad batch"),
                     (dict(mode=1, ld=3), b"below the packed width"), (dict(mode=2, ld=5), b"below the packed width"),
                     (dict(mode=1, count=None), b"click_count"), (dict(logits=None), b"null"), (dict(click=None), b"null"),
                     (dict(buy=None), b"null"), (dict(pred=None), b"null"), (dict(cost=None), b"null")):
        assert _head(L, **kw) == -1, kw
        assert word in L.rec_last_error(), (kw, L.rec_last_error())
    for mode in (0, 1, 2):
        assert _head(L, batch=0, mode=mode, logits=None, click=None, buy=None, pred=None, cost=None, dl=None) == 0
    assert _head(L, batch=0, mode=0, count=None, logits=None, click=None, buy=None, pred=None, cost=None, dl=None) == 0
    assert _head(L, batch=0, mode=1, count=None) == -1                                   # IPW needs click_count at any batch


def test_the_new_exports_take_no_workspace():
    from paddlerec_amd import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("rec_esm_", "rec_field_sumpool")))
    assert names == ["rec_esm_head", "rec_field_sumpool_fwd"] and not any(n.endswith("_bytes") for n in names)
    d = _lib.EsmHeadDesc(7, _lib.REC_ESM_DR, 0, 1.0, 0.5, 0.25)
    assert C.sizeof(d) == 40 and _lib.EsmHeadDesc.ld_logit.offset == 16 and _lib.EsmHeadDesc.global_w.offset == 24
    assert (_lib.REC_ESM_ESMM, _lib.REC_ESM_IPW, _lib.REC_ESM_DR) == (0, 1, 2)
