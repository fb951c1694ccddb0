"""Host checks of the NCF entry points (csrc/ncf_ops.hip): they return before any launch, so they are called here without a
GPU, with dummy non-null pointer values that nothing may dereference.  Every refusal is -1 with the entry named in
rec_last_error(); batch == 0 returns REC_OK after the checks of the sizes."""
import ctypes as C

NEW = ["rec_ncf_dense_numel", "rec_ncf_fused_eligible", "rec_ncf_gather_bwd", "rec_ncf_gather_fwd", "rec_ncf_score", "rec_ncf_step"]
MB = 1 << 20
SHIPPED, BIG, SMALL = (8, [64, 32, 16, 8]), (8, [512, 256, 128, 64]), (3, [8, 6, 5, 2])
MODES = (SHIPPED, (8, []), (0, [64, 32, 16, 8]), SMALL, (2, []), (0, [8, 6, 5, 2]))


def _p(v):
    return None if v is None else C.c_void_p(v)


def _desc(net, users=6040, items=3706):
    from paddlerec_amd import ops
    return ops.ncf_desc(users, items, net[0], net[1])


def _ptrs(names, kw, base=1):
    return {n: kw.pop(n, MB * (i + base)) for i, n in enumerate(names)}


def _refused(L, fn, cases, name, **fixed):
    for kw in cases:
        assert fn(L, **fixed, **kw) == -1, kw
        assert name in L.rec_last_error(), (kw, L.rec_last_error())


def _cu(net):
    return net[0] + (net[1][0] // 2 if net[1] else 0)


def _step(L, net=SHIPPED, desc=True, B=5, mean_over=0, ldu=None, ldi=None, ldgu=None, ldgi=None, **kw):
    v = _ptrs(("users", "items", "labels", "user_table", "item_table", "dense", "pred", "g_user", "g_item", "partials", "g_dense",
               "loss"), kw)
    assert not kw, kw
    cu = _cu(net)
    ld = lambda x: cu if x is None else x
    d = _desc(net) if desc is True else desc
    return L.rec_ncf_step(*d.args(), B, mean_over, _p(v["users"]), _p(v["items"]), _p(v["labels"]),
                          _p(v["user_table"]), ld(ldu), _p(v["item_table"]), ld(ldi), _p(v["dense"]), _p(v["pred"]),
                          _p(v["g_user"]), ld(ldgu), _p(v["g_item"]), ld(ldgi), _p(v["partials"]), _p(v["g_dense"]), _p(v["loss"]),
                          None, None)


def _score(L, net=SHIPPED, desc=True, B=5, ldu=None, ldi=None, **kw):
    v = _ptrs(("users", "items", "user_table", "item_table", "dense", "pred"), kw)
    assert not kw, kw
    cu = _cu(net)
    ld = lambda x: cu if x is None else x
    d = _desc(net) if desc is True else desc
    return L.rec_ncf_score(*d.args(), B, _p(v["users"]), _p(v["items"]), _p(v["user_table"]), ld(ldu),
                           _p(v["item_table"]), ld(ldi), _p(v["dense"]), _p(v["pred"]), None, None)


def _gather_fwd(L, net=SHIPPED, desc=True, B=5, ldu=None, ldi=None, ldp=None, ldm=None, **kw):
    v = _ptrs(("users", "items", "user_table", "item_table", "pred_in", "mlp_in"), kw)
    assert not kw, kw
    cu, w0 = _cu(net), (net[1][0] if net[1] else 0)
    ld = lambda x, d: d if x is None else x
    d = _desc(net) if desc is True else desc
    return L.rec_ncf_gather_fwd(*d.args(), B, _p(v["users"]), _p(v["items"]), _p(v["user_table"]),
                                ld(ldu, cu), _p(v["item_table"]), ld(ldi, cu), _p(v["pred_in"]), ld(ldp, net[0] + 8),
                                _p(v["mlp_in"]), ld(ldm, w0), None, None)


def _gather_bwd(L, net=SHIPPED, desc=True, B=5, ldu=None, ldi=None, ldp=None, ldm=None, ldgu=None, ldgi=None, **kw):
    v = _ptrs(("users", "items", "user_table", "item_table", "d_pred_in", "d_mlp_in", "g_user", "g_item"), kw)
    assert not kw, kw
    cu, w0 = _cu(net), (net[1][0] if net[1] else 0)
    ld = lambda x, d: d if x is None else x
    d = _desc(net) if desc is True else desc
    return L.rec_ncf_gather_bwd(*d.args(), B, _p(v["users"]), _p(v["items"]), _p(v["user_table"]),
                                ld(ldu, cu), _p(v["item_table"]), ld(ldi, cu), _p(v["d_pred_in"]), ld(ldp, net[0] + 8),
                                _p(v["d_mlp_in"]), ld(ldm, w0), _p(v["g_user"]), ld(ldgu, cu), _p(v["g_item"]), ld(ldgi, cu), None)


def _bad_descs():
    from paddlerec_amd import ops
    out = []
    for change in (dict(mf_dim=-1), dict(n_fc=-1), dict(num_users=0), dict(num_items=0), dict(mf_dim=0, n_fc=0)):
        d = ops.ncf_desc(6040, 3706, 8, [64, 32, 16, 8])
        for k, v in change.items():
            setattr(d, k, v)
        out.append(d)
    odd = ops.ncf_desc(6040, 3706, 8, [63, 32, 16, 8])
    null = ops.ncf_desc(6040, 3706, 8, [64, 32, 16, 8])
    null.args = lambda: (8, 3, None, 6040, 3706)                            # a tower without its widths
    return out + [odd, null]


def test_step_refusals_without_gpu(engine_lib):
    L = engine_lib
    cases = [dict(B=-1), dict(B=1 << 31), dict(mean_over=-1), dict(ldu=39), dict(ldi=39), dict(ldgu=39), dict(ldgi=39),
             dict(net=BIG), dict(users=None), dict(items=None), dict(labels=None), dict(user_table=None), dict(item_table=None),
             dict(dense=None), dict(pred=None), dict(g_user=None), dict(g_item=None), dict(partials=None), dict(g_dense=None),
             dict(loss=None), dict(pred=4 * MB), dict(g_user=5 * MB), dict(g_item=6 * MB), dict(partials=4 * MB), dict(g_dense=6 * MB)]
    _refused(L, _step, cases + [dict(desc=d) for d in _bad_descs()], b"rec_ncf_step")
    _refused(L, _step, [dict(desc=_ncf_zero_widths())], b"rec_ncf_step")
    for net in MODES:
        assert _step(L, net=net, B=0) == 0, (net, L.rec_last_error())
        assert _step(L, net=net, B=0, ldu=64, ldi=48, ldgu=44, ldgi=52, mean_over=600) == 0
    assert _step(L, B=0, users=None, items=None, labels=None, user_table=None, item_table=None, dense=None, pred=None, g_user=None,
                 g_item=None, partials=None) == 0
    # the sizes, the desc and the two fold outputs are checked before batch == 0 returns
    assert _step(L, B=0, net=BIG) == -1 and _step(L, B=0, ldgu=39) == -1 and _step(L, B=0, loss=None) == -1
    assert _step(L, net=BIG) == -1 and b"not eligible" in L.rec_last_error()


def _ncf_zero_widths():
    from paddlerec_amd import ops
    d = ops.ncf_desc(6040, 3706, 8, [64, 32, 16, 8])
    d.widths[2] = 0
    return d


def test_score_refusals_without_gpu(engine_lib):
    L = engine_lib
    cases = [dict(B=-1), dict(B=1 << 31), dict(ldu=39), dict(ldi=39), dict(net=BIG), dict(users=None), dict(items=None),
             dict(user_table=None), dict(item_table=None), dict(dense=None), dict(pred=None), dict(pred=3 * MB), dict(pred=4 * MB),
             dict(pred=5 * MB)]
    _refused(L, _score, cases + [dict(desc=d) for d in _bad_descs()] + [dict(desc=_ncf_zero_widths())], b"rec_ncf_score")
    for net in MODES:
        assert _score(L, net=net, B=0) == 0, (net, L.rec_last_error())
    assert _score(L, B=0, users=None, items=None, user_table=None, item_table=None, dense=None, pred=None) == 0
    assert _score(L, B=0, net=BIG) == -1 and _score(L, B=0, ldu=39) == -1


def test_gather_refusals_without_gpu(engine_lib):
    L = engine_lib
    common = [dict(B=-1), dict(B=1 << 31), dict(ldu=39), dict(ldi=39), dict(ldp=7), dict(ldm=63), dict(users=None),
              dict(items=None), dict(user_table=None), dict(item_table=None)] + [dict(desc=d) for d in _bad_descs()]
    _refused(L, _gather_fwd, common + [dict(pred_in=None), dict(mlp_in=None), dict(pred_in=3 * MB), dict(mlp_in=4 * MB)],
             b"rec_ncf_gather_fwd")
    _refused(L, _gather_bwd, common + [dict(ldgu=39), dict(ldgi=39), dict(d_pred_in=None), dict(d_mlp_in=None), dict(g_user=None),
                                       dict(g_item=None), dict(g_user=8 * MB), dict(g_user=3 * MB), dict(g_item=5 * MB),
                                       dict(g_item=6 * MB)], b"rec_ncf_gather_bwd")
    for fn in (_gather_fwd, _gather_bwd):
        for net in MODES + (BIG, (8, [512, 256, 128, 64, 32, 16, 8])):        # any tower: the general route's glue
            assert fn(L, net=net, B=0) == 0, (net, L.rec_last_error())
        assert fn(L, B=0, users=None, items=None, user_table=None, item_table=None) == 0
        assert fn(L, B=0, ldu=39) == -1
    # the input a mode does not have may be null
    assert _gather_fwd(L, net=(8, []), B=0, mlp_in=None) == 0 and _gather_fwd(L, net=(0, [8, 4]), B=0, pred_in=None) == 0
    assert _gather_bwd(L, net=(8, []), B=0, d_mlp_in=None) == 0 and _gather_bwd(L, net=(0, [8, 4]), B=0, d_pred_in=None) == 0


def test_queries_without_gpu(engine_lib):
    L = engine_lib
    ok, n = C.c_int32(-1), C.c_int64(-1)
    for net, want in ((SHIPPED, 1), ((8, []), 1), ((0, [64, 32, 16, 8]), 1), (BIG, 0), (SMALL, 1)):
        assert L.rec_ncf_fused_eligible(*_desc(net).args(), C.byref(ok)) == 0 and ok.value == want, net
    assert L.rec_ncf_fused_eligible(*_desc(SHIPPED).args(), None) == -1 and b"rec_ncf_fused_eligible" in L.rec_last_error()
    for d in _bad_descs():
        assert L.rec_ncf_fused_eligible(*d.args(), C.byref(ok)) == -1 and b"rec_ncf_fused_eligible" in L.rec_last_error()
        assert L.rec_ncf_dense_numel(*d.args(), C.byref(n)) == -1 and b"rec_ncf_dense_numel" in L.rec_last_error()
    assert L.rec_ncf_dense_numel(*_desc(SHIPPED).args(), C.byref(n)) == 0 and n.value == 2764
    assert L.rec_ncf_dense_numel(*_desc((8, [])).args(), C.byref(n)) == 0 and n.value == 12
    assert L.rec_ncf_dense_numel(*_desc(SMALL).args(), C.byref(n)) == 0 and n.value == 48 + 8 + 32 + 8 + 12 + 4 + 8 + 4
    assert L.rec_ncf_dense_numel(*_desc(SHIPPED).args(), None) == -1
    assert L.rec_ncf_dense_numel(*_desc((8, [16, 8, 8, 8, 8, 8])).args(), C.byref(n)) == -1


def test_the_header_lists_exactly_these_entries():
    from paddlerec_amd import _lib
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("rec_ncf_")) == NEW
    assert (_lib.REC_NCF_MAX_FC, _lib.REC_NCF_MAX_WIDTH, _lib.REC_NCF_TILE, _lib.REC_NCF_MAX_BLOCKS,
            _lib.REC_NCF_LDS_BYTES) == (4, 128, 32, 512, 65536)
    for n in NEW:                                                          # the net is the same five arguments everywhere
        assert _lib.SIGNATURES[n][1][:5] == [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64], n
    for n in ("rec_ncf_step", "rec_ncf_score", "rec_ncf_gather_fwd", "rec_ncf_gather_bwd"):
        assert _lib.SIGNATURES[n][1][-1] is C.c_void_p                     # the stream is last
