"""The case table of the workspace-contract tests (tests/test_workspace_contract_gpu.py runs it on the GPU,
tests/test_workspace_contract.py checks on any machine that every *_bytes query of the C-ABI is named by a case).

A case is one workspace-taking entry point at the smallest shape at which one of its routes is live and its query
returns more than 0 bytes.  Importing this module needs no GPU: a case's builder touches the device only when called.

    Case(name, queries, build, bar, stale_with, zero, nondet, refusal, entry)
      entry       the exports of recengine.h whose buffer contract the case holds (tests/test_workspace_contract.py asserts
                  that every export taking (workspace, workspace_bytes) is named by one)
      queries     the *_bytes exports whose answer this case holds the entry point to
      build()     -> Built: seeded device inputs (borrowed from the family's own GPU test) and
                    new_outs()     every tensor the call may write (what the wrapper takes through out=, and buffers it
                                   updates in place), pre-filled: floats the wrapper only writes hold NaN
                    run(ws, outs)  ONE call of the paddlerec_amd.ops wrapper -> list of output tensors
                    nbytes()       what the matching query returns for this shape, asked over ctypes
                    check(outs)    the float64 reference at the family's own bar
      bar         the existing test the float64 reference and its tolerance were taken from
      stale_with  the case (of another kernel file) run in between for the stale-reuse check
      zero        how a 0-byte workspace reaches this entry point, decided from include/recengine.h (see ZERO_*)
      refusal     True: the refusal check runs.  A string: why it does not (the C-ABI gives the buffer no size argument, or
                  the entry point's refusal is already tested elsewhere — named)
      nondet      None: reruns are bit-identical and every comparison is of bits.  A string: where the header or the
                  kernel's comments say that the result depends on the order of atomics; the comparisons with the
                  baseline then use check() (the family's float64 bar) instead.
"""
import collections
import ctypes as C

import numpy as np

DEV = "cuda"

# A zero-length torch view has a null data_ptr().  recengine.h states "REC_EINVAL: null pointer" and "REC_EWORKSPACE:
# workspace too small"; an entry point given (NULL, 0) while it needs bytes answers REC_EWORKSPACE (the size is what is
# wrong).  Every case below asks for > 0 bytes, so a 0-byte view only arises in the refusal check with short = nbytes:
ZERO_NULL = "null view, size 0: refused with REC_EWORKSPACE while the query is > 0"

Case = collections.namedtuple("Case", "name queries build bar stale_with zero nondet refusal entry")
Built = collections.namedtuple("Built", "new_outs run nbytes check state")
Built.__new__.__defaults__ = (None,)       # state(outs) -> the tensors a refused call must leave as they are (default: outs)

# case name -> the entry points it calls with the buffer under test (cases added with entry= are not listed)
ENTRY = {
    "ffm_bwd": ["rec_ffm_bwd"], "fefm_fwd": ["rec_fefm_fwd"], "fefm_bwd": ["rec_fefm_bwd"], "fefm_bwd_d_fe": ["rec_fefm_bwd"],
    "fatffm_bwd": ["rec_fatffm_bwd"], "dcn_cross_fwd_l2": ["rec_dcn_cross_fwd"], "dcn_cross_bwd": ["rec_dcn_cross_bwd"],
    "ctr_head": ["rec_ctr_head_fwd_bwd"], "mlp_head_bwd": ["rec_mlp_head_bwd"], "sigmoid_logloss": ["rec_sigmoid_logloss"],
    "bce_with_logits": ["rec_bce_with_logits"], "sumsq": ["rec_sumsq"], "ids_group": ["rec_ids_group_payload"],
    "ids_group_slots": ["rec_ids_group_slots"], "prelu_bwd": ["rec_prelu_bwd"], "flen_bwd": ["rec_flen_bwd"],
    "gate_emb_bwd": ["rec_gate_emb_bwd"], "autofis_fwd": ["rec_autofis_fwd"], "autofis_bwd": ["rec_autofis_bwd"],
    "deepfm_fm_bwd": ["rec_deepfm_fm_bwd"], "deepfm_fm_bwd_sorted": ["rec_deepfm_fm_bwd_sorted"],
    "din_fwd_tile_split": ["rec_din_attention_pool_fwd_ws"], "din_fwd_tickets": ["rec_din_attention_pool_fwd_ws"],
    "din_bwd_tickets": ["rec_din_attention_pool_bwd_ws"], "dien_aux_fwd": ["rec_dien_aux_fwd"],
    "dmr_match_loss_fwd": ["rec_dmr_match_loss_fwd"], "dmr_match_loss_bwd": ["rec_dmr_match_loss_bwd"],
    "dmr_match_loss_bwd_one_chunk": ["rec_dmr_match_loss_bwd"], "batchnorm_fwd": ["rec_batchnorm_fwd"],
    "batchnorm_bwd": ["rec_batchnorm_bwd"], "batchnorm_relu_fwd": ["rec_batchnorm_relu_fwd"],
    "batchnorm_relu_bwd": ["rec_batchnorm_relu_bwd"], "shard_route": ["rec_shard_route"], "dedup_plan": ["rec_dedup_plan"],
    "gemm_splitk": ["rec_gemm_f32"], "gemm_x3": ["rec_gemm_f32"], "gemm_x3_dw": ["rec_gemm_f32"],
    "gemm_colsum_tiled": ["rec_gemm_f32"], "colsum": ["rec_colsum"], "gemm_relu_bits": ["rec_gemm_f32"],
    "gemm_b_image": ["rec_gemm_b_images"], "segment_partials": ["rec_segment_partials"],
    "crossnet_v2_layer_bwd": ["rec_crossnet_v2_layer_bwd"], "crossnet_mix_layer_bwd": ["rec_crossnet_mix_layer_bwd"],
    "deepfm_train_step": ["rec_deepfm_train_step"], "dcn_v2_train_step": ["rec_dcn_v2_train_step"],
    "din_train_step": ["rec_din_train_step"], "sparse_rows_sumsq": ["rec_sparse_rows_sumsq"],
}
# Entry points that take a caller-owned buffer of a declared size which is NOT called `workspace` (the header parse of
# tests/test_workspace_contract.py cannot see them): the partials of rec_segment_partials_bytes, their consumers that read
# BOTH partials and partials1, and the images of rec_gemm_b_image_bytes.
DECLARED_SIZE_ENTRIES = ("rec_segment_partials", "rec_sparse_adam_record", "rec_adam_record_all", "rec_gemm_b_images")

CASES = collections.OrderedDict()


def case(name, queries, bar, stale_with="ffm_bwd", zero=ZERO_NULL, nondet=None, refusal=True, entry=None):
    def deco(fn):
        assert name not in CASES
        CASES[name] = Case(name, tuple(queries), fn, bar, stale_with, zero, nondet, refusal, tuple(entry or ENTRY[name]))
        return fn
    return deco


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _query(name, *args):
    """One size_t answer of a *_bytes export."""
    from paddlerec_amd import _lib
    n = C.c_size_t(0)
    rc = getattr(_lib.lib(), name)(*args, C.byref(n))
    assert rc == 0, "%s -> %d" % (name, rc)
    return n.value


def _np(ts):
    return [None if t is None else t.detach().cpu().numpy() for t in ts]


# ------------------------------------------------------------------------------------------------ FFM / FEFM / FAT-FFM
@case("ffm_bwd", ["rec_ffm_bwd_workspace_bytes"], "tests/test_ffm_gpu.py::_check (2e-5 of scale)", stale_with="dcn_cross_bwd")
def _ffm_bwd():
    import ffm_ref
    import test_ffm_gpu as T
    from helpers import assert_close_scaled
    from paddlerec_amd import _lib, ops
    B, S, Dn, D, N = 333, 26, 13, 9, 300
    p, ids, dense, dz = T._problem(B, S, Dn, D, N, seed=B * 100 + D * 10 + S)
    R = (S + Dn) * D
    gs = (R + 3) // 4 * 4
    W, dw, idt, dt, dzt = _t(p["W"]), _t(p["dense_w"]), _t(ids), _t(dense), _t(dz)

    def run(ws, outs):
        return list(ops.ffm_bwd(idt, dt, W, dw, dzt, D, ws, out=tuple(outs), status=ops.new_status(DEV)))

    def check(outs):
        rg, ddw, ddw1 = _np(outs)
        wrg, wdw, wdw1 = ffm_ref.backward(ids, dense, p, D, dz, gs)
        assert_close_scaled(rg, wrg, 2e-5, "row_grad")
        assert not rg[:, R:].any()
        assert_close_scaled(ddw, wdw, 2e-5, "d_dense_w")
        assert_close_scaled(ddw1, wdw1, 2e-5, "d_dense_w_one")

    desc = _lib.FFMDesc(B, S, Dn, D, N, p["W"].shape[1], gs)
    return Built(lambda: [_nan(B * S, gs), _nan(Dn, R), _nan(Dn)], run,
                 lambda: _query("rec_ffm_bwd_workspace_bytes", C.byref(desc)), check)


def _fefm(which, want_d_fe=False):
    import test_deepfefm_gpu as T
    from helpers import assert_close_scaled
    from paddlerec_amd import _lib, ops
    B, S, Dn, D, N = 133, 5, 3, 9, 160
    F = S + Dn
    P = F * (F - 1) // 2
    p, ids, dense, dz, dd = T._problem(B, S, Dn, D, N, seed=S * 10 + Dn)
    W, W1, dw1, FE = _t(p["W"]), _t(p["W1"]), _t(p["dense_w_one"]), _t(p["FE"])
    idt, dt, dzt, ddt = _t(ids), _t(dense), _t(dz), _t(dd)
    cols = S * D + Dn + P
    gs = (D + 3) // 4 * 4
    want = T._reference(p, ids, dense, dz, dd, D)
    stride = p["W"].shape[1]
    if which == "fwd":
        import torch

        def new_outs():
            return [_nan(B, 1), _nan(B, 1), _nan(B, cols), torch.full((B, F), -77, dtype=torch.int64, device=DEV)]

        def run(ws, outs):
            return list(ops.fefm_fwd(idt, dt, W, W1, dw1, FE, D, ws, status=ops.new_status(DEV), out=tuple(outs))[:4])

        def check(outs):
            y1, y2, dnn_in, ids_all = _np(outs)
            assert np.array_equal(ids_all, want["ids_all"])
            for k, v in (("y1", y1), ("y2", y2), ("dnn_in", dnn_in)):
                assert_close_scaled(v, want[k], 2e-5, k)

        desc = _lib.FEFMDesc(B, S, Dn, D, N, stride, 0, cols)
        return Built(new_outs, run, lambda: _query("rec_fefm_fwd_workspace_bytes", C.byref(desc)), check)
    ids_all = _t(want["ids_all"].astype(np.int64))

    def new_outs():
        return [_nan(B * F, gs), _nan(Dn), _nan(P, D, D) if want_d_fe else None]

    def run(ws, outs):
        return list(ops.fefm_bwd(ids_all, dt, W, FE, dzt, ddt, S, D, ws, want_d_fe=want_d_fe, out=tuple(outs),
                                 status=ops.new_status(DEV)))

    def check(outs):
        rg, ddw1, dfe = _np(outs)
        assert not rg[:, D:].any() and not rg[(want["ids_all"] == 0).reshape(-1)].any()
        assert_close_scaled(rg[:, :D], want["row_grad"], 2e-5, "row_grad")
        assert_close_scaled(ddw1, want["d_dense_w_one"], 2e-5, "d_dense_w_one")
        if want_d_fe:
            assert_close_scaled(dfe, want["d_FE"], 2e-5, "d_FE")

    desc = _lib.FEFMDesc(B, S, Dn, D, N, stride, gs, dd.shape[1])
    return Built(new_outs, run, lambda: _query("rec_fefm_bwd_workspace_bytes", C.byref(desc), int(want_d_fe)), check)


_FEFM_BAR = "tests/test_deepfefm_gpu.py::_check (2e-5 of scale)"
case("fefm_fwd", ["rec_fefm_fwd_workspace_bytes"], _FEFM_BAR)(lambda: _fefm("fwd"))
case("fefm_bwd", ["rec_fefm_bwd_workspace_bytes"], _FEFM_BAR)(lambda: _fefm("bwd", False))
case("fefm_bwd_d_fe", ["rec_fefm_bwd_workspace_bytes"], _FEFM_BAR)(lambda: _fefm("bwd", True))


@case("fatffm_bwd", ["rec_fatffm_bwd_workspace_bytes"], "tests/test_fat_deepffm_gpu.py::_check (8x the float32 restatement's error)")
def _fatffm_bwd():
    import test_fat_deepffm_gpu as T
    from paddlerec_amd import _lib, ops
    S, Dn, D, B = 3, 2, 4, 1000
    q = T._problem(S, Dn, D, B, seed=S * 1000 + D * 10 + B)
    R = q["R"]
    gs = T._ru4(R)
    ids, dense, W, dw = _t(q["ids"]), _t(q["dense"]), _t(q["W"]), _t(q["dense_w"])
    a, dH, dz, dp = _t(q["a"]), _t(q["dH"]), _t(q["dz"]), _t(q["d_pooled"])

    def run(ws, outs):
        return list(ops.fatffm_bwd(ids, dense, W, dw, a, dH, dz, dp, D, ws, out=tuple(outs), status=ops.new_status(DEV))[:2])

    def check(outs):
        rg, ddw = _np(outs)
        w64, w32 = T._expect(q, np.float64), T._expect(q, np.float32)
        T._close(rg, w64["row_grad"], w32["row_grad"], T.OP_MULT, "row_grad")
        T._close(ddw, w64["d_dense_w"], w32["d_dense_w"], T.OP_MULT, "d_dense_w")
        assert not rg[:, R:].any()

    desc = _lib.FatFFMDesc(_lib.FFMDesc(B, S, Dn, D, q["W"].shape[0], q["W"].shape[1], gs), q["F2"], q["PD"])
    return Built(lambda: [_nan(B * S, gs), _nan(Dn, R)], run,
                 lambda: _query("rec_fatffm_bwd_workspace_bytes", C.byref(desc)), check)


# ------------------------------------------------------------------------------------------------ DCN cross stack
def _dcn(which):
    import dcn_ref as DR
    import test_dcn_gpu as T
    from helpers import assert_close_scaled
    from paddlerec_amd import _lib, ops
    B, d, L = 1000, 247, 3
    x0, w, b, dxl = T._problem(B, d, seed=d * 1000 + L * 10 + B % 7)
    xt, wt, bt, gt = _t(x0), _t(w), _t(b), _t(dxl)
    desc = _lib.DcnCrossDesc(B, d, L, d, d, d, d, 1.0, 0)
    nbytes = lambda: _query("rec_dcn_cross_bwd_workspace_bytes", C.byref(desc))
    if which == "fwd":
        def run(ws, outs):
            return list(ops.dcn_cross_fwd(xt, wt, bt, L, ws, out=tuple(outs)))

        def check(outs):
            xl, saved, l2 = _np(outs)
            wxl, ws_, wl2, _ = DR.cross_forward(x0, w, b, L)
            assert_close_scaled(xl, wxl, T.REL, "x_L")
            assert_close_scaled(saved, ws_, T.REL, "saved s_l")
            assert_close_scaled(l2, np.asarray([wl2]), T.REL, "l2")

        return Built(lambda: [_nan(B, d), _nan(B, L), _nan(1)], run, nbytes, check)
    saved = ops.dcn_cross_fwd(xt, wt, bt, L, ops.Workspace(DEV))[1]

    def run(ws, outs):
        return list(ops.dcn_cross_bwd(xt, wt, bt, saved, gt, ws, out=tuple(outs)))

    def check(outs):
        dx0, dw, db = _np(outs)
        wdx0, wdw, wdb = DR.cross_backward(x0, w, b, L, dxl, 1.0)
        assert_close_scaled(dx0, wdx0, T.REL, "dx0")
        assert_close_scaled(dw, wdw, T.REL, "d_w")
        assert_close_scaled(db, wdb, T.REL, "d_b")

    return Built(lambda: [_nan(B, d), _nan(d), _nan(d)], run, nbytes, check)


_DCN_BAR = "tests/test_dcn_gpu.py::_check (2e-5 of scale)"
case("dcn_cross_fwd_l2", ["rec_dcn_cross_bwd_workspace_bytes"], _DCN_BAR)(lambda: _dcn("fwd"))
case("dcn_cross_bwd", ["rec_dcn_cross_bwd_workspace_bytes"], _DCN_BAR)(lambda: _dcn("bwd"))


# ------------------------------------------------------------------------------------------------ loss heads
def _head_problem(B, n, seed):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    act = torch.relu(torch.randn(B, n, device=DEV, generator=g))
    w = torch.randn(n, 1, device=DEV, generator=g) / n ** 0.5
    b = torch.randn(1, device=DEV, generator=g) * 0.1
    y1 = torch.randn(B, 1, device=DEV, generator=g) * 0.3
    y2 = torch.randn(B, 1, device=DEV, generator=g) * 0.3
    label = (torch.rand(B, 1, device=DEV, generator=g) < 0.3).to(torch.int64)
    return act, w, b, y1, y2, label


def _close_max(x, r, tol, name):
    err, scale = float((x.double() - r).abs().max()), max(float(r.abs().max()), 1e-30)
    assert err <= tol * scale, "%s: %.3e > %.0e of %.3e" % (name, err, tol, scale)


_HEAD_BAR = "tests/test_ctr_head_gpu.py::test_ctr_head_against_float64_and_the_separate_calls"


@case("ctr_head", ["rec_ctr_head_workspace_bytes"], _HEAD_BAR)
def _ctr_head():
    import test_ctr_head_gpu as T
    from helpers import assert_close_floor
    from paddlerec_amd import ops
    B, n = 2048, 260
    act, w, b, y1, y2, label = _head_problem(B, n, B + n)

    def run(ws, outs):
        pred, dz, loss, dx, dw, db = outs
        ops.ctr_head(act, w, b, y1, y2, label, ws, dw, db, out=(pred, dz, loss, dx))
        return outs

    def check(outs):
        pred, dz, loss, dx, dw, db = outs
        p_r, dz_r, loss_r, dx_r, dw_r, db_r = T._ref(act, w, b, y1, y2, label, 1e-4, None)
        dx_r = dx_r * (act > 0)
        _close_max(pred, p_r, 2e-6, "pred"), _close_max(dz, dz_r, 1e-5, "dz"), _close_max(loss, loss_r, 2e-6, "loss")
        _close_max(dx, dx_r, 1e-5, "dx")
        _, _, _, _, dw32, db32 = T._ref(act, w, b, y1, y2, label, 1e-4, None, dtype=__import__("torch").float32)
        n64 = lambda x: x.detach().double().cpu().numpy()
        assert_close_floor(n64(dw), n64(dw_r), n64(dw32), rel=1e-5, err_msg="dw")
        assert_close_floor(n64(db).reshape(1), n64(db_r).reshape(1), n64(db32).reshape(1), rel=1e-5, err_msg="db")

    return Built(lambda: [_nan(B, 1), _nan(B, 1), _nan(1), _nan(B, n), _nan(n, 1), _nan(1)], run,
                 lambda: _query("rec_ctr_head_workspace_bytes", B, n), check)


@case("mlp_head_bwd", ["rec_mlp_head_bwd_workspace_bytes"], _HEAD_BAR)
def _mlp_head_bwd():
    import test_ctr_head_gpu as T
    from helpers import assert_close_floor
    from paddlerec_amd import ops
    import torch
    B, n = 2048, 260
    act, w, b, y1, y2, label = _head_problem(B, n, B + n)
    _, dz_r, _, dx_r, dw_r, db_r = T._ref(act, w, b, y1, y2, label, 1e-4, None)
    _, _, _, _, dw32, db32 = T._ref(act, w, b, y1, y2, label, 1e-4, None, dtype=torch.float32)
    dz = dz_r.float().contiguous()                       # the float64 head's dz, rounded once: the kernel's input

    def run(ws, outs):
        dx, dw, db = outs
        ops.mlp_head_bwd(act, dz, w, ws, dw, db, relu=True, out=dx)
        return outs

    def check(outs):
        dx, dw, db = outs
        _close_max(dx, dx_r * (act > 0), 1e-5, "dx")
        n64 = lambda x: x.detach().double().cpu().numpy()
        assert_close_floor(n64(dw), n64(dw_r), n64(dw32), rel=1e-5, err_msg="dw")
        assert_close_floor(n64(db).reshape(1), n64(db_r).reshape(1), n64(db32).reshape(1), rel=1e-5, err_msg="db")

    return Built(lambda: [_nan(B, n), _nan(n, 1), _nan(1)], run,
                 lambda: _query("rec_mlp_head_bwd_workspace_bytes", B, n), check)


@case("sigmoid_logloss", ["rec_logloss_workspace_bytes"], _HEAD_BAR)
def _sigmoid_logloss():
    import torch
    from paddlerec_amd import ops
    B = 4099
    g = torch.Generator(device=DEV).manual_seed(B)
    y1, y2, y3 = (torch.randn(B, 1, device=DEV, generator=g) * 0.5 for _ in range(3))
    label = (torch.rand(B, 1, device=DEV, generator=g) < 0.3).to(torch.int64)

    def run(ws, outs):
        return list(ops.sigmoid_logloss(y1, y2, y3, label, ws, out=tuple(outs)))

    def check(outs):
        pred, dz, loss = outs
        z = (y1.double() + y2.double() + y3.double()).requires_grad_(True)
        p = torch.sigmoid(z)
        t = label.double()
        lr = (-t * torch.log(p + 1e-4) - (1 - t) * torch.log(1 - p + 1e-4)).mean()
        lr.backward()
        _close_max(pred, p.detach(), 2e-6, "pred"), _close_max(dz, z.grad, 1e-5, "dz"), _close_max(loss, lr.detach(), 2e-6, "loss")

    return Built(lambda: [_nan(B, 1), _nan(B, 1), _nan(1)], run, lambda: _query("rec_logloss_workspace_bytes", B), check)


@case("bce_with_logits", ["rec_logloss_workspace_bytes"], _HEAD_BAR)
def _bce():
    import torch
    from paddlerec_amd import ops
    B = 4099
    g = torch.Generator(device=DEV).manual_seed(B + 1)
    z0 = torch.randn(B, 1, device=DEV, generator=g)
    label = (torch.rand(B, 1, device=DEV, generator=g) < 0.3).float()

    def run(ws, outs):                                   # the wrapper allocates its outputs itself
        return list(ops.bce_with_logits(z0, label, ws))

    def check(outs):
        pred, dz, loss = outs
        z = z0.double().requires_grad_(True)
        lr = torch.nn.functional.binary_cross_entropy_with_logits(z, label.double())
        lr.backward()
        _close_max(pred, torch.sigmoid(z.detach()), 2e-6, "pred"), _close_max(dz, z.grad, 1e-5, "dz")
        _close_max(loss, lr.detach(), 2e-6, "loss")

    return Built(lambda: [], run, lambda: _query("rec_logloss_workspace_bytes", B), check)


# ------------------------------------------------------------------------------------------------ global-norm sums
@case("sumsq", ["rec_sumsq_workspace_bytes"], "tests/test_cross_layers_gpu.py::test_sumsq")
def _sumsq():
    import torch
    from paddlerec_amd import ops
    n = 2 ** 21 + 1
    x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))

    def run(ws, outs):
        return [ops.sumsq(x, outs[0], ws)]

    def check(outs):
        want = float((x.double() ** 2).sum())
        U = 2.0 ** -24                                   # every product and every add of a tree of depth ~log2 n rounds once
        assert abs(float(outs[0][0]) - want) <= 64 * U * want

    return Built(lambda: [_nan(1)], run, lambda: _query("rec_sumsq_workspace_bytes"), check)


# ------------------------------------------------------------------------------------------------ id grouping
def _group_outs(n, rank):
    import torch
    from paddlerec_amd import ops
    g = ops.IdGroups(n, DEV)
    for t in (g.sorted_pos, g.uniq_rows, g.seg_offset, g.n_uniq):
        t.fill_(-77)
    if rank:
        g.want_rank().fill_(-77)
    return g


def _group_tensors(g):
    """What the header calls bit-exact: the first n_valid sorted positions, the first U rows and U + 1 offsets, n_uniq
    and the rank; the tails behind them are not outputs."""
    import torch
    U, nv = (int(x) for x in g.n_uniq.tolist()[:2])
    out = [g.sorted_pos[:nv], g.uniq_rows[:U], g.seg_offset[:U + 1], g.n_uniq]
    return out + ([g.rank] if g.rank is not None else [])


_GROUP_BAR = "tests/test_group_slots_gpu.py::check_against_oracle (bit-exact)"


def _ids_group(mode):
    """general: ops.ids_group (rec_ids_group_payload without a payload); payload: the same with a 32-bit payload travelling
    with every lookup; plain: rec_ids_group itself over ctypes (ops has no wrapper that calls it); slots: the slot-local
    sort of rec_ids_group_slots (B >= 8192)."""
    import torch
    import test_group_slots_gpu as T
    from paddlerec_amd import _lib, ops
    slots = mode == "slots"
    B, S, R_ = (8192, 26, 1000) if slots else (333, 26, 1000)
    ids = T.make_ids(B, S, R_, seed=B + S, hot=not slots)
    idt = _t(ids)
    so = _t(np.arange(S, dtype=np.int64) * R_)
    assert ops.group_slots_eligible(B, S, R_) == bool(slots)
    pay_np = (np.arange(B * S, dtype=np.int32) * 7 + 3).astype(np.int32)
    pay = _t(pay_np)
    status = ops.new_status(DEV)

    class Outs(list):                                    # the IdGroups travels with the list of its tensors
        pass

    def new_outs():
        g = _group_outs(B * S, slots)
        o = Outs([g.sorted_pos, g.uniq_rows, g.seg_offset, g.n_uniq] + ([g.rank] if slots else []))
        o.groups = g
        return o

    def run(ws, outs):
        g = outs.groups
        if slots:
            ops.ids_group_slots(idt, R_, 0, ws, groups=g, want_rank=True)
        elif mode == "plain":
            nb = C.c_size_t(0)
            _lib.check(_lib.lib().rec_ids_group_workspace_bytes(B * S, S * R_, C.byref(nb)), "rec_ids_group_workspace_bytes")
            w = ws.get(nb.value)
            pv = lambda t: C.c_void_p(t.data_ptr())
            _lib.check(_lib.lib().rec_ids_group(B * S, S, S * R_, 0, pv(idt), pv(so), pv(g.sorted_pos), pv(g.uniq_rows),
                                                pv(g.seg_offset), pv(g.n_uniq), pv(status), pv(w),
                                                C.c_size_t(w.numel()), ops._stream()), "rec_ids_group")
        else:
            ops.ids_group(idt, S * R_, 0, ws, so, groups=g, payload=pay if mode == "payload" else None)
        r = Outs(_group_tensors(g))
        r.groups = g
        return r

    def check(outs):
        g = outs.groups
        if mode == "payload":                            # sorted_pos holds the payload of the position the oracle sorts there
            spos, uniq, offs = g.host()
            rspos, runiq, roffs = T.oracle_group(ids, R_)
            assert np.array_equal(spos, pay_np[rspos]) and np.array_equal(uniq, runiq) and np.array_equal(offs, roffs)
        else:
            T.check_against_oracle(g, ids, R_)

    if slots:
        nbytes = lambda: _query("rec_ids_group_slots_workspace_bytes", B, S, R_)
    else:
        nbytes = lambda: _query("rec_ids_group_workspace_bytes", B * S, S * R_)
    return Built(new_outs, run, nbytes, check)


case("ids_group", ["rec_ids_group_workspace_bytes"], _GROUP_BAR)(lambda: _ids_group("general"))
case("ids_group_payload", ["rec_ids_group_workspace_bytes"], _GROUP_BAR, entry=["rec_ids_group_payload"])(
    lambda: _ids_group("payload"))
case("ids_group_plain", ["rec_ids_group_workspace_bytes"], _GROUP_BAR, entry=["rec_ids_group"])(lambda: _ids_group("plain"))
case("ids_group_slots", ["rec_ids_group_slots_workspace_bytes"], _GROUP_BAR)(lambda: _ids_group("slots"))


# ------------------------------------------------------------------------------------------------ DMR
_DMR_BAR = "tests/test_dmr_gpu.py::_close"


@case("prelu_bwd", ["rec_prelu_workspace_bytes"], _DMR_BAR)
def _prelu_bwd():
    import dmr_ref as R
    import test_dmr_gpu as T
    from paddlerec_amd import ops
    m, n, period, base, num_alpha = 150, 8, 50, 0, 50
    rng = np.random.default_rng(7 * m + n)
    x = rng.standard_normal((m, n + 3)).astype(np.float32)
    x[rng.random(x.shape) < 0.15] = 0.0
    dy = rng.standard_normal((m, n)).astype(np.float32)
    alpha = rng.uniform(0.05, 0.5, num_alpha).astype(np.float32)
    xv = x[:, :n]
    tx, tdy, ta = _t(x)[:, :n], _t(dy), _t(alpha)

    def run(ws, outs):
        return list(ops.prelu_bwd(tx, tdy, ta, ws, period=period, base=base, dalpha=outs[1], out=outs[0]))

    def check(outs):
        dx64, da64 = R.prelu_bwd(xv, dy, alpha, period, base)
        dx32, da32 = R.prelu_bwd(xv, dy, alpha, period, base, dtype=np.float32)
        T._close("prelu dx", outs[0], dx64, dx32)
        T._close("prelu dalpha", outs[1], da64, da32)

    return Built(lambda: [_nan(m, n), _nan(num_alpha)], run,
                 lambda: _query("rec_prelu_workspace_bytes", m, n, 1, period), check)


# ------------------------------------------------------------------------------------------------ FLEN / GateNet / AutoFIS
@case("flen_bwd", ["rec_flen_bwd_workspace_bytes"], "tests/test_flen_gpu.py::_check (2e-5 of scale)")
def _flen_bwd():
    import flen_ref as FR
    import test_flen_gpu as T
    from helpers import assert_close_scaled
    from paddlerec_amd import ops
    B, sizes, D, N = 1000, (5, 1, 2, 3), 9, 50
    rng = np.random.default_rng(D * 1000 + B)
    gb = FR.group_begin(sizes)
    S, G = gb[-1], len(sizes)
    P = G * (G - 1) // 2
    w_np, W = T._table(N, D, rng)
    kmf = rng.uniform(-1.0, 1.0, (P, 1)).astype(np.float32)
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    dx_np = rng.standard_normal((B, S * D)).astype(np.float32)
    dh_np = rng.standard_normal((B, D)).astype(np.float32)
    idt, kt, dht, dxt = _t(ids), _t(kmf), _t(dh_np), _t(dx_np)
    fw = ops.flen_fwd(idt, W, gb, kt, ops.new_status(DEV))[2]

    def run(ws, outs):                                   # g holds d X0 on entry and the row gradient on return
        g, dk = outs
        ops.flen_bwd(idt, N, gb, kt, fw, dht, g, ws, ops.new_status(DEV), out=dk)
        return outs

    def check(outs):
        rg_got, dk_got = _np(outs)
        E, live = FR.lookup(ids, w_np)
        FW, _ = FR.flen_forward(E, gb, kmf)
        rg, dk = FR.flen_backward(FW, gb, kmf, dh_np, dx_np.reshape(B, S, D), live)
        assert_close_scaled(rg_got, rg.reshape(B, -1), T.REL, "row gradient")
        assert_close_scaled(dk_got, dk, T.REL, "d kernel_mf")

    return Built(lambda: [dxt.clone(), _nan(P)], run, lambda: _query("rec_flen_bwd_workspace_bytes", B, S, G, D), check)


@case("gate_emb_bwd", ["rec_gate_emb_bwd_workspace_bytes"], "tests/test_gatenet_gpu.py::_emb_check (its REL of scale)")
def _gate_emb_bwd():
    import test_gatenet_gpu as T
    from helpers import assert_close_scaled
    from paddlerec_amd import ops
    B, S, D, N = 1000, 26, 9, 50
    rng = np.random.default_rng(B + S + D)
    w_np, W = T._table(N, D, rng)
    gw = rng.standard_normal(S).astype(np.float32)
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    g_np = rng.standard_normal((B, S * D)).astype(np.float32)
    idt, gwt, gt = _t(ids), _t(gw), _t(g_np)

    def run(ws, outs):                                   # g holds d out on entry and d e on return
        g, dw = outs
        ops.gate_emb_bwd(idt, W, gwt, g, ws, None, ops.new_status(DEV), out=dw)
        return outs

    def check(outs):
        de_got, dw_got = _np(outs)
        _, de, dw = T._emb_want(dict(ids=ids, w=w_np, gw=gw, g=g_np))
        assert_close_scaled(de_got, de, T.REL, "d e")
        assert_close_scaled(dw_got, dw, T.REL, "d w_s")

    return Built(lambda: [gt.clone(), _nan(S)], run, lambda: _query("rec_gate_emb_bwd_workspace_bytes", B * S, S), check)


def _autofis(which):
    import torch
    import test_autofis_gpu as T
    from helpers import assert_close_scaled
    from paddlerec_amd import ops
    B, S, D, kind = 257, 7, 4, "full"
    d = T.make_draw(B, S, D, kind, seed=1000 * S + 10 * D + B)
    P = d["P"]
    want = T.restate(d)
    V, W1 = T._tables(d["v"], d["w"])
    gamma, beta, mask, idt = _t(d["gamma"]), _t(d["beta"]), _t(d["mask"]), _t(d["ids"])
    pairs = ops.AutofisPairs(d["cols"], d["rows"], S, DEV)
    if which == "fwd":
        def run(ws, outs):                               # the running statistics move in place: they are outputs too
            x0, L, rm, rv = outs
            X0, s, Lr, sm, si, _ = ops.autofis_fwd(idt, V, W1, pairs, gamma, beta, mask, rm, rv, ws, True,
                                                   status=ops.new_status(DEV), out=(x0, L))
            return [X0, Lr, rm, rv, s, sm, si]

        def check(outs):
            X0, L, rm, rv, s, sm, si = _np(outs)
            assert np.array_equal(X0, want["X0"].astype(np.float32))
            for k, v in (("L", L), ("rm", rm), ("rv", rv), ("s", s), ("mean", sm), ("invstd", si)):
                assert_close_scaled(v, want[k], T.REL, k)

        return Built(lambda: [_nan(B, S * D), _nan(B, P), _t(d["rm0"]), _t(d["rv0"])], run,
                     lambda: _query("rec_autofis_fwd_workspace_bytes", B, S, D, P), check)
    X0, _, L, sm, si, _ = ops.autofis_fwd(idt, V, W1, pairs, gamma, beta, mask, _t(d["rm0"]), _t(d["rv0"]),
                                          ops.Workspace(DEV), True)
    dz, dx = _t(d["dz"]), _t(d["dx"])

    def run(ws, outs):                                   # dX holds the DNN's gradient on entry and gets the pair term added
        dX, dm, dg, db = outs
        ops.autofis_bwd(dz, L, X0, pairs, sm, si, gamma, beta, mask, dX, ws, out=(dm, dg, db))
        return outs

    def check(outs):
        for v, k in zip(_np(outs), ("dX", "d_mask", "d_gamma", "d_beta")):
            assert_close_scaled(v, want[k], T.REL, k)

    return Built(lambda: [dx.clone(), _nan(P), _nan(P), _nan(P)], run,
                 lambda: _query("rec_autofis_bwd_workspace_bytes", B, S, D, P), check)


_AF_BAR = "tests/test_autofis_gpu.py::check_case (its REL of scale)"
case("autofis_fwd", ["rec_autofis_fwd_workspace_bytes"], _AF_BAR)(lambda: _autofis("fwd"))
case("autofis_bwd", ["rec_autofis_bwd_workspace_bytes"], _AF_BAR)(lambda: _autofis("bwd"))


# ------------------------------------------------------------------------------------------------ DeepFM FM block
def _deepfm_fm_bwd(sorted_rows):
    import test_deepfm_gpu as T
    from helpers import make_deepfm_problem
    from oracle import deepfm_ref as R
    from paddlerec_amd import ops
    B, D, S, Dn = 777, 16, 26, 13
    pr = make_deepfm_problem(B=B, D=D, N=3000, seed=B)
    _, _, feat, sum_emb = T.run_fm_fwd(ops, pr)
    rng = np.random.default_rng(B)
    dfeat = (rng.standard_normal(tuple(feat.shape)) * 1e-3).astype(np.float32)
    dz = (rng.standard_normal((B, 1)) * 1e-3).astype(np.float32)
    dense, dft, dzt = _t(pr["dense"]), _t(dfeat), _t(dz)

    def run(ws, outs):
        return list(ops.deepfm_fm_bwd(dense, feat, sum_emb, dft, dzt, dzt, S, ws, out=tuple(outs)))

    def check(outs):
        rg, ddw, ddw1 = _np(outs)
        f = feat.cpu().numpy()
        ref = R.fm_backward(pr["ids"], pr["dense"], f, dfeat, dz, dz, 0, pr["slot_offsets"])
        np.testing.assert_allclose(rg, ref["row_grad"], rtol=T.RTOL, atol=1e-9)
        ref64 = R.fm_backward(pr["ids"], pr["dense"].astype(np.float64), f.astype(np.float64), dfeat.astype(np.float64),
                              dz.astype(np.float64), dz.astype(np.float64))
        np.testing.assert_allclose(ddw, ref64["d_dense_w"][0], rtol=T.RTOL, atol=T.RTOL * np.abs(ref64["d_dense_w"]).max())
        np.testing.assert_allclose(ddw1, ref64["d_dense_w_one"], rtol=T.RTOL,
                                   atol=T.RTOL * np.abs(ref64["d_dense_w_one"]).max())

    desc = ops.make_desc(B, S, Dn, D, 1, None)
    nbytes = lambda: _query("rec_deepfm_fm_bwd_workspace_bytes", C.byref(desc))
    if not sorted_rows:
        return Built(lambda: [_nan(B * S, D), _nan(Dn, D), _nan(Dn)], run, nbytes, check)
    # rec_deepfm_fm_bwd_sorted: the same backward, the row of lookup pos written at its rank in the grouping
    groups, _ = ops.ids_group(_t(pr["ids"]), 3000, 0, ops.Workspace(DEV))
    rank = ops.ids_rank(groups)

    def run_sorted(ws, outs):
        return list(ops.deepfm_fm_bwd(dense, feat, sum_emb, dft, dzt, dzt, S, ws, out=tuple(outs), row_rank=rank))

    def check_sorted(outs):
        rk = rank.cpu().numpy()
        live = rk >= 0
        assert live.sum() == int(groups.n_uniq[1]) and (~live).any()
        unsorted = np.zeros((B * S, D), np.float32)
        unsorted[live] = outs[0].cpu().numpy()[rk[live]]
        plain = ops.deepfm_fm_bwd(dense, feat, sum_emb, dft, dzt, dzt, S, ops.Workspace(DEV))
        assert np.array_equal(unsorted[live], plain[0].cpu().numpy()[live]), "the sorted rows are not the plain call's rows"
        check([plain[0], outs[1], outs[2]])

    return Built(lambda: [_nan(B * S, D), _nan(Dn, D), _nan(Dn)], run_sorted, nbytes, check_sorted)


_FM_BAR = "tests/test_deepfm_gpu.py::test_fm_bwd_vs_oracle (RTOL)"
case("deepfm_fm_bwd", ["rec_deepfm_fm_bwd_workspace_bytes"], _FM_BAR)(lambda: _deepfm_fm_bwd(False))
case("deepfm_fm_bwd_sorted", ["rec_deepfm_fm_bwd_workspace_bytes"], _FM_BAR)(lambda: _deepfm_fm_bwd(True))


# ------------------------------------------------------------------------------------------------ DIN attention pool
def _din(which, B, Tn):
    """E 128 with the 80-40-1 attention MLP: the compile-time-shaped kernel pair, the only one that uses a workspace.
    fwd at B 32, T 152 (the reference's batch): one block per history tile + the combine launch; fwd at B 2049, T 33:
    more tiles than the split takes, the blocks draw samples from the ticket word; bwd at B 1100, T 33: the ticket word."""
    import test_din_gpu as T
    from helpers import assert_close_floor, assert_close_scaled
    from oracle import din_ref as Dn
    from paddlerec_amd import _lib, ops
    Ei = Ec = 64
    E, ni, nc = 128, 200, 41
    rng = np.random.default_rng(B * Tn)
    tabs = [rng.uniform(-0.3, 0.3, (n, d)).astype(np.float32) for n, d in ((ni, Ei), (nc, Ec), (ni, Ei), (nc, Ec))]
    hi, hc, ti, tc, mask, _ = T._din_problem(rng, B, Tn, ni, nc)
    tis, tcs = np.repeat(ti[:, None], Tn, 1), np.repeat(tc[:, None], Tn, 1)
    aw = [rng.uniform(-0.3, 0.3, sh).astype(np.float32) for sh in ((4 * E, 80), (80, 40), (40, 1))]
    ab = [rng.uniform(-0.1, 0.1, sh).astype(np.float32) for sh in ((80,), (40,), (1,))]
    dout = rng.standard_normal((B, E)).astype(np.float32)
    taw, tab, tt = [_t(w) for w in aw], [_t(b) for b in ab], [_t(t) for t in tabs]
    ids = [_t(x) for x in (hi, hc, tis, tcs)]
    tmask = _t(mask)
    h = np.concatenate([tabs[0][hi], tabs[1][hc]], 2)
    q = np.concatenate([tabs[2][tis], tabs[3][tcs]], 2)
    desc = _lib.DinDesc(B, Tn, Ei, Ec, 80, 40, ni, nc, Ei, Ec)
    if which == "fwd":
        def run(ws, outs):                               # the wrapper allocates out and the weights itself
            out, attw, status = ops.din_attention_pool(*ids, tmask, *tt, taw, tab, ws=ws)
            return [out, attw, status]

        def check(outs):
            out, attw, status = _np(outs)
            assert int(status[0]) == 0
            want, wts = Dn.attention_pool(h, q, mask.astype(np.float32), aw, ab, return_weights=True)
            np.testing.assert_allclose(out, want, rtol=1e-5, atol=2e-6)
            assert_close_scaled(attw, wts, 1e-5)
            assert np.all(attw[mask != 0] == 0.0)

        return Built(lambda: [], run, lambda: _query("rec_din_attention_pool_fwd_workspace_bytes", C.byref(desc)), check)
    saved = {}
    _, attw, _ = ops.din_attention_pool(*ids, tmask, *tt, taw, tab, saved=saved)
    assert saved["act1"] is not None
    tdout = _t(dout)

    def run(ws, outs):
        return list(ops.din_attention_pool_bwd(*ids, *tt, taw, tab, attw, tdout, saved=saved, ws=ws))

    def check(outs):
        dh, dq = _np(outs)
        f64 = lambda xs: [x.astype(np.float64) for x in xs]
        ref = Dn.attention_pool_backward(h.astype(np.float64), q.astype(np.float64), mask.astype(np.float64), f64(aw),
                                         f64(ab), dout.astype(np.float64))
        ref32 = Dn.attention_pool_backward(h, q, mask.astype(np.float32), aw, ab, dout)
        scale = max(np.abs(ref["dh"]).max(), np.abs(ref["dq"]).max())
        assert_close_floor(dh, ref["dh"], ref32["dh"], err_msg="dh", scale=scale)
        assert_close_floor(dq, ref["dq"], ref32["dq"], err_msg="dq", scale=scale)
        assert np.all(dh[mask != 0] == 0.0) and np.all(dq[mask != 0] == 0.0)

    return Built(lambda: [], run, lambda: _query("rec_din_attention_pool_bwd_workspace_bytes", C.byref(desc)), check)


_DIN_FWD_BAR = "tests/test_din_gpu.py::test_attention_pool_vs_oracle"
_DIN_BWD_BAR = "tests/test_din_gpu.py::test_attention_pool_bwd_vs_oracle"
case("din_fwd_tile_split", ["rec_din_attention_pool_fwd_workspace_bytes"], _DIN_FWD_BAR)(lambda: _din("fwd", 32, 152))
case("din_fwd_tickets", ["rec_din_attention_pool_fwd_workspace_bytes"], _DIN_FWD_BAR)(lambda: _din("fwd", 2049, 33))
case("din_bwd_tickets", ["rec_din_attention_pool_bwd_workspace_bytes"], _DIN_BWD_BAR)(lambda: _din("bwd", 1100, 33))


# ------------------------------------------------------------------------------------------------ DIEN aux loss
@case("dien_aux_fwd", ["rec_dien_aux_workspace_bytes"], "tests/test_dien_gpu.py::check (test_aux_loss_fwd_and_bwd)")
def _dien_aux():
    import dien_ref as R
    import test_dien_gpu as T
    from paddlerec_amd import ops
    B, Tn, Ei = 5, 257, 4
    pr = T._aux_problem(B, Tn, Ei, seed=B + Tn + Ei)
    a = [_t(pr[k]) for k in ("go", "hist", "ni", "nc", "Wi", "Wc")]

    def run(ws, outs):
        aux, _ = ops.dien_aux_fwd(*a, ws, padding_idx=0, status=ops.new_status(DEV), out=outs[0] if outs else None)
        return [aux]

    def check(outs):
        neg = T._neg_rows(pr)
        T.check("aux", _np(outs)[0], R.aux_fwd(pr["go"], pr["hist"], neg, np.float64)[0],
                R.aux_fwd(pr["go"], pr["hist"], neg, np.float32)[0])

    return Built(lambda: [_nan(1)], run, lambda: _query("rec_dien_aux_workspace_bytes", B, Tn), check)


# ------------------------------------------------------------------------------------------------ DMR match loss
def _match(which, B, Cn, K):
    import dmr_ref as R
    import test_dmr_gpu as T
    from paddlerec_amd import _lib, ops
    rng = np.random.default_rng(K + B + Cn)
    U = rng.standard_normal((B, K)).astype(np.float32)
    V = (rng.standard_normal((Cn, K)) * 0.7).astype(np.float32)
    bias = rng.standard_normal(Cn).astype(np.float32)
    label = rng.integers(0, Cn, B).astype(np.int64)
    label[0] = Cn - 1
    tU, tV, tb, tl = _t(U), _t(V), _t(bias), _t(label)

    def both():
        fb, bb = C.c_size_t(0), C.c_size_t(0)
        assert _lib.lib().rec_dmr_match_loss_workspace_bytes(B, Cn, K, C.byref(fb), C.byref(bb)) == 0
        return fb.value, bb.value

    if which == "fwd":
        def run(ws, outs):                               # loss and lse are allocated by the wrapper
            loss, lse, status = ops.dmr_match_loss_fwd(tU, tV, tb, tl, ws)
            return [loss, lse, status]

        def check(outs):
            l64, lse64 = R.match_loss_fwd(U, V, bias, label)
            l32, lse32 = R.match_loss_fwd(U, V, bias, label, dtype=np.float32)
            T._close("loss", outs[0], [l64], [l32])
            T._close("lse", outs[1], lse64, lse32)
            assert int(outs[2].item()) == 0

        return Built(lambda: [], run, lambda: both()[0], check)
    lse = ops.dmr_match_loss_fwd(tU, tV, tb, tl, ops.Workspace(DEV))[1]

    def run(ws, outs):
        dU = ops.dmr_match_loss_bwd(tU, tV, tb, tl, lse, 0.1, outs[0], ws, accumulate=False)
        return [outs[0], dU]

    def check(outs):
        dU64, dV64 = R.match_loss_bwd(U, V, bias, label, 0.1)
        dU32, dV32 = R.match_loss_bwd(U, V, bias, label, 0.1, dtype=np.float32)
        T._close("dV", outs[0], dV64, dV32)
        T._close("dU", outs[1], dU64, dU32)

    return Built(lambda: [_nan(Cn, K)], run, lambda: both()[1], check)


_MATCH_BAR = "tests/test_dmr_gpu.py::_close (test_match_loss_against_float64)"
case("dmr_match_loss_fwd", ["rec_dmr_match_loss_workspace_bytes"], _MATCH_BAR)(lambda: _match("fwd", 100, 1031, 36))
case("dmr_match_loss_bwd", ["rec_dmr_match_loss_workspace_bytes"], _MATCH_BAR)(lambda: _match("bwd", 100, 1031, 36))
case("dmr_match_loss_fwd_one_chunk", ["rec_dmr_match_loss_workspace_bytes"], _MATCH_BAR,
     entry=["rec_dmr_match_loss_fwd"])(lambda: _match("fwd", 17, 7, 4))
case("dmr_match_loss_bwd_one_chunk", ["rec_dmr_match_loss_workspace_bytes"], _MATCH_BAR)(lambda: _match("bwd", 17, 7, 4))


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn(which, relu_fused):
    """M 1000 x N 513: several row blocks per column, a ragged last column tile."""
    from paddlerec_amd import ops
    M, N = 1000, 513
    rng = np.random.default_rng(M + N)
    x = (rng.standard_normal((M, N)) * 2 + 3).astype(np.float32)
    if relu_fused:
        x = (x - 3).astype(np.float32)                   # BN output of both signs: the fused ReLU has something to cut
    gamma, beta = (1 + 0.3 * rng.standard_normal(N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    rm, rv = rng.standard_normal(N).astype(np.float32), (1 + rng.random(N)).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    X, tg, tb, tdy = _t(x), _t(gamma), _t(beta), _t(dy)
    x64 = x.astype(np.float64)
    mean, var = x64.mean(0), x64.var(0)
    xhat = (x64 - mean) / np.sqrt(var + 1e-5)
    y64 = xhat * gamma + beta
    nbytes = lambda: _query("rec_batchnorm_workspace_bytes", M, N)
    if which == "fwd":
        fwd = ops.batchnorm_relu_fwd if relu_fused else ops.batchnorm_fwd

        def run(ws, outs):                               # the running statistics move in place: they are outputs too
            y, trm, trv = outs
            _, sm, si = fwd(X, tg, tb, trm, trv, ws, True, out=y)
            return [y, trm, trv, sm, si]

        def check(outs):
            y, trm, trv, sm, si = _np(outs)
            np.testing.assert_allclose(y, np.maximum(y64, 0) if relu_fused else y64, rtol=2e-5, atol=2e-5)
            np.testing.assert_allclose(sm, mean, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(si, 1 / np.sqrt(var + 1e-5), rtol=2e-5)
            np.testing.assert_allclose(trm, 0.9 * rm + 0.1 * mean, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(trv, 0.9 * rv + 0.1 * var, rtol=1e-5, atol=1e-6)

        return Built(lambda: [_nan(M, N), _t(rm), _t(rv)], run, nbytes, check)
    y, sm, si = (ops.batchnorm_relu_fwd if relu_fused else ops.batchnorm_fwd)(X, tg, tb, _t(rm), _t(rv), ops.Workspace(DEV), True)

    def run(ws, outs):
        dx, dg, db = outs
        if relu_fused:
            return list(ops.batchnorm_relu_bwd(X, y, tdy, tg, sm, si, ws, dgamma=dg, dbeta=db, out=dx))
        return list(ops.batchnorm_bwd(X, tdy, tg, sm, si, ws, relu_mask=False, dgamma=dg, dbeta=db, out=dx))

    def check(outs):
        dx, dg, db = _np(outs)
        d = dy.astype(np.float64) * (y.cpu().numpy() > 0) if relu_fused else dy.astype(np.float64)   # the kernel's own mask
        wdb, wdg = d.sum(0), (d * xhat).sum(0)
        wdx = gamma / np.sqrt(var + 1e-5) * (d - wdb / M - xhat * wdg / M)
        np.testing.assert_allclose(dx, wdx, rtol=2e-5, atol=2e-5 * max(np.abs(wdx).max(), 1e-3))
        np.testing.assert_allclose(dg, wdg, rtol=2e-5, atol=1e-5 * max(np.abs(wdg).max(), 1))
        np.testing.assert_allclose(db, wdb, rtol=2e-5, atol=1e-5 * max(np.abs(wdb).max(), 1))

    return Built(lambda: [_nan(M, N), _nan(N), _nan(N)], run, nbytes, check)


_BN_BAR = "tests/test_dlrm.py::test_batchnorm_kernels_vs_numpy"
case("batchnorm_fwd", ["rec_batchnorm_workspace_bytes"], _BN_BAR)(lambda: _bn("fwd", False))
case("batchnorm_bwd", ["rec_batchnorm_workspace_bytes"], _BN_BAR)(lambda: _bn("bwd", False))
case("batchnorm_relu_fwd", ["rec_batchnorm_workspace_bytes"], _BN_BAR)(lambda: _bn("fwd", True))
case("batchnorm_relu_bwd", ["rec_batchnorm_workspace_bytes"], _BN_BAR)(lambda: _bn("bwd", True))


# ------------------------------------------------------------------------------------------------ sharding plans
@case("shard_route", ["rec_shard_route_workspace_bytes"], "tests/test_sharded.py::test_shard_route_gpu (bit-exact)")
def _shard_route():
    import torch
    from helpers import make_deepfm_problem
    from oracle import shard_ref
    from paddlerec_amd import ops
    B, N, G = 1000, 5000, 3
    pr = make_deepfm_problem(B=B, N=N, seed=B + G, pad_frac=0.03, tables=True)
    want = shard_ref.shard_route(pr["ids"], G, 0, pr["slot_offsets"])
    ids, so = _t(pr["ids"]), _t(pr["slot_offsets"])
    n, k = pr["ids"].size, len(want["send_pos"])

    class Outs(list):
        pass

    def new_outs():
        r = ops.ShardRoute(n, G, DEV)
        o = Outs([r.send_local_row, r.send_pos, r.send_sample, r.slot_of_pos, r.send_counts])
        for t in o:
            t.fill_(-77)
        o.route = r
        return o

    def run(ws, outs):                                   # the first k entries are the outputs; the tails are not written
        r = outs.route
        ops.shard_route(ids, pr["N"], 0, G, ws, so, route=r)
        return [r.send_counts, r.send_local_row[:k], r.send_pos[:k], r.send_sample[:k], r.slot_of_pos[:n]]

    def check(outs):
        got = _np(outs)
        for g, key in zip(got, ("send_counts", "send_local_row", "send_pos", "send_sample", "slot_of_pos")):
            assert np.array_equal(g, want[key]), key

    return Built(new_outs, run, lambda: _query("rec_shard_route_workspace_bytes", n, G), check)


@case("dedup_plan", ["rec_dedup_plan_workspace_bytes"],
      "tests/test_sharded.py::test_dedup_plan_device_equals_the_oracle_statement (bit-exact)")
def _dedup_plan():
    import torch
    import cpu_kernels as K
    from paddlerec_amd import ops
    B, S, N, G, cap = 300, 26, 5003, 8, 2000
    rng = np.random.default_rng(8)
    local = (N + G - 1) // G
    ids = np.minimum(rng.zipf(1.2, size=(B, S)), N - 1).astype(np.int64)
    ids[rng.random((B, S)) < 0.05] = 0
    idt = _t(ids)
    ph, _ = K.dedup_plan(torch.from_numpy(ids), N, 0, G, local, cap, None, None, K.new_status("cpu"))

    class Outs(list):
        pass

    def new_outs():
        pl = ops.DedupPlan(B * S, G, cap, DEV)
        g = pl.groups
        o = Outs([pl.send_rows, pl.slot_of_pos, pl.slot_of_uniq, pl.counts, g.sorted_pos, g.uniq_rows, g.seg_offset, g.n_uniq])
        for t in o:
            t.fill_(-77)
        o.plan = pl
        return o

    def run(ws, outs):
        pl = outs.plan
        ops.dedup_plan(idt, N, 0, G, local, cap, ws, None, ops.new_status(DEV), plan=pl)
        U = int(pl.groups.n_uniq[0])
        return [pl.send_rows, pl.slot_of_pos[: B * S], pl.counts, pl.slot_of_uniq[:U]] + _group_tensors(pl.groups)

    def check(outs):
        got = _np(outs)
        assert np.array_equal(got[0], ph.send_rows.numpy())
        assert np.array_equal(got[1], ph.slot_of_pos.numpy()[: B * S])
        assert np.array_equal(got[2], ph.counts.numpy())

    return Built(new_outs, run, lambda: _query("rec_dedup_plan_workspace_bytes", B * S, G, local), check)


# ------------------------------------------------------------------------------------------------ GEMM
_GEMM_BAR = "tests/gemm_ref.py::check (the exact-f32 accumulate's float64 bound, 4e-7 of sum |a||b|)"


def _gemm(kind):
    """splitk: 130 x 90 x 2042 in 7 K slices (tiled 80x80 + the reduce, which applies the bias);
    x3: 8192 x 400 x 64, the bf16 x 3 forward / dX kernel, op(B)'s plane image in the workspace;
    x3_dw: dW [400, 400] = X^T G over K 8192 with db = colsum(G): partial tiles and partial column sums in the workspace;
    colsum_tiled: a trans_a call below the bf16 x 3 widths with b_colsum (the memset-then-accumulate column sums)."""
    import gemm_ref
    from paddlerec_amd import ops
    rng = np.random.default_rng(len(kind))
    mk = lambda *shape: rng.uniform(-1, 1, size=shape).astype(np.float32)
    if kind == "splitk":
        M, N, K = 130, 90, 2042
        A, Bm, bias = mk(M, K), (mk(K, N) * (1.5 / np.sqrt(K))).astype(np.float32), mk(N)
        At, Bt, bt = _t(A), _t(Bm), _t(bias)
        kw = dict(epilogue="bias", bias=bt, split_k=7)
        route = ops.GemmRouteInfo("tiled", "80x80", 7, frozenset())
        d = (M, N, K, K, N, N, 0, 0, "bias", 7)
        want, bound = gemm_ref.epi_reference("bias", A, Bm, bias, None, None, None)
        outs = lambda: [_nan(M, N)]
    elif kind == "x3":
        M, N, K = 8192, 400, 64
        A, Bm, bias = mk(M, K), mk(K, N), mk(N)
        At, Bt, bt = _t(A), _t(Bm), _t(bias)
        kw = dict(epilogue="bias_relu", bias=bt)
        route = "x3"
        d = (M, N, K, K, N, N, 0, 0, "bias_relu", 0)
        want, bound = gemm_ref.epi_reference("bias_relu", A, Bm, bias, None, None, None)
        outs = lambda: [_nan(M, N)]
    else:
        rows, kin, nout = (8192, 400, 400) if kind == "x3_dw" else (2100, 130, 90)
        X, G = mk(rows, kin), mk(rows, nout)
        At, Bt = _t(X), _t(G)
        kw = dict(trans_a=True)
        route = "x3_dw" if kind == "x3_dw" else "tiled"
        d = (kin, nout, rows, kin, nout, nout, 1, 0, "none", 0)
        want = X.astype(np.float64).T @ G.astype(np.float64)
        bound = 4e-7 * (np.abs(X).astype(np.float64).T @ np.abs(G).astype(np.float64))
        cwant, cbound = G.astype(np.float64).sum(0), 4e-7 * np.abs(G).astype(np.float64).sum(0)
        outs = lambda: [_nan(kin, nout), _nan(nout)]

    def run(ws, outs_):
        if len(outs_) == 2:
            ops.gemm(At, Bt, ws, out=outs_[0], b_colsum=outs_[1], **kw)
        else:
            ops.gemm(At, Bt, ws, out=outs_[0], **kw)
        r = ops.gemm_last_route()
        assert (r.family == route) if isinstance(route, str) else (r == route), "the call took %r, the case means %r" % (r, route)
        return outs_

    def check(outs_):
        got = _np(outs_)
        gemm_ref.check(got[0], want, bound, "C")
        if len(got) == 2:
            gemm_ref.check(got[1], cwant, cbound, "b_colsum")

    def nbytes():
        from paddlerec_amd import _lib
        desc = _lib.GemmDesc(*d[:8], _lib.EPI[d[8]], d[9], 0)
        return _query("rec_gemm_f32_workspace_bytes", C.byref(desc))

    return Built(outs, run, nbytes, check)


for _k in ("splitk", "x3", "x3_dw", "colsum_tiled"):
    case("gemm_" + _k, ["rec_gemm_f32_workspace_bytes"], _GEMM_BAR)(lambda _k=_k: _gemm(_k))


@case("colsum", ["rec_colsum_workspace_bytes"], "tests/test_gemm_gpu.py (rec_colsum against float64, 4e-7 of sum |g|)")
def _colsum():
    import gemm_ref
    from paddlerec_amd import ops
    M, N = 4099, 400
    G = np.random.default_rng(M).uniform(-1, 1, size=(M, N)).astype(np.float32)
    Gt = _t(G)

    def check(outs):
        gemm_ref.check(_np(outs)[0], G.astype(np.float64).sum(0), 4e-7 * np.abs(G).astype(np.float64).sum(0), "colsum")

    return Built(lambda: [_nan(N)], lambda ws, outs: [ops.colsum(Gt, ws, out=outs[0])],
                 lambda: _query("rec_colsum_workspace_bytes", M, N), check)


# ---- caller-owned buffers of a declared size that are not `workspace`: the C-ABI gives them no size argument, so there is
# nothing to refuse; they are laid into a GuardedWorkspace all the same (exact size, poisoned, stale)
_NO_SIZE_ARG = "the entry point takes the buffer without a size argument: nothing it could refuse"


@case("gemm_relu_bits", ["rec_gemm_relu_bits_bytes"], _GEMM_BAR, refusal=_NO_SIZE_ARG)
def _relu_bits():
    """Forward BIAS_RELU writes the mask as bits into a buffer of exactly rec_gemm_relu_bits_bytes; the dX call reads it
    instead of the activation: dX must equal the call that reads aux0, bit for bit (recengine.h), and the float64 bound."""
    import torch
    import gemm_ref
    from paddlerec_amd import _lib, ops
    M, N, K = 8192, 400, 64
    rng = np.random.default_rng(17)
    mk = lambda *shape: rng.uniform(-1, 1, size=shape).astype(np.float32)
    A, W, bias, Gy = mk(M, K), mk(K, N), mk(N), mk(M, N)
    At, Wt, bt, Gt = _t(A), _t(W), _t(bias), _t(Gy)
    plain = ops.Workspace(DEV)
    desc = _lib.GemmDesc(M, N, K, K, N, N, 0, 0, _lib.EPI["bias_relu"], 0, 0)

    def nbytes():
        ok, nb = C.c_int32(0), C.c_size_t(0)
        assert _lib.lib().rec_gemm_relu_bits_bytes(C.byref(desc), C.byref(ok), C.byref(nb)) == 0 and ok.value == 1
        return nb.value

    def run(ws, outs):
        y, dx = outs
        bits = ws.get(nbytes()).view(torch.int64)
        d, x, _, need = ops._gemm_prepare(At, Wt, False, False, "bias_relu", bt, None, None, y, 0, None, None, None, 0, None)
        x.relu_bits = bits.data_ptr()
        w = plain.get(need)
        _lib.check(_lib.lib().rec_gemm_f32(C.byref(d), At.data_ptr(), Wt.data_ptr(), y.data_ptr(), C.byref(x), w.data_ptr(),
                                           C.c_size_t(w.numel()), ops._stream()), "rec_gemm_f32")
        assert ops.gemm_last_route().family == "x3"
        # dX [M, K] = relu'(y) * (Gy W^T) has N = K = 64 columns: no bit form; the mask is read back by a call of the
        # forward's own (m, n): dY [M, N] = mask(y) * (A W), the same product
        ops.gemm(At, Wt, plain, epilogue="relu_mask", aux0=None, out=dx, relu_bits=bits)
        assert ops.gemm_last_route().family == "x3"
        return [y, dx]

    def check(outs):
        y, dx = outs
        want, bound = gemm_ref.epi_reference("bias_relu", A, W, bias, None, None, None)
        gemm_ref.check(y.cpu().numpy(), want, bound, "y")
        ref = ops.gemm(At, Wt, ops.Workspace(DEV), epilogue="relu_mask", aux0=y)
        assert torch.equal(ref, dx), "the bit mask and the activation mask give different dX bits"

    return Built(lambda: [_nan(M, N), _nan(M, N)], run, nbytes, check)


@case("gemm_b_image", ["rec_gemm_b_image_bytes"], _GEMM_BAR, refusal=_NO_SIZE_ARG)
def _b_image():
    """op(B)'s bf16 x 3 image made ahead of time into a buffer of exactly rec_gemm_b_image_bytes, consumed by the GEMM:
    the same bits as the call that splits B itself."""
    import torch
    import gemm_ref
    from paddlerec_amd import _lib, ops
    M, N, K = 8192, 400, 64
    rng = np.random.default_rng(23)
    mk = lambda *shape: rng.uniform(-1, 1, size=shape).astype(np.float32)
    A, W = mk(M, K), mk(K, N)
    At, Wt = _t(A), _t(W)
    plain = ops.Workspace(DEV)

    def nbytes():
        ok, nb = C.c_int32(0), C.c_size_t(0)
        assert _lib.lib().rec_gemm_b_image_bytes(K, N, C.byref(ok), C.byref(nb)) == 0 and ok.value == 1
        return nb.value

    def run(ws, outs):
        img = ws.get(nbytes())
        item = (_lib.GemmBImage * 1)()
        item[0].B, item[0].ldb, item[0].k, item[0].n, item[0].trans_b, item[0].image = Wt.data_ptr(), N, K, N, 0, img.data_ptr()
        _lib.check(_lib.lib().rec_gemm_b_images(1, item, ops._stream()), "rec_gemm_b_images")
        ops.gemm(At, Wt, plain, out=outs[0], b_image=img)
        assert ops.gemm_last_route().family == "x3"
        return outs

    def check(outs):
        want, bound = gemm_ref.epi_reference("none", A, W, None, None, None, None)
        gemm_ref.check(outs[0].cpu().numpy(), want, bound, "C")
        assert torch.equal(ops.gemm(At, Wt, ops.Workspace(DEV)), outs[0]), "the handed-in image and the call's own differ"

    return Built(lambda: [_nan(M, N)], run, nbytes, check)


@case("segment_partials", ["rec_segment_partials_bytes"],
      "tests/test_deepfm_gpu.py::test_hot_rows_segment_partials (1e-6 of sum |g| per merged row)", refusal=_NO_SIZE_ARG)
def _segment_partials():
    """The tile partials of the hot rows in a buffer of exactly rec_segment_partials_bytes, consumed by the SGD row
    update (P = the merged gradient): every tile case of the 64-position tiles, a ragged tail."""
    import torch
    import test_deepfm_gpu as T
    from paddlerec_amd import ops
    D = 16
    rng = np.random.default_rng(D)
    ids, N = T._hot_row_ids(rng)
    n = ids.size
    grad = rng.standard_normal((n, D)).astype(np.float32)
    groups, _ = ops.ids_group(_t(ids.reshape(-1, 1)), N, 0, ops.Workspace(DEV))
    tg = _t(grad)

    def run(ws, outs):
        buf = ws.get(_query("rec_segment_partials_bytes", n, D)).view(torch.float32)
        pp = ops.segment_partials(groups, tg, D, out=buf)
        assert pp.data_ptr() == buf.data_ptr()
        outs[0].zero_()
        ops.sparse_sgd_rows(groups, tg, outs[0], -1.0, partials=pp)
        return outs

    def check(outs):
        got = _np(outs)[0]
        live = ids != 0
        ref, mag = np.zeros((N, D), np.float64), np.zeros((N, D), np.float64)
        np.add.at(ref, ids[live], grad.astype(np.float64)[live])
        np.add.at(mag, ids[live], np.abs(grad.astype(np.float64))[live])
        assert np.all(np.abs(got - ref) <= 1e-6 * mag + 1e-6) and not got[0].any()

    return Built(lambda: [_nan(N, D)], run, lambda: _query("rec_segment_partials_bytes", n, D), check)


# ------------------------------------------------------------------------------------------------ CrossNet layers
_CROSS_REFUSAL = "tests/test_cross_layers_gpu.py::test_v2_bwd_wide_gradient_strides / test_mix_bwd_wide_gradient_strides refuse them"


@case("crossnet_v2_layer_bwd", ["rec_crossnet_v2_layer_workspace_bytes"], "tests/test_cross_layers_gpu.py::close",
      refusal=_CROSS_REFUSAL)
def _cross_v2():
    import test_cross_layers_gpu as T
    from paddlerec_amd import _lib, ops
    B, d = 130, 156
    x0, xl, W, b, dxn, old = T._v2_inputs(B, d, seed=B * 10000 + d)
    tx0, txl, Wt, bt, tdxn = _t(x0), _t(xl), _t(W), _t(b), _t(dxn)
    u = _nan(B, d)
    ops.crossnet_v2_layer_fwd(tx0, txl, Wt, bt, ops.Workspace(DEV), u=u)

    def run(ws, outs):
        dxl, acc, dW, db = outs
        ops.crossnet_v2_layer_bwd(tx0, txl, Wt, u, tdxn, acc, False, False, dW, db, ws, out=dxl)
        return outs

    def check(outs):
        want = T.both(T.v2_ref, x0, xl, W, b, dxn, old)
        for got, k in zip(outs, ("dxl", "dx0_acc", "dW", "db")):
            T.close(got, want[0][k], want[1][k], "v2 " + k)

    def nbytes():
        desc, nb = _lib.CrossV2Desc(B, d, d, d, d, d), C.c_size_t(0)
        assert _lib.lib().rec_crossnet_v2_layer_workspace_bytes(C.byref(desc), None, C.byref(nb)) == 0
        return nb.value

    return Built(lambda: [_nan(B, d), _nan(B, d), _nan(d, d), _nan(d)], run, nbytes, check)


@case("crossnet_mix_layer_bwd", ["rec_crossnet_mix_layer_workspace_bytes"], "tests/test_cross_layers_gpu.py::close",
      refusal=_CROSS_REFUSAL)
def _cross_mix():
    import test_cross_layers_gpu as T
    from paddlerec_amd import _lib, ops
    B, d, r, E = 130, 39, 5, 3
    inp = T._mix_inputs(B, d, r, E, seed=B + d + r + E)
    x0, xl, Um, Vm, Cm, bias, gw, gb, dxn, old = inp
    tx0, txl, Ut, Vt, Ct, bt, gwt, gbt, tdxn = (_t(a) for a in (x0, xl, Um, Vm, Cm, bias, gw, gb, dxn))
    _, t1, t2, prob = ops.crossnet_mix_layer_fwd(tx0, txl, Ut, Vt, Ct, bt, gwt, gbt, ops.Workspace(DEV))

    def run(ws, outs):
        dxl, acc, gU, gV, gC, gbias, ggw, ggb = outs
        ops.crossnet_mix_layer_bwd(tx0, txl, Ut, Vt, Ct, bt, gwt, t1, t2, prob, tdxn, acc, False, False, gU, gV, gC, gbias,
                                   ggw, ggb, False, ws, out=dxl)
        return outs

    def check(outs):
        want = T.both(T.mix_ref, *inp)
        for got, k in zip(outs, ("dxl", "dx0_acc", "gU", "gV", "gC", "gbias", "g_gate_w", "g_gate_b")):
            T.close(got, want[0][k], want[1][k], "mix " + k)

    def nbytes():
        desc, nb = _lib.CrossMixDesc(B, d, r, E, d, d, d), C.c_size_t(0)
        assert _lib.lib().rec_crossnet_mix_layer_workspace_bytes(C.byref(desc), None, C.byref(nb)) == 0
        return nb.value

    return Built(lambda: [_nan(B, d), _nan(B, d), _nan(E, d, r), _nan(E, d, r), _nan(E, r, r), _nan(d), _nan(d, E), _nan(E)],
                 run, nbytes, check)


# ------------------------------------------------------------------------------------------------ whole-step calls
def _step_case(make, batch, step_kw, state, query):
    """One rec_*_train_step call on a freshly seeded mirror layer whose C-step workspace is the one under test.  The
    reference is the layer's own eager step from the same seed: the one-call step issues the same entry points in the same
    order, so loss, predictions, every parameter and every moment are bit-identical (the bar of the family's test)."""
    import torch

    class Outs(list):
        pass

    def new_outs():
        o = Outs()
        o.model = make()
        query(o.model)               # builds the layer's rec_*_net (and the optimizer state it points into) ahead of the call
        return o

    def run(ws, outs):
        m = outs.model
        m._ws_c = ws
        loss, pred = m.train_step_c(*batch, **step_kw)
        torch.cuda.synchronize()
        assert int(m.status.item()) == 0
        return [loss, pred] + state(m)

    def check(outs):
        ref = make()
        loss, pred = ref.train_step(*batch, **step_kw)
        torch.cuda.synchronize()
        want = [loss, pred] + state(ref)
        assert len(want) == len(outs)
        for i, (g, w) in enumerate(zip(outs, want)):
            assert torch.equal(g, w), "output %d of the one-call step differs from the mirror's eager step" % i

    return Built(new_outs, run, lambda: query(make()), check, lambda outs: state(outs.model))


@case("deepfm_train_step", ["rec_deepfm_train_step_workspace_bytes"],
      "tests/test_deepfm_step_c.py::test_c_step_equals_the_mirrors_eager_step (bit-identical)")
def _deepfm_step():
    import torch
    from paddlerec_amd import _lib
    from paddlerec_amd.deepfm import DeepFMLayer
    B, N, D, Dn, S, fc = 700, 5000, 16, 13, 26, [64, 32]        # 18200 lookups: grouping sort + partials + record update
    g = torch.Generator(device=DEV).manual_seed(11)
    ids = torch.randint(0, N, (B, S), device=DEV, generator=g)
    dense = torch.rand(B, Dn, device=DEV, generator=g)
    label = (torch.rand(B, 1, device=DEV, generator=g) < 0.3).to(torch.int64)

    def make():
        torch.manual_seed(3)
        return DeepFMLayer(N, D, Dn, S, fc, device=DEV)

    def state(m):
        return [m.fm.rec, m.dense.data, m.dense.m, m.dense.v] + ([m.sparse_state["mv"]] if m.sparse_state else [])

    def query(m):
        net = m.c_net()
        return _query("rec_deepfm_train_step_workspace_bytes", C.byref(net), B)

    return _step_case(make, (ids, dense, label), dict(lr=1e-2), state, query)


@case("dcn_v2_train_step", ["rec_dcn_v2_train_step_workspace_bytes"],
      "tests/test_dcn_v2_step_c.py::test_c_step_equals_the_mirror_bit_for_bit (bit-identical)")
def _dcn_v2_step():
    import torch
    import test_dcn_v2_step_c as T
    B = 512
    batch = tuple(T._batch(np.random.default_rng(B), B, 26, 3000))

    def make():
        torch.manual_seed(5)
        return T._model(True, True, False, [64, 32])            # stacked CrossNetMix: every workspace-taking layer call

    def state(m):
        return list(m.state_dict().values()) + [m.dense.grad, m.dense.m, m.dense.v] + \
            ([m.sparse_state["mv"]] if m.sparse_state else [])

    def query(m):
        net = m.c_net(10.0)
        return _query("rec_dcn_v2_train_step_workspace_bytes", C.byref(net), B)

    return _step_case(make, batch, dict(lr=1e-2, clip_norm=10.0), state, query)


@case("din_train_step", ["rec_din_train_step_workspace_bytes"],
      "tests/test_din_step_c.py::test_c_step_equals_the_mirror_bit_for_bit (bit-identical)")
def _din_step():
    import torch
    import test_din_step_c as T
    from paddlerec_amd.din import DINLayer
    B, Tn, ni, nc = 32, 152, 900, 60                            # din/config.yaml's batch: the tile-split attention forward
    batch = tuple(T._problem(np.random.default_rng(B + 64), B, Tn, ni, nc))

    def make():
        torch.manual_seed(7)
        return DINLayer(64, 64, "sigmoid", False, True, ni, nc, device=DEV)

    def state(m):
        return list(m.state_dict().values())

    def query(m):
        net = m.c_net()
        return _query("rec_din_train_step_workspace_bytes", C.byref(net), B, Tn)

    return _step_case(make, batch, dict(base_lr=0.5), state, query)


# ------------------------------------------------------------------------------------------------ merged-row norm
@case("sparse_rows_sumsq", ["rec_sumsq_workspace_bytes"],
      "tests/test_deepfm_gpu.py::test_hot_rows_segment_partials (rtol 1e-5 against the float64 sum)")
def _rows_sumsq():
    import torch
    import test_deepfm_gpu as T
    from paddlerec_amd import ops
    D = 16
    rng = np.random.default_rng(D + 1)
    ids, N = T._hot_row_ids(rng)
    grad = rng.standard_normal((ids.size, D)).astype(np.float32)
    groups, _ = ops.ids_group(_t(ids.reshape(-1, 1)), N, 0, ops.Workspace(DEV))
    tg = _t(grad)

    def check(outs):
        ref = np.zeros((N, D), np.float64)
        np.add.at(ref, ids[ids != 0], grad.astype(np.float64)[ids != 0])
        np.testing.assert_allclose(float(outs[0].item()), float((ref ** 2).sum()), rtol=1e-5)

    return Built(lambda: [_nan(1)], lambda ws, outs: [ops.sparse_rows_sumsq(groups, tg, D, outs[0], ws)],
                 lambda: _query("rec_sumsq_workspace_bytes"), check)


# ------------------------------------------------------------------------------------------------ Linear backward pair
def _pair(rows, kin, nout, want_pair):
    """rec_gemm_f32_pair through ops.linear_backward: dW = X^T G, db = colsum(G), dX = relu'(X) * (G W^T); workspace = the
    larger of the two GEMMs' queries.  300 x 64 x 48: launch-bound, both GEMMs in ONE launch (route flag pair);
    2100 x 130 x 90: K 2100 leaves the direct kernel, two rec_gemm_f32 calls (split-K dW first)."""
    import gemm_ref
    from paddlerec_amd import _lib, ops
    rng = np.random.default_rng(rows + kin)
    mk = lambda *shape: rng.uniform(-1, 1, size=shape).astype(np.float32)
    X, G, W = mk(rows, kin), mk(rows, nout), mk(kin, nout)
    X[::3, ::2] = 0.0                                    # the ReLU mask has something to cut
    Xt, Gt, Wt = _t(X), _t(G), _t(W)

    def run(ws, outs):
        dW, db, dX = outs
        ops.linear_backward(Xt, Gt, Wt, ws, dW, db, relu_src=Xt, out=dX)
        r = ops.gemm_last_route()
        assert ("pair" in r.flags) == want_pair, "the call took %r" % (r,)
        return outs

    def check(outs):
        dW, db, dX = _np(outs)
        f = lambda a: a.astype(np.float64)
        gemm_ref.check(dW, f(X).T @ f(G), 4e-7 * (np.abs(f(X)).T @ np.abs(f(G))), "dW")
        gemm_ref.check(db, f(G).sum(0), 4e-7 * np.abs(f(G)).sum(0), "db")
        gemm_ref.check(dX, np.where(X > 0, f(G) @ f(W).T, 0), 4e-7 * (np.abs(f(G)) @ np.abs(f(W)).T), "dX")

    def nbytes():
        d0 = _lib.GemmDesc(kin, nout, rows, kin, nout, nout, 1, 0, _lib.EPI["none"], 0, 0)
        d1 = _lib.GemmDesc(rows, kin, nout, nout, nout, kin, 0, 1, _lib.EPI["relu_mask"], 0, 0)
        return max(_query("rec_gemm_f32_workspace_bytes", C.byref(d0)), _query("rec_gemm_f32_workspace_bytes", C.byref(d1)))

    return Built(lambda: [_nan(kin, nout), _nan(nout), _nan(rows, kin)], run, nbytes, check)


case("gemm_pair_one_launch", ["rec_gemm_f32_workspace_bytes"], _GEMM_BAR, entry=["rec_gemm_f32_pair"])(
    lambda: _pair(300, 64, 48, True))
case("gemm_pair_two_calls", ["rec_gemm_f32_workspace_bytes"], _GEMM_BAR, entry=["rec_gemm_f32_pair"])(
    lambda: _pair(2100, 130, 90, False))


# ------------------------------------------------------------------------------------------------ record row updates
def _adam_record(all_rows):
    """Both partials buffers of the record update: partials (D 16, the case's guarded buffer) and partials1 (D 1, a guarded
    buffer of its own made inside the call and checked there), each of exactly rec_segment_partials_bytes, read by
    rec_sparse_adam_record / rec_adam_record_all from zero moments at step 1: the first moments are 0.1 x the merged
    gradients."""
    import torch
    import test_deepfm_gpu as T
    from helpers import GuardedWorkspace
    from paddlerec_amd import ops
    D, stride = 16, 32
    rng = np.random.default_rng(D + 2 + all_rows)
    ids, N = T._hot_row_ids(rng)
    n = ids.size
    grad, grad1 = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32)
    groups, _ = ops.ids_group(_t(ids.reshape(-1, 1)), N, 0, ops.Workspace(DEV))
    tg, tg1 = _t(grad), _t(grad1)
    rec0 = np.zeros((N, stride), np.float32)
    rec0[:, :D + 1] = rng.standard_normal((N, D + 1)) * 0.1
    update = ops.adam_record_all if all_rows else ops.sparse_adam_record

    def run(ws, outs):
        rec, mv = outs
        guarded = isinstance(ws, GuardedWorkspace)
        ws1 = GuardedWorkspace(DEV, fill=ws.fill, short=0, refill=ws.refill) if guarded else ops.Workspace(DEV)
        b16, b1 = _query("rec_segment_partials_bytes", n, D), _query("rec_segment_partials_bytes", n, 1)
        buf, buf1 = ws.get(b16).view(torch.float32), ws1.get(b1).view(torch.float32)
        pp = ops.segment_partials(groups, tg, D, out=buf)
        pp1 = ops.segment_partials(groups, tg1, 1, out=buf1)
        assert pp.data_ptr() == buf.data_ptr() and pp1.data_ptr() == buf1.data_ptr()
        update(groups, tg, tg1, 1, rec, mv, D, 1, lr=1e-3, partials=pp, partials1=pp1)
        torch.cuda.synchronize()
        if guarded and ws.refill:
            assert ws1.intact(), "partials1 was written outside its declared bytes"
        return outs

    def check(outs):
        rec, mv = _np(outs)
        live = ids != 0
        for g, got, name in ((grad, mv[:, :D], "m"), (grad1, rec[:, D + 1:D + 2], "m1")):
            ref, mag = np.zeros((N, g.shape[1]), np.float64), np.zeros((N, g.shape[1]), np.float64)
            np.add.at(ref, ids[live], g.astype(np.float64)[live])
            np.add.at(mag, ids[live], np.abs(g.astype(np.float64))[live])
            assert np.all(np.abs(got - 0.1 * ref) <= 1e-7 * mag + 1e-7), name
        assert np.array_equal(rec[0], rec0[0]) or all_rows    # the padding row of the lazy update does not move

    return Built(lambda: [_t(rec0), _t(np.zeros((N, stride), np.float32))], run,
                 lambda: _query("rec_segment_partials_bytes", n, D), check)


_REC_BAR = "tests/test_deepfm_gpu.py::test_hot_rows_segment_partials (first moment = 0.1 x merged g, 1e-7 of sum |g|)"
case("sparse_adam_record_partials", ["rec_segment_partials_bytes"], _REC_BAR, refusal=_NO_SIZE_ARG,
     entry=["rec_sparse_adam_record", "rec_segment_partials"])(lambda: _adam_record(False))
case("adam_record_all_partials", ["rec_segment_partials_bytes"], _REC_BAR, refusal=_NO_SIZE_ARG,
     entry=["rec_adam_record_all", "rec_segment_partials"])(lambda: _adam_record(True))


# ------------------------------------------------------------------------------------------------ exemptions
# *_bytes exports that no case above names, each with the reason.
EXEMPT = {
}
# workspace-taking entry points that no case names
EXEMPT_ENTRY = {
    "rec_crossnet_v2_layer_fwd": "tests/test_cross_layers_gpu.py holds it to an exact-size workspace, NaN-poisoned outputs "
                                 "and a refusal that writes nothing; the table carries the layer's backward",
    "rec_crossnet_mix_layer_fwd": "as rec_crossnet_v2_layer_fwd",
}
