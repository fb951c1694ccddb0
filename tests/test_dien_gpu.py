"""DIEN on the GPU: the recurrent, auxiliary-loss and attention kernels of csrc/dien_ops.hip against tests/dien_ref.py,
whole train steps against the golden and the restatement, and the trainer.

Tolerance of the recurrent, aux and attention kernels and of whole steps: err = max|got - ref64| / max|ref64| per
tensor against dien_ref.py in float64; the bound is 8 x the same error of dien_ref.py evaluated in float32 on the same
inputs, floor 1e-6 (the factor 8: a different summation order compounding over T).  Both errors are printed.

Sizes: the recurrent kernels own 16 batch rows per block (B 1, 17, 33 = one row, a tile plus one, two tiles plus one);
they have no time tile; the softmax kernel walks T in strides of 256 threads and the attention backward in strides of 4
waves (T 257 = one more than either); H 8 and 12 take the general path (12 is no multiple of 16), H 128 the
registers-resident one (small B, T <= 5)."""
import os
import shutil

import numpy as np
import pytest
import torch

import dien_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
FEEDS = ("hist_item_seq", "hist_cat_seq", "target_item", "target_cat", "label", "mask", "target_item_seq",
         "target_cat_seq", "neg_hist_item_seq", "neg_hist_cat_seq")
F32 = np.float32


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def check(name, got, ref64, ref32):
    """The 8 x float32-error rule of the module docstring."""
    e, e32 = R.relerr(got, ref64), R.relerr(ref32, ref64)
    bound = max(8 * e32, 1e-6)
    print("%-28s err %.3e  float32-cpu %.3e  bound %.3e" % (name, e, e32, bound))
    assert e <= bound, (name, e, e32)
    return e


def _gru_problem(B, T, H, seed):
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(H)
    return dict(X=rng.standard_normal((B, T, H)).astype(F32), W_ih=rng.uniform(-s, s, (3 * H, H)).astype(F32),
                W_hh=rng.uniform(-s, s, (3 * H, H)).astype(F32), b_ih=rng.uniform(-s, s, 3 * H).astype(F32),
                b_hh=rng.uniform(-s, s, 3 * H).astype(F32), dH=rng.standard_normal((B, T, H)).astype(F32),
                dhT=rng.standard_normal((B, H)).astype(F32))


GRU_SIZES = [(1, 2, 8), (17, 3, 8), (33, 257, 8), (1, 3, 12), (17, 257, 12), (33, 2, 12), (1, 5, 128), (17, 2, 128),
             (33, 3, 128)]


def _saved_of(sv):
    return np.concatenate([sv[k] for k in ("r", "z", "c", "hc", "hp")], 2)


@pytest.mark.parametrize("B,T,H", GRU_SIZES)
def test_gru_seq_fwd_and_bwd(engine_lib, B, T, H):
    from paddlerec_amd import ops
    pr = _gru_problem(B, T, H, seed=B * 1000 + T * 10 + H)
    ws = ops.Workspace(DEV)
    args = [pr[k] for k in ("X", "W_ih", "W_hh", "b_ih", "b_hh")]
    H64, sv64 = R.gru_fwd(*args)
    H32, sv32 = R.gru_fwd(*args, dtype=F32)
    X, W_ih, W_hh, b_ih, b_hh = (_t(a) for a in args)
    Hout, saved = ops.gru_layer_fwd(X, W_ih, W_hh, b_ih, b_hh, ws)
    check("H_out", _n(Hout), H64, H32)
    check("saved r|z|c|hc|hp", _n(saved), _saved_of(sv64), _saved_of(sv32))
    Hinf, none = ops.gru_layer_fwd(X, W_ih, W_hh, b_ih, b_hh, ws, want_saved=False)
    assert none is None and torch.equal(Hinf, Hout)
    for tag, dH, dhT in (("dH_out", pr["dH"], None), ("dh_T", None, pr["dhT"]), ("both", pr["dH"], pr["dhT"])):
        ref = []
        for dt, sv in ((np.float64, sv64), (F32, sv32)):
            dGi, dGh = R.gru_bwd(sv, pr["W_hh"], dH, dhT, dtype=dt)
            ref.append(dict(R.gru_param_grads(pr["X"], sv, dGi, dGh, pr["W_ih"], dt), dGi=dGi, dGh=dGh))
        dGi, dGh = ops.gru_seq_bwd(saved, W_hh, None if dH is None else _t(dH), None if dhT is None else _t(dhT))
        check(tag + " dGi", _n(dGi), ref[0]["dGi"], ref[1]["dGi"])
        check(tag + " dGh", _n(dGh), ref[0]["dGh"], ref[1]["dGh"])
        g = {k: torch.full(sh, 7.0, device=DEV) for k, sh in (("weight_ih", (3 * H, H)), ("weight_hh", (3 * H, H)),
                                                               ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,)))}
        dX = ops.gru_layer_bwd(X, saved, W_ih, W_hh, ws, g["weight_ih"], g["weight_hh"], g["bias_ih"], g["bias_hh"],
                               dH_out=None if dH is None else _t(dH), dh_T=None if dhT is None else _t(dhT))
        for k in g:
            check(tag + " d" + k, _n(g[k]), ref[0][k], ref[1][k])
        check(tag + " dX", _n(dX), ref[0]["dX"], ref[1]["dX"])
    add = _t(pr["dH"])
    dX2 = ops.gru_layer_bwd(X, saved, W_ih, W_hh, ws, g["weight_ih"], g["weight_hh"], g["bias_ih"], g["bias_hh"],
                            dH_out=_t(pr["dH"]), dh_T=_t(pr["dhT"]), dX_add=add)
    np.testing.assert_allclose(_n(dX2), _n(dX) + pr["dH"], rtol=1e-5, atol=1e-6)
    # a rerun is bit-identical
    H2, saved2 = ops.gru_layer_fwd(X, W_ih, W_hh, b_ih, b_hh, ws)
    a, b = ops.gru_seq_bwd(saved2, W_hh, _t(pr["dH"]), _t(pr["dhT"]))
    assert torch.equal(H2, Hout) and torch.equal(saved2, saved) and torch.equal(a, dGi) and torch.equal(b, dGh)


def test_gru_known_answer_with_zero_recurrent_weights(engine_lib):
    """W_hh = 0: the step closes to h' = z*h + (1-z)*tanh(gi_c + r*b_hc), computed here directly."""
    from paddlerec_amd import ops
    B, T, H = 17, 3, 12
    pr = _gru_problem(B, T, H, seed=5)
    Gi = (pr["X"].reshape(-1, H).astype(np.float64) @ pr["W_ih"].T.astype(np.float64) + pr["b_ih"]).reshape(B, T, 3 * H)
    b = pr["b_hh"].astype(np.float64)
    sg = lambda x: 1 / (1 + np.exp(-x))
    h, want = np.zeros((B, H)), np.zeros((B, T, H))
    for t in range(T):
        r, z = sg(Gi[:, t, :H] + b[:H]), sg(Gi[:, t, H:2 * H] + b[H:2 * H])
        h = z * h + (1 - z) * np.tanh(Gi[:, t, 2 * H:] + r * b[2 * H:])
        want[:, t] = h
    Hout, _ = ops.gru_seq_fwd(_t(Gi.astype(F32)), torch.zeros(3 * H, H, device=DEV), _t(pr["b_hh"]))
    np.testing.assert_allclose(_n(Hout), want, rtol=1e-5, atol=1e-6)


def test_gru_register_path_equals_general_path_bitwise(engine_lib):
    """H 128: W_hh held in registers issues the MFMAs of the general path in the same order.  The switch is read once per
    process, so the general path runs in a child process."""
    import subprocess
    import sys
    from paddlerec_amd import ops
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_dien_gpu as t\nfrom paddlerec_amd import ops\n"
            "pr = t._gru_problem(17, 4, 128, 9); ws = ops.Workspace('cuda')\n"
            "H, sv = ops.gru_layer_fwd(*(t._t(pr[k]) for k in ('X', 'W_ih', 'W_hh', 'b_ih', 'b_hh')), ws)\n"
            "a, b = ops.gru_seq_bwd(sv, t._t(pr['W_hh']), t._t(pr['dH']), t._t(pr['dhT']))\n"
            "np.savez(sys.argv[1], H=t._n(H), sv=t._n(sv), a=t._n(a), b=t._n(b))\n"
            % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "general.npz")
        subprocess.run([sys.executable, "-c", code, out], check=True, timeout=300, env=dict(os.environ, REC_GRU_REGW="0"))
        gen = np.load(out)
        pr = _gru_problem(17, 4, 128, 9)
        ws = ops.Workspace(DEV)
        H, sv = ops.gru_layer_fwd(*(_t(pr[k]) for k in ("X", "W_ih", "W_hh", "b_ih", "b_hh")), ws)
        a, b = ops.gru_seq_bwd(sv, _t(pr["W_hh"]), _t(pr["dH"]), _t(pr["dhT"]))
        for k, v in (("H", H), ("sv", sv), ("a", a), ("b", b)):
            assert np.array_equal(gen[k], _n(v)), k


# ------------------------------------------------------------------------------------------------ auxiliary loss
def _aux_problem(B, T, Ei, seed, rows=30):
    rng = np.random.default_rng(seed)
    H = 2 * Ei
    Wi, Wc = rng.standard_normal((rows, Ei)).astype(F32), rng.standard_normal((rows - 3, Ei)).astype(F32)
    ni, nc = rng.integers(0, rows, (B, T)), rng.integers(0, rows - 3, (B, T))
    return dict(go=(0.5 * rng.standard_normal((B, T, H))).astype(F32), hist=rng.standard_normal((B, T, H)).astype(F32),
                Wi=Wi, Wc=Wc, ni=ni.astype(np.int64), nc=nc.astype(np.int64), dh0=rng.standard_normal((B, T, H)).astype(F32))


def _neg_rows(pr):
    return np.concatenate([R.lookup(pr["Wi"], pr["ni"]), R.lookup(pr["Wc"], pr["nc"])], 2)


def _aux_run(pr, accumulate=True):
    from paddlerec_amd import ops
    ws = ops.Workspace(DEV)
    st = ops.new_status(DEV)
    a = [_t(pr[k]) for k in ("go", "hist", "ni", "nc", "Wi", "Wc")]
    aux, _ = ops.dien_aux_fwd(*a, ws, padding_idx=0, status=st)
    d_hist = _t(pr["dh0"]).clone()
    d_go, d_neg = ops.dien_aux_bwd(*a, d_hist, accumulate=accumulate, d_aux=1.0, padding_idx=0, status=st)
    return _n(aux), _n(d_go), _n(d_hist), _n(d_neg), int(st.item())


@pytest.mark.parametrize("B,T,Ei", [(1, 2, 4), (17, 3, 6), (5, 257, 4), (3, 5, 64)])
def test_aux_loss_fwd_and_bwd(engine_lib, B, T, Ei):
    pr = _aux_problem(B, T, Ei, seed=B + T + Ei)
    pr["go"][0, 0, :] = 3.0                                     # one n far beyond +15: no gradient through the clip
    pr["ni"][0, 1], pr["nc"][0, 1] = 7, 8
    pr["Wi"][7], pr["Wc"][8] = 2.0, 2.0
    neg = _neg_rows(pr)
    assert (pr["go"][0, 0] * neg[0, 1]).sum() > 15
    aux, d_go, d_hist, d_neg, flag = _aux_run(pr)
    ref = [(R.aux_fwd(pr["go"], pr["hist"], neg, dt)[0], R.aux_bwd(pr["go"], pr["hist"], neg, 1.0, dt))
           for dt in (np.float64, F32)]
    assert flag == 0
    check("aux", aux, ref[0][0], ref[1][0])
    check("d_gru_out", d_go, ref[0][1][0], ref[1][1][0])
    check("d_hist (accumulated)", d_hist, ref[0][1][1] + pr["dh0"], (ref[1][1][1] + pr["dh0"]).astype(F32))
    check("d_neg", d_neg, ref[0][1][2], ref[1][1][2])
    assert not d_neg[0, 1].any()                               # |n| > 15
    assert not d_go[:, T - 1].any() and not d_neg[:, 0].any()  # exactly 0
    np.testing.assert_array_equal(d_hist[:, 0], pr["dh0"][:, 0])
    _, _, written, _, _ = _aux_run(pr, accumulate=False)
    check("d_hist (written)", written, ref[0][1][1], ref[1][1][1])
    assert not written[:, 0].any()
    again = _aux_run(pr)
    assert all(np.array_equal(x, y) for x, y in zip(again[:4], (aux, d_go, d_hist, d_neg)))


def test_aux_padded_ids_and_out_of_range_ids(engine_lib):
    B, T, Ei = 2, 4, 4
    pr = _aux_problem(B, T, Ei, seed=3)
    pr["ni"][0], pr["nc"][0], pr["hist"][0] = 0, 0, 0.0         # sample 0: padded negatives, zero history rows
    pr["go"], pr["ni"], pr["nc"], pr["hist"], pr["dh0"] = (pr[k][:1] for k in ("go", "ni", "nc", "hist", "dh0"))
    aux, d_go, d_hist, d_neg, flag = _aux_run(pr)
    np.testing.assert_allclose(aux[0], (T - 1) * 2 * np.log(1e-8 + 0.5), rtol=1e-6)
    assert flag == 0 and not d_go.any()
    # ... and no gradient: d_neg is the gradient of the gathered rows; the padding id's share is dropped where the rows
    # are merged (padding_idx of rec_ids_group), so the table does not move
    from paddlerec_amd import ops
    ws, st = ops.Workspace(DEV), ops.new_status(DEV)
    for ids, W, col in ((pr["ni"], pr["Wi"], 0), (pr["nc"], pr["Wc"], Ei)):
        table, g = _t(W).clone(), _t(d_neg)
        grp = ops.IdGroups(ids.size, DEV)
        ops.ids_group(_t(ids).reshape(-1), W.shape[0], 0, ws, None, st, grp)
        ops.sparse_sgd_rows(grp, g[:, :, col:], table, 0.5, grad_group=1, grad_group_stride=2 * Ei)
        assert np.array_equal(_n(table), W) and d_neg[0, 1:, col:col + Ei].any()
    pr = _aux_problem(3, 4, Ei, seed=4)                        # an id outside the table: flagged, reads as zero
    bad = dict(pr, ni=pr["ni"].copy(), nc=pr["nc"].copy())
    bad["ni"][1, 2], bad["nc"][2, 1] = 30, -1
    aux, d_go, _, d_neg, flag = _aux_run(bad)
    from paddlerec_amd import _lib
    assert flag & _lib.REC_FLAG_INDEX_OOB
    neg = _neg_rows(pr)
    neg[1, 2, :Ei], neg[2, 1, Ei:] = 0, 0
    np.testing.assert_allclose(aux[0], R.aux_fwd(pr["go"], pr["hist"], neg)[0], rtol=1e-5)
    np.testing.assert_allclose(d_go, R.aux_bwd(pr["go"], pr["hist"], neg)[0], rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ attention sequence
def _att_problem(B, T, E, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[1] = 0                                             # masked everywhere
    mask = np.where(np.arange(T)[None, :] < lens[:, None], 0.0, -1e9).astype(F32)
    sizes = [4 * E, 80, 40, 1]
    att_w = [rng.uniform(-0.3, 0.3, (sizes[i], sizes[i + 1])).astype(F32) for i in range(3)]
    att_b = [(0.1 * rng.standard_normal(sizes[i + 1])).astype(F32) for i in range(3)]
    return dict(hist=rng.standard_normal((B, T, E)).astype(F32), q=rng.standard_normal((B, T, E)).astype(F32), mask=mask,
                att_w=att_w, att_b=att_b, dx=rng.standard_normal((B, T, E)).astype(F32),
                dh0=rng.standard_normal((B, T, E)).astype(F32), lens=lens)


@pytest.mark.parametrize("B,T,E", [(1, 2, 8), (17, 3, 12), (3, 257, 8), (2, 5, 128)])
def test_attention_seq_fwd_and_bwd(engine_lib, B, T, E):
    from paddlerec_amd import ops
    pr = _att_problem(B, T, E, seed=B + T + E)
    ws = ops.Workspace(DEV)
    hist, q, mask, dx = (_t(pr[k]) for k in ("hist", "q", "mask", "dx"))
    att_w, att_b = [_t(a) for a in pr["att_w"]], [_t(a) for a in pr["att_b"]]
    w, x_att, saved = ops.dien_attention_seq(hist, q, mask, att_w, att_b, ws)
    ref = []
    for dt in (np.float64, F32):
        w_, x_, sv_ = R.attention_fwd(pr["hist"], pr["q"], pr["mask"], pr["att_w"], pr["att_b"], dt)
        dh_, dq_, ds_ = R.attention_bwd(pr["hist"], pr["q"], w_, sv_, pr["att_w"], pr["dx"], dt)
        ref.append((w_, x_, dh_, dq_))
    check("w", _n(w), ref[0][0], ref[1][0])
    check("x_att", _n(x_att), ref[0][1], ref[1][1])
    wn, xn = _n(w), _n(x_att)
    np.testing.assert_allclose(wn.sum(1), 1.0, rtol=0, atol=2e-6 * max(1, T // 64))
    if B > 1:
        assert wn[1].max() == wn[1].min() and abs(wn[1, 0] - 1.0 / T) < 1e-6        # uniform, by plain arithmetic
    for b in range(B):
        if 0 < pr["lens"][b] < T:
            assert not xn[b, pr["lens"][b]:].any() and not wn[b, pr["lens"][b]:].any()   # exactly 0
    d_hist = _t(pr["dh0"]).clone()
    d_q = ops.dien_attention_seq_bwd(hist, q, w, saved, att_w, dx, d_hist, ws, accumulate=True)
    check("d_hist (accumulated)", _n(d_hist), ref[0][2] + pr["dh0"], (ref[1][2] + pr["dh0"]).astype(F32))
    check("d_tgt_seq", _n(d_q), ref[0][3], ref[1][3])
    d_w = torch.empty_like(d_hist)
    d_q2 = ops.dien_attention_seq_bwd(hist, q, w, saved, att_w, dx, d_w, ws, accumulate=False)
    check("d_hist (written)", _n(d_w), ref[0][2], ref[1][2])
    assert torch.equal(d_q2, d_q)


# ------------------------------------------------------------------------------------------------ whole steps
def _gold():
    g = np.load(os.path.join(GOLDEN, "dien_D8.npz"))
    p = {k[2:]: g[k] for k in g.files if k.startswith("p_")}
    att = ([g["att_w%d" % i] for i in range(3)], [g["att_b%d" % i] for i in range(3)])
    return g, p, att, [g[k] for k in FEEDS]


def _layer(p, att, Ei, items, cats):
    from paddlerec_amd.dien import DIENLayer
    m = DIENLayer(Ei, Ei, "sigmoid", False, False, items, cats, device=DEV)
    m.set_dict(p)
    m.set_attention(*att)
    return m


def _step_against_ref(m, p, att, feeds, lr):
    ref = []
    for dt in (np.float64, F32):
        fw = R.forward(p, att, feeds, dt)
        gr = R.backward(p, att, feeds, fw, dt)
        ref.append((fw, gr, R.sgd_step(p, gr, lr, dt)))
    cost, pred, aux = m.train_step(*[_t(a) for a in feeds], base_lr=lr)
    check("cost", _n(cost), ref[0][0]["cost"], ref[1][0]["cost"])
    check("aux", _n(aux), ref[0][0]["aux"], ref[1][0]["aux"])
    check("pred", _n(pred), ref[0][0]["pred"], ref[1][0]["pred"])
    for k, name in (("d_hist", "_d_hist"), ("d_q", "_d_q"), ("d_neg", "_d_neg")):
        check(k, _n(m._last[k]), ref[0][1][name], ref[1][1][name])
    for k in m._gb:
        check("grad " + k, _n(m._gb[k]), ref[0][1][k], ref[1][1][k])
    for k, v in m.state_dict().items():
        check("new " + k, _n(v), ref[0][2][k], ref[1][2][k])
    assert int(m.status.item()) == 0
    return ref


def test_train_step_matches_the_golden_and_reruns_bit_identically(engine_lib):
    g, p, att, feeds = _gold()
    lr = float(g["lr"][0])
    m = _layer(p, att, 4, 31, 29)
    logit, aux = m.forward(*[_t(a) for a in feeds])
    assert R.relerr(_n(logit), g["logit"]) < 2e-5 and R.relerr(_n(aux), g["aux"]) < 2e-5
    _step_against_ref(m, p, att, feeds, lr)
    for k, v in m.state_dict().items():                       # the golden: the reference's own float32 run (bound of
        e = R.relerr(_n(v), g["n_" + k])                       # tests/test_dien.py)
        assert e < 2e-5, (k, e)
    for n in R.TABLES:                                          # id 0 sits at valid positions: row 0 is bit-unchanged
        assert np.array_equal(_n(m.params[n + ".weight"])[0], p[n + ".weight"][0]), n
    assert all(np.array_equal(_n(a), b) for a, b in zip(m.attention_w + m.attention_b, att[0] + att[1]))
    m2 = _layer(p, att, 4, 31, 29)
    m2.train_step(*[_t(a) for a in feeds], base_lr=lr)
    for k in m.state_dict():
        assert torch.equal(m.state_dict()[k], m2.state_dict()[k]), k


def test_train_step_at_E128_B32_T8_matches_the_restatement(engine_lib):
    from paddlerec_amd.dien import DIENLayer
    Ei, B, T, items, cats = 64, 32, 8, 50, 40
    torch.manual_seed(11)
    m = DIENLayer(Ei, Ei, "sigmoid", False, False, items, cats, device=DEV)
    rng = np.random.default_rng(12)
    with torch.no_grad():
        for i in range(3):
            m.attention_b[i].copy_(_t((0.1 * rng.standard_normal(m.attention_b[i].shape)).astype(F32)))
            m.params["linear_%d.bias" % i].copy_(_t((0.1 * rng.standard_normal(m.params["linear_%d.bias" % i].shape)).astype(F32)))
        m.params["item_b_attr.weight"].copy_(_t((0.1 * rng.standard_normal((items, 1))).astype(F32)))
    p = {k: _n(v).copy() for k, v in m.state_dict().items()}
    att = ([_n(a).copy() for a in m.attention_w], [_n(a).copy() for a in m.attention_b])
    lens = rng.integers(1, T + 1, B)
    valid = np.arange(T)[None, :] < lens[:, None]
    hi = np.where(valid, rng.integers(0, items, (B, T)), 0).astype(np.int64)
    hc = np.where(valid, rng.integers(0, cats, (B, T)), 0).astype(np.int64)
    ti, tc = rng.integers(0, items, B).astype(np.int64), rng.integers(0, cats, B).astype(np.int64)
    feeds = [hi, hc, ti, tc, (rng.random(B) < 0.5).astype(F32), np.where(valid, 0.0, -1e9).astype(F32).reshape(B, T, 1),
             np.repeat(ti[:, None], T, 1), np.repeat(tc[:, None], T, 1), rng.integers(0, items, (B, T)).astype(np.int64),
             rng.integers(0, cats, (B, T)).astype(np.int64)]
    _step_against_ref(m, p, att, feeds, 0.85)


def test_out_of_range_id_sets_the_flag_and_reads_as_zero(engine_lib):
    g, p, att, feeds = _gold()
    m = _layer(p, att, 4, 31, 29)
    bad = [a.copy() for a in feeds]
    bad[8][2, 3] = 31                                          # a negative item id outside the table
    zero = [a.copy() for a in feeds]
    zero[8][2, 3] = 0                                          # ... reads as the padding id does
    logit, aux = m.forward(*[_t(a) for a in bad])
    from paddlerec_amd import _lib
    assert int(m.status.item()) & _lib.REC_FLAG_INDEX_OOB
    m2 = _layer(p, att, 4, 31, 29)
    logit0, aux0 = m2.forward(*[_t(a) for a in zero])
    assert torch.equal(aux, aux0) and torch.equal(logit, logit0) and int(m2.status.item()) == 0


def test_trainer_model_dien_train_save_load_infer(engine_lib, tmp_path, capsys, monkeypatch):
    """`python -m paddlerec_amd.trainer -m <yaml> --model dien` on the sample lines: one epoch, checkpoint, --infer."""
    import pickle
    from paddlerec_amd import trainer
    d = tmp_path / "somewhere"
    (d / "data").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "dien_sample.txt"), d / "data" / "sample_data.txt")
    monkeypatch.chdir(d)
    out = str(tmp_path / "out")
    (d / "config.yaml").write_text(
        "runner:\n  train_data_dir: data\n  test_data_dir: data\n  train_batch_size: 4\n  epochs: 1\n  print_interval: 2\n"
        "  model_save_path: %s\n  infer_batch_size: 4\n  infer_load_path: %s\n  infer_start_epoch: 0\n  infer_end_epoch: 1\n"
        "hyper_parameters:\n  optimizer:\n    class: SGD\n    learning_rate_base_lr: 0.85\n  item_emb_size: 8\n"
        "  cat_emb_size: 8\n  is_sparse: False\n  item_count: 63001\n  cat_count: 801\n  act: sigmoid\n" % (out, out))
    trainer.main(["-m", str(d / "config.yaml"), "--model", "dien"])
    path = os.path.join(out, "0", "rec.pdparams")
    assert os.path.exists(path)
    with open(path, "rb") as f:
        sd = pickle.load(f)
    want = ([n + ".weight" for n in R.TABLES] + ["item_b_attr.weight"] +
            ["linear_%d.%s" % (i, s) for i in range(3) for s in ("weight", "bias")] +
            [pat % k for pat in R.GRUS for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])
    assert sorted(sd) == sorted(want)
    assert all(np.isfinite(v).all() for v in sd.values()) and not sd["hist_item_emb_attr.weight"][0].any()
    trainer.main(["-m", str(d / "config.yaml"), "--model", "dien", "--infer"])
    printed = capsys.readouterr().out
    import re
    aucs = [float(x) for x in re.findall(r"'auc': ([0-9.eE+-]+|nan)", printed)]
    assert aucs and all(np.isfinite(a) and 0.0 <= a <= 1.0 for a in aucs), printed[-2000:]
