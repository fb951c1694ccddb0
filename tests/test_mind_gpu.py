"""The MIND kernels (csrc/mind_ops.hip) and the layer (paddlerec_amd/mind.py) on the GPU against tests/mind_ref.py.

Tolerance, the project's rule (tests/mtl_checks.py), for every output: err = max|got - ref64| / max|ref64|, bound max(8 x
the float32 restatement's error on the same inputs, 1e-6).  Every kernel runs twice and the two results are compared bit for
bit.  Shapes: the smallest that reach each path — one lane of work (T = K = H = 1), the golden's shape, the limits
(T 64, K 8, H 128, iters 8: one wave per block, both column passes), and 67 samples of the config's width (four waves per
block, a ragged last block, the float4 staging).  The routing's inputs are scaled so that a round's logit update stays of order
one: with |low| ~ sqrt(H) the eight rounds amplify ANY float32 rounding beyond what a tolerance can state."""
import numpy as np
import pytest
import torch

import mind_checks as K
import mind_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _close(got, ref64, ref32, what):
    e, b = R.relerr(got.cpu().numpy().reshape(np.shape(ref64)), ref64), K.bound_of(ref32, ref64)
    print("%-44s err %.3g  float32-ref err %.3g" % (what, e, b / 8))
    assert e <= b, (what, e, b)


def _strided(a, pad):
    """a [rows, cols] as a view of a wider NaN-filled buffer -> (view, buffer)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _t(a)
    return buf[:, :a.shape[1]], buf


# ------------------------------------------------------------------------------------------------ routing
ROUTING = [(3, 1, 1, 1, 1, 0), (5, 6, 3, 12, 3, 0), (2, 64, 8, 128, 8, 0), (67, 20, 4, 64, 3, 0), (5, 6, 3, 12, 3, 3),
           (67, 20, 4, 64, 3, 4), (6, 7, 2, 65, 2, 0)]


@pytest.mark.parametrize("B,T,Kc,H,iters,pad", ROUTING)
def test_routing_fwd_bwd(engine_lib, B, T, Kc, H, iters, pad):
    """seq_len cycles through 0 (all padded: the inner softmax is uniform over T), 1, T and T + 3 (none padded), then random;
    the padded positions of low hold garbage of magnitude 3 — the final softmax gives them 1 / K, so it IS part of Z.
    pad: a row stride wider than H (3: the scalar staging, 4: float4), NaN behind every row.  (6, 7, 2, 65, 2): an odd H above
    one column pass."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(B * 1000 + T * 10 + H)
    seq = np.array(([0, 1, T, T + 3] * B)[:B], np.int64)
    if B > 4:
        seq[4:] = rng.integers(1, T + 1, B - 4)
    low = (rng.standard_normal((B, T, H)) / np.sqrt(H)).astype(np.float32)
    padded = np.arange(T)[None, :] >= seq[:, None]
    low[padded] = (3.0 * rng.standard_normal((int(padded.sum()), H))).astype(np.float32)
    logits = rng.standard_normal((Kc, T)).astype(np.float32)
    g = rng.standard_normal((B, Kc, H)).astype(np.float32)
    x, buf = _strided(low.reshape(B * T, H), pad)
    outs = [ops.mind_routing_fwd(x, _t(seq), _t(logits), iters) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    W, Z, caps = outs[0]
    r64, r32 = (R.routing_fwd(low, seq, logits, iters, dt) for dt in (np.float64, np.float32))
    for name, got, a, b in zip(("W", "Z", "caps"), (W, Z, caps), r64, r32):
        _close(got, a, b, "routing %s %s" % (name, (B, T, Kc, H, iters, pad)))
    Wn = W.cpu().numpy()
    full = np.broadcast_to(padded[:, None, :], Wn.shape)
    assert np.array_equal(Wn[full], np.full(int(full.sum()), np.float32(1.0) / np.float32(Kc)))       # exactly 1 / K, not 0
    assert np.allclose(Wn.sum(1), 1.0, atol=1e-6)
    # backward from the reference's own Z and W, so that its error is the backward's alone
    Z64, W64 = r64[1].astype(np.float32), r64[0].astype(np.float32)
    dl = []
    for _ in range(2):
        dbuf = torch.full((B * T, H + pad), NAN, dtype=torch.float32, device=DEV)
        dl.append(ops.mind_routing_bwd(_t(g), _t(Z64), _t(W64), out=dbuf[:, :H]).clone())
        assert pad == 0 or bool(torch.isnan(dbuf[:, H:]).all())
    assert torch.equal(dl[0], dl[1])
    d64, d32 = (R.routing_bwd(g, Z64, W64, dt).reshape(B * T, H) for dt in (np.float64, np.float32))
    _close(dl[0], d64, d32, "routing d_low %s" % ((B, T, Kc, H, iters, pad),))
    assert pad == 0 or bool(torch.isnan(buf[:, H:]).all())


def test_routing_squash_gradient_against_finite_differences():
    """mind_ref.routing_bwd itself (what the kernel is held to) against central differences of sum(g * squash(W low))."""
    rng = np.random.default_rng(5)
    B, T, Kc, H = 2, 4, 3, 5
    low, W = rng.standard_normal((B, T, H)), rng.random((B, Kc, T))
    g = rng.standard_normal((B, Kc, H))
    f = lambda x: float((g * R.squash(R.bmm(W, x))[0]).sum())
    want = np.zeros_like(low)
    for i in np.ndindex(*low.shape):
        d = np.zeros_like(low)
        d[i] = 1e-6
        want[i] = (f(low + d) - f(low - d)) / 2e-6
    assert R.relerr(R.routing_bwd(g, R.bmm(W, low), W), want) < 1e-7


# ------------------------------------------------------------------------------------------------ label-aware attention
@pytest.mark.parametrize("pow_p", [1.0, 2.0])
@pytest.mark.parametrize("B,Kc,H,pad", [(3, 1, 12, 0), (5, 8, 12, 0), (67, 4, 64, 0), (67, 4, 64, 4), (5, 8, 13, 3), (3, 8, 128, 0),
                                        (2, 3, 1, 0)])
def test_label_attention_fwd_bwd(engine_lib, B, Kc, H, pad, pow_p):
    """K 1 (the softmax is one and d(score) exactly 0) and K 8; H 12 / 64 / 128 the float4 form on 4 / 16 / 32 lanes, H 13 and
    1 the scalar form; pow_p 2 squares negative scores as torch.pow does.  caps2 is non-negative (it follows a ReLU)."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(B * 100 + Kc * 10 + H)
    caps2 = np.maximum(rng.standard_normal((B, Kc, H)), 0).astype(np.float32)
    target = (rng.standard_normal((B, H)) / np.sqrt(H)).astype(np.float32)
    g = rng.standard_normal((B, H)).astype(np.float32)
    x, _ = _strided(caps2.reshape(B * Kc, H), pad)
    q, _ = _strided(target, pad)
    gv, _ = _strided(g, pad)
    outs = [ops.mind_label_attn_fwd(x, q, Kc, pow_p) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    user, attn = outs[0]
    r64, r32 = (R.label_attn_fwd(caps2, target, pow_p, dt) for dt in (np.float64, np.float32))
    _close(user, r64[0], r32[0], "label attention user")
    _close(attn, r64[1], r32[1], "label attention attn")
    a64 = r64[1].astype(np.float32)
    outs = [ops.mind_label_attn_bwd(x, q, _t(a64), gv, pow_p) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    b64, b32 = (R.label_attn_bwd(caps2, target, a64, g, pow_p, dt) for dt in (np.float64, np.float32))
    _close(outs[0][0], b64[0].reshape(B * Kc, H), b32[0].reshape(B * Kc, H), "label attention d_caps2")
    _close(outs[0][1], b64[1], b32[1], "label attention d_target")
    if Kc == 1:
        assert np.array_equal(attn.cpu().numpy(), np.ones((B, 1), np.float32))
        assert not outs[0][1].any()                                              # d(target) = d(score) * caps2 = 0 exactly


# ------------------------------------------------------------------------------------------------ sampled-softmax head
@pytest.mark.parametrize("B,H,n,pad", [(3, 12, 1, 0), (7, 12, 6, 0), (7, 12, 6, 3), (5, 64, 130, 0), (67, 64, 130, 2),
                                       (3, 64, 1024, 0), (3, 1, 6, 0)])
def test_ssm_head(engine_lib, B, H, n, pad):
    """n 1 / 6 / 130 / 1024: below a wave, three passes of a wave, sixteen.  Sample 0's label is hit by negative 0 — with n 1
    every sample column of that row is hit — the last sample's label is in no negative, and sample 1 (where there is one) has
    sample logits spread over more than 80 around a true logit of -40: without the maximum subtracted exp overflows."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(B * 100 + H * 10 + n)
    N = 4 * n + 50
    neg = rng.permutation(np.arange(1, N))[:n].astype(np.int64)
    rest = np.setdiff1d(np.arange(1, N), neg)
    labels = rng.choice(rest, B).astype(np.int64)
    labels[0] = neg[0]
    user = rng.standard_normal((B, H)).astype(np.float32)
    true_w = rng.standard_normal((B, H)).astype(np.float32)
    S = rng.standard_normal((B, n)).astype(np.float32)
    if B > 1:
        S[1] = np.linspace(-60.0, 100.0, n, dtype=np.float32) if n > 1 else np.float32(100.0)
        true_w[1] = -40.0 * user[1] / (user[1] ** 2).sum()
    true_b, sample_b = rng.standard_normal(B).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    lq = np.log(rng.random(N) * 0.9 + 0.01).astype(np.float32)
    u, _ = _strided(user, pad)
    tw, _ = _strided(true_w, pad)
    args = (_t(true_b),), (_t(sample_b), _t(labels), _t(neg), _t(lq[labels]), _t(lq[neg]), 1.0 / B)
    outs = []
    for _ in range(2):
        s, sbuf = _strided(S, pad)
        dtw, dtw_buf = _strided(np.zeros((B, H), np.float32), pad)
        du0, du0_buf = _strided(np.zeros((B, H), np.float32), pad)
        loss, d_true, dS = ops.mind_ssm_head(u, tw, *args[0], s, *args[1], d_true_w=dtw, d_user0=du0)
        assert dS.data_ptr() == s.data_ptr()
        assert pad == 0 or all(bool(torch.isnan(x[:, w:]).all()) for x, w in ((sbuf, n), (dtw_buf, H), (du0_buf, H)))
        outs.append((loss.clone(), d_true.clone(), dS.clone(), dtw.clone(), du0.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    r64, r32 = (R.ssm_head(user, true_w, true_b, S, sample_b, labels, neg, lq[labels], lq[neg], 1.0 / B, dt)
                for dt in (np.float64, np.float32))
    for name, got, a, b in zip(("loss", "dS", "d_true"), (outs[0][0], outs[0][2], outs[0][1]), r64, r32):
        assert bool(torch.isfinite(got).all())
        _close(got, a, b, "head %s %s" % (name, (B, H, n, pad)))
    for got, row in ((outs[0][3], user), (outs[0][4], true_w)):                  # one float32 product each: exact
        assert np.array_equal(got.cpu().numpy(), outs[0][1].cpu().numpy()[:, None] * row)
    s = _t(S.copy())                                                              # without the optional outputs
    assert torch.equal(ops.mind_ssm_head(_t(user), _t(true_w), *args[0], s, *args[1])[0], outs[0][0])
    dS = outs[0][2].cpu().numpy()
    assert dS[0, 0] == 0.0 and (n == 1 or dS[0, 1:].all())                         # the hit column: exactly 0
    assert dS[B - 1].all()                                                         # no hit: every column carries a gradient


# ------------------------------------------------------------------------------------------------ the layer, the trainer
def test_layer_matches_the_reference_on_both_golden_steps(engine_lib):
    G = K.gold()
    m = K.layer_of(G, DEV)
    K.check_layer(G, m, "gpu layer")
    assert m.step_count == 2
    again = K.layer_of(G, DEV)                                                     # the same two steps once more: bit for bit
    again.set_dict(G["p"])
    for s in range(2):
        hist, seq, label, neg = K.feeds(G, s, DEV)
        again.train_step(hist, seq, label, G["lr"], neg=neg)
    for k, v in m.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    m.eval()
    user_cap, W = m.forward(*K.feeds(G, 0, DEV)[:2])
    assert tuple(user_cap.shape) == (7, 3, 12) and tuple(W.shape) == (7, 3, 6) and bool(torch.isfinite(user_cap).all())


def test_search_finds_the_brute_force_top_n(engine_lib):
    from paddlerec_amd import ops
    from paddlerec_amd.mind import search_inner_product
    rng = np.random.default_rng(11)
    table, q = rng.standard_normal((1000, 16)).astype(np.float32), rng.standard_normal((12, 16)).astype(np.float32)
    D, I = search_inner_product(ops, ops.Workspace(DEV), _t(q), _t(table), 20, chunk=300)       # four chunks, one ragged
    scores = q.astype(np.float64) @ table.astype(np.float64).T
    want = np.argsort(-scores, axis=1, kind="stable")[:, :20]
    got = I.cpu().numpy()
    assert (np.sort(got, 1) == np.sort(want, 1)).mean() > 0.99                     # float32 ties at the cut may swap one id
    assert np.allclose(D.cpu().numpy(), np.take_along_axis(scores, got, 1), rtol=1e-5, atol=1e-5)
    assert (np.diff(D.cpu().numpy(), axis=1) <= 0).all()


def test_trainer_trains_on_the_sample_and_infers(engine_lib, tmp_path):
    from paddlerec_amd import trainer
    cfg = K.mind_config(tmp_path, epochs=1)
    out, m = trainer.train(cfg, "mind", device=DEV)
    assert len(out) == 1 and out[0]["batches"] == 3 and np.isfinite(out[0]["loss"]) and m.step_count == 3
    assert int(m.status.item()) == 0 and not bool(m.embedding_bias.any())
    res = trainer.infer(cfg, "mind", device=DEV)
    assert [r["epoch"] for r in res] == [0] and res[0]["samples"] == 12
    assert all(0.0 <= res[0][k] <= 1.0 for k in ("recall@20", "ndcg@20", "hitrate@20"))
