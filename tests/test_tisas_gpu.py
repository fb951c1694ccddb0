"""TiSASRec's kernels (csrc/tisas_ops.hip) and layer (paddlerec_amd/tisas.py) on the GPU against tests/tisas_ref.py.

Tolerance, everywhere: err = max|got - ref64| / max|ref64| per tensor against tisas_ref.py in float64; the bound is 8 x the same
error of tisas_ref.py evaluated in float32 on the same inputs, floor 1e-6 (tests/tisas_checks.py).  Both errors are printed.

Shapes, the smallest at which the kernels can go wrong:
  * base: B 3, L 5, D 6, T 4 with H 1 and H 2 (head size 3: no 16-byte rows anywhere).  Sample 0 starts with padding, sample 1
    is ALL padding (uniform rows over all keys, future ones included), sample 2 is full; tm holds 0 and T - 1, and row 2 of
    the time tables is hit by nothing: its gradient must be exactly 0;
  * L 18 with H 2: more than one block of 16 query rows, the second one partly filled;
  * the shipped L 50, D 50, H 1, T 257 at B 2, and L 70: more keys than a wavefront has lanes (two keys per lane);
  * B 130 at L 3: more samples than REC_TISAS_MAX_PARTIALS, so a block of the time-table pass owns two samples."""
import numpy as np
import pytest
import torch

import tisas_checks as TC
import tisas_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITES = ("att", "pos_k", "pos_v", "time_k", "time_v")


def _ops():
    from paddlerec_amd import ops
    return ops


def case(B, L, D, T, seed=0, pad=True):
    rng = np.random.default_rng(seed)
    log_seqs = rng.integers(1, 9, (B, L)).astype(np.int64)
    if pad and B >= 3:
        log_seqs[0, :min(2, L - 1)] = 0
        log_seqs[1, :] = 0
    ts = np.cumsum(rng.integers(0, 3, (B, L)), 1) * (log_seqs != 0)
    tm = np.minimum(np.abs(ts[:, :, None] - ts[:, None, :]), T - 1).astype(np.int64)
    if T == 4:
        tm[tm == 2] = 3                                # row 2 of the time tables is hit by nothing
        tm[-1, -1, 0], tm[-1, 0, 0] = T - 1, 0
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(B=B, L=L, D=D, T=T, log_seqs=log_seqs, tm=tm, q=f(B * L, D), k=f(B * L, D), v=f(B * L, D), d_out=f(B * L, D),
                tables=[0.5 * f(L, D), 0.5 * f(L, D), 0.5 * f(T, D), 0.5 * f(T, D)])


def dev(a):
    return torch.as_tensor(a).to(DEV).contiguous()


def rebuilt_mask(shape, p, seed, stream):
    """rec_dropout applied to ones: the mask the fused kernels must have used."""
    if not p:
        return None
    return _ops().dropout(torch.ones(*shape, dtype=torch.float32, device=DEV), p, seed, stream).cpu().numpy()


def attn_masks(c, H, probs, seed, streams):
    B, L, D = c["B"], c["L"], c["D"]
    shapes = dict(att=(B * H * L, L), pos_k=(B * L, D), pos_v=(B * L, D), time_k=(B * L * L, D), time_v=(B * L * L, D))
    p = dict(att=probs[0], pos_k=probs[1], pos_v=probs[1], time_k=probs[2], time_v=probs[2])
    return {s: rebuilt_mask(shapes[s], p[s], seed, st) for s, st in zip(SITES, streams)}


NAMES = ("out", "lse", "dq", "dk", "dv", "d_pos_k", "d_pos_v", "d_time_k", "d_time_v")


def ref_attn(c, H, masks, dtype):
    scale = 1.0 / np.sqrt(c["D"] // H)
    o, lse, cache = R.attn_fwd(c["q"], c["k"], c["v"], c["tables"], c["tm"], c["log_seqs"], H, scale, masks, dtype)
    return dict(zip(NAMES, (o, lse) + tuple(R.attn_bwd(c["d_out"], cache, dtype))))


def gpu_attn(c, H, probs=(0.0, 0.0, 0.0), seed=0, streams=(0, 0, 0, 0, 0), packed=False, accumulate=False, d_tables=None):
    ops = _ops()
    B, L, D = c["B"], c["L"], c["D"]
    scale = 1.0 / np.sqrt(D // H)
    if packed:                                         # q, k, v and the gradients as column ranges of wider matrices
        qkv = torch.zeros(B * L, 3 * D + 5, device=DEV)
        qkv[:, :D], qkv[:, D + 2:2 * D + 2], qkv[:, 2 * D + 5:] = dev(c["q"]), dev(c["k"]), dev(c["v"])
        q, k, v = qkv[:, :D], qkv[:, D + 2:2 * D + 2], qkv[:, 2 * D + 5:]
        dqkv = torch.full((B * L, 3 * D + 5), 7.0, device=DEV)
        grads = (dqkv[:, :D], dqkv[:, D + 2:2 * D + 2], dqkv[:, 2 * D + 5:])
        d_out = torch.zeros(B * L, D + 3, device=DEV)[:, 1:D + 1]
        d_out.copy_(dev(c["d_out"]))
        out = torch.full((B * L, D + 1), 7.0, device=DEV)[:, :D]
    else:
        q, k, v, d_out, grads, out = dev(c["q"]), dev(c["k"]), dev(c["v"]), dev(c["d_out"]), None, None
    tables = [dev(t) for t in c["tables"]]
    tm, ls = dev(c["tm"]), dev(c["log_seqs"])
    status = ops.new_status(DEV)
    o, lse = ops.tisas_attn_fwd(q, k, v, tables, tm, ls, H, scale, probs, seed, streams, status=status, out=out)
    if d_tables is None:
        d_tables = [torch.full_like(t, 7.0) for t in tables]
    dq, dk, dv = ops.tisas_attn_bwd(q, k, v, tables, tm, ls, H, scale, lse, d_out, d_tables, probs, seed, streams, grads=grads,
                                    accumulate=accumulate)
    if packed:
        assert float(dqkv[:, D:D + 2].min()) == 7.0 and float(dqkv[:, 2 * D + 2:2 * D + 5].max()) == 7.0   # the gaps are not written
    res = dict(zip(NAMES, [t.cpu().numpy() for t in (o, lse, dq, dk, dv) + tuple(d_tables)]))
    res["status"] = int(status.item())
    return res


def compare(got, c, H, masks, what):
    r64, r32 = ref_attn(c, H, masks, np.float64), ref_attn(c, H, masks, np.float32)
    for n in NAMES:
        TC.check_tensor(what, n, got[n], r64[n], r32[n])
    assert got["status"] == 0


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("packed", [False, True])
def test_attention_base_shape(H, packed):
    c = case(3, 5, 6, 4)
    got = gpu_attn(c, H, packed=packed)
    compare(got, c, H, None, "base H%d" % H)
    assert not got["d_time_k"][2].any() and not got["d_time_v"][2].any()            # the row nothing hit: exactly zero
    assert (c["tm"] == 0).any() and (c["tm"] == 3).any() and not (c["tm"] == 2).any()
    # the all-padding sample: every row attends uniformly over ALL keys, so its output rows are all the same mean
    out = got["out"].reshape(3, 5, 6)
    assert (c["tm"][1] == 0).all() and np.abs(out[1] - out[1, :1]).max() <= 1e-6 * np.abs(out[1]).max()
    lse = got["lse"].reshape(3, H, 5)
    assert (lse[1] == np.float32(-2.0 ** 32)).all() and (lse[0, :, :2] == np.float32(-2.0 ** 32)).all()


@pytest.mark.parametrize("B,L,D,T,H", [(2, 18, 8, 5, 2), (2, 50, 50, 257, 1), (1, 70, 50, 257, 1), (130, 3, 4, 3, 2)])
def test_attention_tiles_and_the_shipped_shape(B, L, D, T, H):
    c = case(B, L, D, T, seed=L)
    compare(gpu_attn(c, H), c, H, None, "L%d D%d" % (L, D))


def test_accumulate_adds_to_the_table_gradients():
    c = case(3, 5, 6, 4)
    first = gpu_attn(c, 2)
    d_tables = [torch.full((n, 6), 0.25, device=DEV) for n in (5, 5, 4, 4)]
    second = gpu_attn(c, 2, accumulate=True, d_tables=d_tables)
    for n in NAMES[5:]:
        assert np.array_equal(second[n], np.float32(0.25) + first[n]), n


@pytest.mark.parametrize("probs", [(0.2, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, 0.2), (0.2, 0.2, 0.2)])
@pytest.mark.parametrize("H", [1, 2])
def test_attention_dropout_sites(probs, H):
    c = case(3, 5, 6, 4, seed=3)
    seed, streams = 4242, (11, 12, 13, 2 ** 40 + 14, 15)
    masks = attn_masks(c, H, probs, seed, streams)
    assert all((masks[s] is None) == (p == 0.0) for s, p in zip(SITES, (probs[0], probs[1], probs[1], probs[2], probs[2])))
    for m in masks.values():
        if m is not None:
            u = np.unique(m)
            assert len(u) == 2 and u[0] == 0 and abs(u[1] - 1.25) < 1e-6 and 0.6 < (m != 0).mean() < 0.95
    compare(gpu_attn(c, H, probs, seed, streams), c, H, masks, "drop %s" % (probs,))


def test_p_zero_is_the_no_dropout_path_bit_for_bit():
    c = case(3, 5, 6, 4, seed=5)
    a, b = gpu_attn(c, 2), gpu_attn(c, 2, (0.0, 0.0, 0.0), 99, (5, 6, 7, 8, 9))
    for n in NAMES:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n


def test_attention_reruns_bit_identical():
    c = case(2, 50, 50, 257, seed=8)
    probs, streams = (0.2, 0.2, 0.2), (1, 2, 3, 4, 5)
    a, b = gpu_attn(c, 1, probs, 7, streams), gpu_attn(c, 1, probs, 7, streams)
    for n in NAMES:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n
    other = gpu_attn(c, 1, probs, 8, streams)
    assert not np.array_equal(a["out"], other["out"])                                  # the seed matters


def test_out_of_range_time_id_sets_the_status_flag():
    from paddlerec_amd import _lib
    c = case(3, 5, 6, 4)
    for bad in (4, -1, 2 ** 40):
        c2 = dict(c, tm=c["tm"].copy())
        c2["tm"][2, 3, 1] = bad
        got = gpu_attn(c2, 1)
        assert got["status"] == _lib.REC_FLAG_INDEX_OOB
        c2["tm"][2, 3, 1] = 0                                                          # it reads row 0
        want = gpu_attn(c2, 1)
        for n in NAMES:
            assert np.array_equal(got[n], want[n]), n


def test_limits_are_refused_with_einval():
    from paddlerec_amd._lib import RecError
    ops = _ops()
    for B, L, D, T, H in ((1, 129, 4, 3, 1), (1, 4, 65, 3, 1), (1, 128, 64, 3, 1)):
        c = case(B, L, D, T, pad=False)
        with pytest.raises(RecError, match=r"rc=-1"):
            ops.tisas_attn_fwd(dev(c["q"]), dev(c["k"]), dev(c["v"]), [dev(t) for t in c["tables"]], dev(c["tm"]), dev(c["log_seqs"]),
                               H, 1.0)
    c = case(1, 4, 64, 257, pad=False)                                                 # 257 * 64 > REC_TISAS_MAX_TIME_TILE
    args = (dev(c["q"]), dev(c["k"]), dev(c["v"]), [dev(t) for t in c["tables"]], dev(c["tm"]), dev(c["log_seqs"]), 1, 1.0)
    out, lse = ops.tisas_attn_fwd(*args)                                               # the forward keeps no time tile
    with pytest.raises(RecError, match=r"rc=-1"):
        ops.tisas_attn_bwd(*args, lse, dev(c["d_out"]), [torch.zeros_like(dev(t)) for t in c["tables"]])
    with pytest.raises(RecError, match=r"rc=-1"):
        ops.tisas_attn_fwd(*args[:6], 3, 1.0)                                          # 64 % 3 != 0


# ------------------------------------------------------------------------------------------------ layer norm, embed, head
@pytest.mark.parametrize("m,n", [(7, 6), (9, 50), (130, 70)])
def test_affine_layer_norm(m, n):
    ops = _ops()
    rng = np.random.default_rng(m)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, r, gamma, beta, dy, dy2, e1, e2 = f(m, n), f(m, n), 1 + 0.3 * f(n), 0.3 * f(n), f(m, n), f(m, n), f(m, n), f(m, n)
    ids = rng.integers(0, 3, m).astype(np.int64)
    wide = lambda a: torch.cat([dev(a), torch.full((m, 3), 9.0, device=DEV)], 1)[:, :n]     # a row stride of n + 3
    for has_r, has_ids in ((False, False), (True, False), (True, True)):
        rr, ii = (r if has_r else None), (ids if has_ids else None)
        sum_out = torch.empty(m, n, device=DEV)
        y, mean, rstd = ops.affine_layer_norm_fwd(wide(x), dev(gamma), dev(beta), 1e-8, r=wide(rr) if has_r else None,
                                                  row_ids=dev(ii) if has_ids else None, sum_out=sum_out)
        r64, r32 = (R.ln_fwd(x, gamma, beta, 1e-8, rr, ii, dt) for dt in (np.float64, np.float32))
        for name, got, i in (("y", y, 0), ("t", sum_out, 1), ("mean", mean, 2)):
            TC.check_tensor("ln %dx%d" % (m, n), name, got.cpu().numpy(), r64[i], r32[i])
        if has_ids:
            assert not sum_out.cpu().numpy()[ids == 0].any()
            assert np.allclose(y.cpu().numpy()[ids == 0], beta)                             # a masked row normalises to beta
        else:
            TC.check_tensor("ln %dx%d" % (m, n), "rstd", rstd.cpu().numpy(), r64[3], r32[3])
        dg, db = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        g_in = wide(dy)
        dx = ops.affine_layer_norm_bwd(sum_out, mean, rstd, dev(gamma), g_in, dg, db, dy2=dev(dy2), e1=wide(e1), e2=dev(e2),
                                       row_ids=dev(ii) if has_ids else None, out=g_in)       # in place on dy
        b64, b32 = (R.ln_bwd(R.ln_fwd(x, gamma, beta, 1e-8, rr, ii, dt)[1], *R.ln_fwd(x, gamma, beta, 1e-8, rr, ii, dt)[2:], gamma,
                             dy.astype(dt) + dy2.astype(dt), ii, e1.astype(dt) + e2.astype(dt), dt) for dt in (np.float64, np.float32))
        for name, got, i in (("dx", dx, 0), ("dgamma", dg, 1), ("dbeta", db, 2)):
            TC.check_tensor("ln %dx%d" % (m, n), name, got.cpu().numpy(), b64[i], b32[i])


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_embed_forward_and_backward(p):
    from paddlerec_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(2)
    N, D, n = 12, 6, 35
    table = rng.standard_normal((N, D)).astype(np.float32)
    ids = rng.integers(0, N, n).astype(np.int64)
    ids[:3] = 0
    d_out = rng.standard_normal((n, D)).astype(np.float32)
    scale, seed, stream = float(np.sqrt(D)), 5, 77
    mask = rebuilt_mask((n, D), p, seed, stream)
    status = ops.new_status(DEV)
    out = ops.tisas_embed_fwd(dev(ids), dev(table), scale, p, seed, stream, status=status)
    G = torch.full((n, D + 2), 3.0, device=DEV)
    rows = ops.tisas_embed_bwd(dev(ids), dev(d_out), N, scale, p, seed, stream, out=G[:, :D])
    for name, got, fn, src in (("out", out, R.embed_fwd, table), ("rows", rows, R.embed_bwd, d_out)):
        r64, r32 = (fn(src, ids, scale, mask, dt) for dt in (np.float64, np.float32))
        TC.check_tensor("embed p%.1f" % p, name, got.cpu().numpy(), r64, r32)
    assert not out.cpu().numpy()[:3].any() and not rows.cpu().numpy()[:3].any() and float(G[:, D:].min()) == 3.0
    assert int(status.item()) == 0
    bad = ids.copy()
    bad[5] = N
    out2 = ops.tisas_embed_fwd(dev(bad), dev(table), scale, p, seed, stream, status=status)
    assert int(status.item()) == _lib.REC_FLAG_INDEX_OOB and not out2.cpu().numpy()[5].any()


def test_head():
    from paddlerec_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(4)
    N, D, n = 12, 50, 37
    table = rng.standard_normal((N, D)).astype(np.float32)
    table[0] = 0
    feats = rng.standard_normal((n, D)).astype(np.float32)
    pos, neg = rng.integers(1, N, n).astype(np.int64), rng.integers(1, N, n).astype(np.int64)
    pos[::4], neg[::4] = 0, 0
    G = torch.full((2 * n, D), 3.0, device=DEV)
    status = ops.new_status(DEV)
    loss2, d_feats, cp, cn, row_loss, pl, nl = ops.tisas_head(dev(feats), dev(pos), dev(neg), dev(table), status=status,
                                                              d_pos_rows=G[:n], d_neg_rows=G[n:])
    r64, r32 = (R.head(feats, pos, neg, table, dt) for dt in (np.float64, np.float32))
    assert float(loss2[1].item()) == r64["cnt"] == (pos != 0).sum()
    got = dict(loss=loss2[:1], d_feats=d_feats, coef_pos=cp, coef_neg=cn, row_loss=row_loss, pl=pl, nl=nl)
    for k, v in got.items():
        TC.check_tensor("head", k, v.cpu().numpy(), np.asarray(r64[k]).reshape(v.shape), np.asarray(r32[k]).reshape(v.shape))
    TC.check_tensor("head", "d_pos_rows", G[:n].cpu().numpy(), r64["coef_pos"][:, None] * feats, r32["coef_pos"][:, None] * feats)
    TC.check_tensor("head", "d_neg_rows", G[n:].cpu().numpy(), r64["coef_neg"][:, None] * feats, r32["coef_neg"][:, None] * feats)
    assert int(status.item()) == 0
    # nothing selected: the loss is NaN, as the reference's mean over an empty selection, and the gradients are zero
    z = torch.zeros(n, dtype=torch.int64, device=DEV)
    loss2, d_feats, cp, cn, _, _, _ = ops.tisas_head(dev(feats), z, dev(neg), dev(table))
    assert torch.isnan(loss2[0]) and float(loss2[1]) == 0.0 and not d_feats.any() and not cp.any() and not cn.any()
    bad = pos.copy()
    bad[1] = N + 3
    ops.tisas_head(dev(feats), dev(bad), dev(neg), dev(table), status=status)
    assert int(status.item()) == _lib.REC_FLAG_INDEX_OOB


# ------------------------------------------------------------------------------------------------ the layer
@pytest.mark.parametrize("name", TC.FIXTURES)
def test_layer_matches_the_golden(name):
    G = TC.gold(name)
    m = TC.layer_of(G, device=DEV)
    TC.check_layer(G, m, "gpu " + name[6:8])
    TC.check_infer(G, m, "gpu " + name[6:8])


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_layer_with_every_dropout_site(name):
    from test_tisas import masks_of
    G = TC.gold(name)
    m = TC.layer_of(G, device=DEV, dropout_rate=0.2, dropout_seed=31)
    TC.check_layer(G, m, "gpu drop " + name[6:8], masks_of=masks_of(rebuilt_mask))


def test_train_step_reruns_bit_identical():
    G = TC.gold(TC.FIXTURES[1])
    runs = []
    for _ in range(2):
        m = TC.layer_of(G, device=DEV, dropout_rate=0.2, dropout_seed=31)
        m.set_dict(G["p"])
        losses = [m.train_step(*TC.feeds(G, s, DEV), lr=G["lr"])[0].value().cpu().numpy() for s in range(G["steps"])]
        runs.append((losses, {k: v.cpu().numpy() for k, v in m.state_dict().items()},
                     {k: v.cpu().numpy() for k, v in m.last_gradients().items()}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i in (1, 2):
        for k in runs[0][i]:
            assert np.array_equal(runs[0][i][k].view(np.uint32), runs[1][i][k].view(np.uint32)), k


def test_trainer_train_then_infer(tmp_path, capsys):
    """Train, then --infer, through the trainer's command line on tests/golden/tisas_sample.txt."""
    import yaml
    from paddlerec_amd import trainer
    flat = TC.tisas_config(tmp_path, epochs=2)
    doc = {"runner": {}, "hyper_parameters": {"optimizer": {}}}
    for k, v in flat.items():
        part, _, key = k.partition(".")
        if part == "runner":
            doc["runner"][key] = v
        elif key.startswith("optimizer."):
            doc["hyper_parameters"]["optimizer"][key[len("optimizer."):]] = v
        elif part == "hyper_parameters":
            doc["hyper_parameters"][key] = v
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(doc))
    trainer.main(["-m", str(path), "--model", "tisas"])
    trained = capsys.readouterr().out
    epochs = [eval(ln, {"__builtins__": {}}, {}) for ln in trained.splitlines() if ln.startswith("{'epoch':")]
    assert len(epochs) == 2 and all(np.isfinite(e["loss"]) and e["batches"] == 1 for e in epochs)
    trainer.main(["-m", str(path), "--model", "tisas", "--infer"])
    out = capsys.readouterr().out
    (line,) = [ln for ln in out.splitlines() if "NDCG@10" in ln]
    vals = eval(line, {"__builtins__": {}}, {})              # the summary dict the trainer prints
    assert vals["batches"] == 2 and np.isfinite(vals["NDCG@10"]) and np.isfinite(vals["HR@10"])
    assert 0.0 <= vals["NDCG@10"] <= vals["HR@10"] <= 1.0
