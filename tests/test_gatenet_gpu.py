"""rank/gatenet on the HIP kernels (csrc/gate_ops.hip): the five rec_gate_* / rec_relu_mask_inplace entry points against
the float64 NumPy restatement (tests/gatenet_ref.py), the layer against the fixture, the trainer loops.

Inputs of the kernel tests are the net's own: table rows ~ U[-1, 1], gate scalars ~ N(0, 1), so the sigmoid's argument
w_s * sum_k e_k has standard deviation sqrt(D / 3) — about 4 at D 48, where the draws reach both tails.  Tolerance:
helpers.assert_close_scaled at 2e-5, the bar of the DCN / FFM / FEFM kernels against float64.  Every value here is a
product of a handful of float32 factors and a sum of at most D (or, for d w_s, B) terms: the float32 restatement's own
scaled error against float64 on these inputs stays under 1e-6, so no case asks for more."""
import numpy as np
import pytest
import torch

import gatenet_ref as GR
from helpers import assert_close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 2e-5
DN = 13
SENT = -7.25                  # what the floats no kernel may touch hold


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _table(N, D, rng):
    """[N, D] table ~ U[-1, 1]: the [:, :D] view of a line-aligned record buffer when D % 4 == 0 (16-byte rows), a
    contiguous tensor otherwise."""
    w = rng.uniform(-1.0, 1.0, (N, D)).astype(np.float32)
    if D % 4:
        return w, _t(w)
    rec = torch.zeros(N, (D + 31) // 32 * 32, device=DEV)
    rec[:, :D] = _t(w)
    return w, rec[:, :D]


def _rows(B, width, ld, offset, fill=SENT):
    """A [B, width] device view of row stride ld, `offset` floats into a buffer filled with `fill`."""
    buf = torch.full((B * ld + offset + 8,), fill, dtype=torch.float32, device=DEV)
    return torch.as_strided(buf, (B, width), (ld, 1), offset), buf


def _untouched(buf, B, width, ld, offset):
    """True when every float of `buf` outside the [B, width] view still holds the sentinel, bit for bit."""
    a = buf.cpu().numpy().copy()
    for b in range(B):
        a[offset + b * ld: offset + b * ld + width] = SENT
    return bool((a == np.float32(SENT)).all())


def _emb_case(B, S, D, ld, offset, seed, N=50, padding_idx=None, ids=None):
    """fwd + bwd through ops at feature-row stride ld -> numpy dict; checks that nothing outside the slots moved."""
    from paddlerec_amd import ops
    rng = np.random.default_rng(seed)
    w_np, W = _table(N, D, rng)
    gw = rng.standard_normal(S).astype(np.float32)
    if ids is None:
        ids = rng.integers(0, N, (B, S), dtype=np.int64)                      # N 50: duplicates in every batch
        if B:
            ids[0, 0] = 0
    g_np = rng.standard_normal((B, S * D)).astype(np.float32)
    status = ops.new_status(DEV)
    ws = ops.Workspace(DEV)
    out, obuf = _rows(B, S * D, ld, offset)
    gv, gbuf = _rows(B, S * D, ld, offset)
    ops.gate_emb_fwd(_t(ids), W, _t(gw), padding_idx, status, out=out)
    torch.cuda.synchronize()
    assert _untouched(obuf, B, S * D, ld, offset), "the forward wrote outside its slots"
    gv.copy_(_t(g_np))
    _, dw, _ = ops.gate_emb_bwd(_t(ids), W, _t(gw), gv, ws, padding_idx, status)
    torch.cuda.synchronize()
    assert _untouched(gbuf, B, S * D, ld, offset), "the backward wrote outside its slots"
    return dict(ids=ids, w=w_np, gw=gw, g=g_np, out=out.cpu().numpy(), de=gv.cpu().numpy(), dw=dw.cpu().numpy(),
                status=int(status.item()))


def _emb_want(r, padding_idx=None):
    ids, N = r["ids"], r["w"].shape[0]
    B, S = ids.shape
    live = (ids >= 0) & (ids < N)
    if padding_idx is not None:
        live &= ids != padding_idx
    e = r["w"].astype(np.float64)[np.where(live, ids, 0)] * live[..., None]
    out = GR.gate_emb_forward(e, r["gw"])[0] * live[..., None]
    de, dw = GR.gate_emb_backward(e, r["gw"], r["g"].reshape(B, S, -1) * live[..., None])
    return out.reshape(B, -1), (de * live[..., None]).reshape(B, -1), dw


def _emb_check(r, padding_idx=None):
    B, S = r["ids"].shape
    assert r["dw"].shape == (S,)
    if B == 0:
        assert not r["dw"].any()                                              # an empty batch sum
        return
    out, de, dw = _emb_want(r, padding_idx)
    assert_close_scaled(r["out"], out, REL, "out")
    assert_close_scaled(r["de"], de, REL, "d e")
    assert_close_scaled(r["dw"], dw, REL, "d w_s")


@pytest.mark.parametrize("B", [0, 1, 63, 1000])
@pytest.mark.parametrize("S", [1, 26])
@pytest.mark.parametrize("D", [1, 4, 9, 16, 33, 48])
def test_gate_emb_shapes_and_strides(engine_lib, D, S, B):
    """One-lane groups (D 1, 4), ragged last lanes (D 9, 33, 48 as 12 float4 lanes of 16), multi-lane groups; B 1000 x S 26
    spans many blocks.  Feature rows back to back at S*D + Dn floats, 3 floats into the buffer (the scalar path), and at
    the stride rounded up to 4, 4 floats in (16-byte vectors where D % 4 == 0).  The dense columns, the padding floats and
    the floats in front of the first row keep their bits through both kernels."""
    d = S * D + DN
    for ld, offset in ((d, 3), ((d + 3) // 4 * 4, 4)):
        r = _emb_case(B, S, D, ld, offset, seed=D * 1000 + S * 10 + B % 7 + ld % 2)
        assert r["status"] == 0
        _emb_check(r)


def test_gate_emb_id_zero_padding_and_out_of_range(engine_lib):
    B, S, D, N = 6, 26, 9, 50
    rng = np.random.default_rng(3)
    ids = rng.integers(1, N, (B, S), dtype=np.int64)
    ids[:, 2] = 7                                                             # duplicates
    ids[1, 4] = ids[3, 0] = 0
    live = _emb_case(B, S, D, 248, 0, 5, N, None, ids)                        # padding_idx None: id 0 is a live row
    assert live["status"] == 0
    _emb_check(live)
    slot = lambda a, b, s: a[b, s * D:(s + 1) * D]
    assert slot(live["out"], 1, 4).any() and slot(live["de"], 1, 4).any() and slot(live["de"], 3, 0).any()
    pad = _emb_case(B, S, D, 248, 0, 5, N, 0, ids)                            # the same ids with padding_idx = 0
    assert pad["status"] == 0
    _emb_check(pad, 0)
    assert not slot(pad["out"], 1, 4).any() and not slot(pad["de"], 1, 4).any() and not slot(pad["de"], 3, 0).any()
    assert np.array_equal(slot(pad["out"], 0, 0), slot(live["out"], 0, 0))
    bad = ids.copy()
    bad[2, 5], bad[4, 1] = N, -1                                              # bounds-checked before any load
    oob = _emb_case(B, S, D, 248, 0, 5, N, None, bad)
    assert oob["status"] & 1
    _emb_check(oob)
    assert not slot(oob["out"], 2, 5).any() and not slot(oob["out"], 4, 1).any()
    assert not slot(oob["de"], 2, 5).any() and not slot(oob["de"], 4, 1).any()


def test_gate_weight_gradient_bit_identical_reruns(engine_lib):
    """d w_s is a batch sum folded in a fixed order: two runs on the same inputs give identical bits (B 20000 x S 26 at
    D 9: 32500 chunks over the 2048 blocks of the backward's grid)."""
    a = _emb_case(20000, 26, 9, 248, 0, seed=10, N=5000)
    b = _emb_case(20000, 26, 9, 248, 0, seed=10, N=5000)
    assert np.array_equal(a["dw"], b["dw"]) and np.array_equal(a["de"], b["de"]) and np.array_equal(a["out"], b["out"])
    _emb_check(a)


def _hidden_problem(B, n, seed):
    rng = np.random.default_rng(seed)
    y = np.maximum(rng.standard_normal((B, n)), 0).astype(np.float32)         # a ReLU output: about half exact zeros
    t = (rng.standard_normal((B, n)) * 1.5).astype(np.float32)                # tanh(t) < 0 on about half
    u = rng.standard_normal((B, n)).astype(np.float32)
    acc = rng.standard_normal((B, n)).astype(np.float32)
    return y, t, u, acc


@pytest.mark.parametrize("B", [0, 1, 63, 1000])
@pytest.mark.parametrize("n", [1, 32, 100, 512])
@pytest.mark.parametrize("strided", [False, True])
def test_gate_hidden_and_relu_mask(engine_lib, n, B, strided):
    """Contiguous rows (16-byte vectors where n % 4 == 0) and rows of stride n + 3 starting 1 float into their buffers
    (the scalar form); the floats between the rows keep their bits."""
    from paddlerec_amd import ops
    y, t, u, acc = _hidden_problem(B, n, seed=n * 10 + B % 7)
    ld, off = (n + 3, 1) if strided else (n, 0)
    views = {}
    for name, a in (("y", y), ("t", t), ("u", u), ("dy", acc), ("x", None), ("dt", None), ("uh", None)):
        views[name] = _rows(B, n, ld, off)
        if a is not None:
            views[name][0].copy_(_t(a))
    V = {k: v[0] for k, v in views.items()}
    x, h = ops.gate_hidden_fwd(V["y"], V["t"], out=V["x"])
    assert h is V["t"] and x is V["x"]
    dt, uh = ops.gate_hidden_bwd(V["u"], V["y"], h, out=(V["dt"], V["uh"]))
    ops.relu_mask_(V["dy"], V["y"])
    torch.cuda.synchronize()
    for name, (_, buf) in views.items():
        assert _untouched(buf, B, n, ld, off), name
    if B == 0:
        return
    wx, wh = GR.gate_hidden_forward(y, t)
    if B * n > 8:
        assert ((wx < 0) & (y > 0)).any() and (y == 0).any()                  # the mask of y differs from the mask of x
    wdt, wuh = GR.gate_hidden_backward(u, y, wh)
    assert_close_scaled(x.cpu().numpy(), wx, REL, "x")
    assert_close_scaled(h.cpu().numpy(), wh, REL, "h")
    assert_close_scaled(dt.cpu().numpy(), wdt, REL, "dt")
    assert_close_scaled(uh.cpu().numpy(), wuh, REL, "uh")
    assert np.array_equal(V["dy"].cpu().numpy(), np.where(y > 0, acc, np.float32(0)))
    # new tensors when no outputs are given
    x2, _ = ops.gate_hidden_fwd(V["y"], _t(t))
    assert torch.equal(x2, x.contiguous())


def test_ops_reject_bad_arguments(engine_lib):
    from paddlerec_amd import _lib, ops
    ws = ops.Workspace(DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    ids = torch.zeros(4, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.RecError, match="one scalar per field"):
        ops.gate_emb_fwd(ids, z(10, 8), z(4))
    with pytest.raises(_lib.RecError, match=r"\[B, S\]"):
        ops.gate_emb_fwd(ids.reshape(-1), z(10, 8), z(3))
    with pytest.raises(_lib.RecError, match="out must be"):
        ops.gate_emb_fwd(ids, z(10, 8), z(3), out=z(4, 23))
    with pytest.raises(_lib.RecError, match="int64"):
        ops.gate_emb_fwd(ids.to(torch.int32), z(10, 8), z(3))
    with pytest.raises(_lib.RecError, match="device"):
        ops.gate_emb_fwd(ids, torch.zeros(10, 8), z(3))
    with pytest.raises(_lib.RecError, match="g must be"):
        ops.gate_emb_bwd(ids, z(10, 8), z(3), z(4, 25), ws)
    with pytest.raises(_lib.RecError, match="d_gate_w"):
        ops.gate_emb_bwd(ids, z(10, 8), z(3), z(4, 24), ws, out=z(4))
    with pytest.raises(_lib.RecError, match="t must be"):
        ops.gate_hidden_fwd(z(4, 8), z(4, 7))
    with pytest.raises(_lib.RecError, match="uh must be"):
        ops.gate_hidden_bwd(z(4, 8), z(4, 8), z(4, 8), out=(z(4, 8), z(8, 4)))
    with pytest.raises(_lib.RecError, match="alias"):
        u = z(4, 8)
        ops.gate_hidden_bwd(u, z(4, 8), z(4, 8), out=(u, z(4, 8)))
    with pytest.raises(_lib.RecError, match="y must be"):
        ops.relu_mask_(z(4, 8), torch.zeros(4, 8))


# ------------------------------------------------------------------ the layer and the loops
def test_layer_matches_fixture_gpu(engine_lib):
    import test_gatenet
    test_gatenet.check_layer_on_fixture(DEV, None, 2e-5)


@pytest.mark.parametrize("lazy", [False, True])
def test_adam_trajectory_gpu(engine_lib, lazy):
    import test_gatenet
    test_gatenet.check_adam_trajectory(DEV, None, lazy, 1e-5)


@pytest.mark.parametrize("emb_gate,hidden_gate", [(True, True), (True, False), (False, True), (False, False)])
def test_gate_switches_gpu(engine_lib, emb_gate, hidden_gate):
    import test_gatenet
    test_gatenet.check_gate_switches(DEV, None, emb_gate, hidden_gate, 2e-5)


def test_full_size_step_b512(engine_lib):
    """gatenet/config.yaml: 1 000 001 rows, D 9, the [512, 256, 128, 32] tower, both gates, batch 512.  Two train steps; the
    loss and prediction of the first equal the restatement's on the same draw, and exactly the rows the batches touched
    have moved (a zero gradient on zero moments moves nothing under the dygraph Adam either; row 0 is a row like any).

    The tower's weights are rescaled first (Linear x 2, hidden gates x 4).  With the reference's own initialisers a gated
    layer's output is about the SQUARE of its input's size (x = y tanh(y G) ~ y^2 for small y), so after four layers the
    activations are ~1e-10, every prediction is 0.5 +- 1e-11 and the table's gradients are ~1e-21: far below the
    ~1e-12 at which lr g / (|g| + eps) of Adam (eps 1e-8, lr 1e-3) still exceeds half an ulp of a weight of size 1, so
    touched rows would not move in float32, in the reference no more than here, and a comparison of 0.5 with 0.5 would
    show nothing.  Rescaled, the activations keep a size of 0.4 - 0.6 through the tower and the predictions spread over
    (0.05, 0.97); the restatement's merged gradient of every touched row is asserted to be above 1e-9, a factor 1000
    over that threshold, before the rows are compared."""
    from paddlerec_amd.gatenet import GateDNNLayer
    N, B, S, D = 1000001, 512, 26, 9
    m = GateDNNLayer(N, D, DN, S, [512, 256, 128, 32], True, True, device=DEV)
    for i in range(4):
        m.dense.p["linear_%d.weight" % i].mul_(2.0)
        m.dense.p["hidden_gate_weight_%d" % i].mul_(4.0)
    rng = np.random.default_rng(B)
    ids = rng.integers(0, N, (B, S), dtype=np.int64)
    ids[rng.random((B, S)) < 0.05] = 0
    ids[:, 1] = N - 1                                                         # a hot row at the table's end
    dense = rng.random((B, DN), dtype=np.float32)
    label = (rng.random((B, 1)) < 0.3).astype(np.int64)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    loss, pred = m.train_step(_t(ids), _t(dense), _t(label), lr=1e-3)
    o = GR.loss_and_grads(ids, dense, label, sd, D)
    f = {"pred": o["pred"]}
    print("full size: pred in [%.4f, %.4f], max |pred - want| %.3e, loss %.7f want %.7f" % (
        o["pred"].min(), o["pred"].max(), np.abs(pred.cpu().numpy() - o["pred"]).max(), float(loss), float(o["loss"])))
    assert o["pred"].max() - o["pred"].min() > 0.5                              # not the vanishing regime
    np.testing.assert_allclose(float(loss), float(GR.log_loss_mean(f["pred"], label)), rtol=1e-5)
    np.testing.assert_allclose(pred.cpu().numpy(), f["pred"], rtol=1e-5, atol=1e-6)
    m.train_step(_t(ids), _t(dense), _t(label), lr=1e-3)
    assert int(m.status.item()) == 0 and m.step_count == 2
    moved = (m.embedding.cpu().numpy() != sd["embedding.weight"]).any(axis=1)
    touched = np.zeros(N, bool)
    touched[ids.reshape(-1)] = True
    row_grad = np.abs(o["g"]["embedding.weight"][touched]).max(axis=1)
    print("full size: %d touched rows, smallest merged row gradient %.3e, %d moved" % (
        touched.sum(), row_grad.min(), moved.sum()))
    assert row_grad.min() > 1e-9                                              # every touched row has a gradient Adam can act on
    assert touched[0] and np.array_equal(moved, touched)
    assert not m.rec[:, D:].any()
    now = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for s in range(S):
        assert now["embedding_gate_weight_%d" % s] != sd["embedding_gate_weight_%d" % s], s
    for i in range(4):
        k = "hidden_gate_weight_%d" % i
        assert (now[k] != sd[k]).any(), k
    del m


@pytest.mark.parametrize("lazy", [True, False])
def test_gatenet_trainer_loops_gpu(engine_lib, tmp_path, lazy):
    import test_gatenet
    test_gatenet.run_trainer_loops(tmp_path, "cuda", None, lazy)


def test_trainer_command_line_model_gatenet_gpu(engine_lib, tmp_path, capsys):
    """`python -m paddlerec_amd.trainer -m <yaml> --model gatenet` and `--infer` on the sample lines (the YAML sits in a
    directory whose name says nothing, so the switch is what selects the net)."""
    import os
    import shutil
    from helpers import GOLDEN
    from paddlerec_amd import trainer
    d = tmp_path / "somewhere"
    (d / "data").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "criteo_slot_sample.txt"), d / "data" / "part-0")
    out = str(tmp_path / "out")
    (d / "config.yaml").write_text(
        "runner:\n  train_data_dir: data\n  test_data_dir: data\n  use_auc: True\n  train_batch_size: 2\n  epochs: 1\n"
        "  print_interval: 2\n  model_save_path: %s\n  infer_batch_size: 2\n  infer_load_path: %s\n  infer_start_epoch: 0\n"
        "  infer_end_epoch: 1\nhyper_parameters:\n  optimizer:\n    class: Adam\n    learning_rate: 0.001\n"
        "  sparse_inputs_slots: 27\n  sparse_feature_number: 1000001\n  sparse_feature_dim: 9\n  dense_input_dim: 13\n"
        "  fc_sizes: [32, 16]\n  use_embedding_gate: True\n  use_hidden_gate: True\n" % (out, out))
    trainer.main(["-m", str(d / "config.yaml"), "--model", "gatenet"])
    assert os.path.exists(os.path.join(out, "0", "rec.pdparams"))
    trainer.main(["-m", str(d / "config.yaml"), "--model", "gatenet", "--infer"])
    printed = capsys.readouterr().out
    assert printed.count("'epoch': 0") == 2 and "'auc'" in printed
