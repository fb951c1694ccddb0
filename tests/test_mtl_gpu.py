"""The multitask kernels (csrc/mtl_ops.hip) and nets (paddlerec_amd/mmoe.py, ple.py) on the GPU against tests/mtl_ref.py.

Kernel cases: err = max|got - ref64| / max|ref64| per output, bound max(8 x the float32 restatement's error on the same
inputs, 1e-6); every case is run twice and the two results compared bit for bit.  The shapes are the smallest at which a
path changes: B below, at and across a block's rows (a block holds 256 >> k rows, k from S); S = 1, 3 (scalar), 16 (float4,
4 lanes a row), 68 (float4: 17 chunks in 32 lanes; scalar with odd strides: 64 lanes making two column passes)."""
import numpy as np
import pytest
import torch

import mtl_checks as K
import mtl_cpu_kernels
import mtl_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# name: (B, S, n_slots, gates, extra row stride of every operand)
MIX_CASES = {
    "b1_s1": (1, 1, 3, [(0, 3, 0, 0)], 0),
    "b5_s3_two_ranges": (5, 3, 4, [(0, 2, 2, 2), (1, 3, 0, 0)], 0),
    "b64_s16_block_rows": (64, 16, 8, [(0, 8, 0, 0), (0, 8, 0, 0)], 0),
    "b257_s68": (257, 68, 5, [(0, 3, 3, 2), (3, 2, 0, 3)], 0),
    "unselected_slots": (5, 4, 5, [(0, 2, 3, 1)], 0),
    "slot_in_three_gates": (5, 16, 4, [(0, 2, 0, 0), (1, 2, 0, 0), (3, 1, 1, 1)], 0),
    "sixty_four_experts": (5, 4, 64, [(0, 40, 40, 24)], 0),
    "sixteen_gates": (64, 8, 6, [(g % 5, 1 + g % 2, 0, 0) if g % 3 else (4, 2, 0, 3) for g in range(16)], 0),
    "strided_s16": (65, 16, 3, [(0, 2, 2, 1), (0, 3, 0, 0)], 8),
    "strided_s68_scalar": (9, 68, 2, [(0, 2, 0, 0), (1, 1, 0, 1)], 3),
}


def _padded(a, pad):
    """a [B, n] on the device inside a [B, n + pad] buffer whose padding columns hold NaN -> (view, buffer)."""
    a = torch.as_tensor(np.ascontiguousarray(a, np.float32))
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = a.to(DEV)
    return buf[:, :a.shape[1]], buf


def _padding_intact(buf, n):
    return buf.shape[1] == n or bool(torch.isnan(buf[:, n:]).all())


def _close(got, ref64, ref32, what):
    e, b = R.relerr(got.cpu().numpy(), ref64), K.bound_of(ref32, ref64)
    print("%-40s err %.3g  float32-ref err %.3g" % (what, e, b / 8))
    assert e <= b, (what, e, b)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("name", sorted(MIX_CASES))
def test_mix_kernels(engine_lib, name, relu):
    from paddlerec_amd import ops
    B, S, n_slots, gates, pad = MIX_CASES[name]
    rng = np.random.default_rng(sorted(MIX_CASES).index(name))
    mix = ops.MtlMix(S, n_slots, gates)
    sl = R.gate_slots(mix.gates)
    H = np.maximum(rng.standard_normal((B, n_slots * S)), 0).astype(np.float32)          # exact zeros: the ReLU's off side
    logits = (2 * rng.standard_normal((B, mix.n_logit))).astype(np.float32)
    logits[0, :] = 80.0 * np.sign(logits[0, :])                                           # saturated rows
    if B > 2:
        logits[2, 0] = -80.0
    dmix = rng.standard_normal((B, mix.n_gates * S)).astype(np.float32)
    assert (H == 0).any()
    Hv, _ = _padded(H, pad)
    Lv, _ = _padded(logits, pad)
    Dv, _ = _padded(dmix, pad)
    ref = {dt: R.mix_fwd(H, logits, S, n_slots, sl, dtype=dt) for dt in (np.float64, np.float32)}
    outs = []
    for _ in range(2):
        Pv, Pb = _padded(np.zeros((B, mix.n_logit)), pad)
        Mv, Mb = _padded(np.zeros((B, mix.n_gates * S)), pad)
        ops.mtl_mix_fwd(mix, Hv, Lv, prob=Pv, out=Mv)
        assert _padding_intact(Pb, mix.n_logit) and _padding_intact(Mb, mix.n_gates * S)
        outs.append((Pv.clone(), Mv.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _close(outs[0][0], ref[np.float64][0], ref[np.float32][0], name + " prob")
    _close(outs[0][1], ref[np.float64][1], ref[np.float32][1], name + " mix")
    # the backward from the device's own probabilities
    prob = outs[0][0].cpu().numpy()
    Pv, _ = _padded(prob, pad)
    refb = {dt: R.mix_bwd(H, prob, dmix, S, n_slots, sl, relu, dtype=dt) for dt in (np.float64, np.float32)}
    outs = []
    for _ in range(2):
        Gh, Ghb = _padded(np.full((B, n_slots * S), 7.0), pad)
        Gl, Glb = _padded(np.full((B, mix.n_logit), 7.0), pad)
        ops.mtl_mix_bwd(mix, Hv, Pv, Dv, relu, dH=Gh, dlogits=Gl)
        assert _padding_intact(Ghb, n_slots * S) and _padding_intact(Glb, mix.n_logit)
        outs.append((Gh.clone(), Gl.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _close(outs[0][0], refb[np.float64][0], refb[np.float32][0], name + " dH")
    _close(outs[0][1], refb[np.float64][1], refb[np.float32][1], name + " dlogits")
    used = {e for s in sl for e in s}
    for e in range(n_slots):
        if e not in used:                                                                 # zeros written, not left stale
            assert not outs[0][0][:, e * S:(e + 1) * S].any()
    if relu:
        assert not outs[0][0][torch.as_tensor(H == 0).to(DEV)].any()


def _offset(a):
    """a [B, n] on the device as columns 1 .. n of a [B, n + 4] NaN buffer: row stride a multiple of 4, base 4 bytes past
    a 16-byte boundary -> (view, buffer)."""
    a = torch.as_tensor(np.ascontiguousarray(a, np.float32))
    buf = torch.full((a.shape[0], a.shape[1] + 4), NAN, dtype=torch.float32, device=DEV)
    buf[:, 1:1 + a.shape[1]] = a.to(DEV)
    view = buf[:, 1:1 + a.shape[1]]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 0
    return view, buf


def _offset_intact(buf):
    return bool(torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, -3:]).all())


def test_mix_kernels_unaligned_base_takes_the_scalar_form(engine_lib):
    """S and every stride are multiples of 4 but H, mix, dmix and dH start 4 bytes past a 16-byte boundary: float4 accesses
    would be misaligned, the entry points must pick the scalar kernels."""
    from paddlerec_amd import ops
    B, S, n_slots, gates = 67, 16, 3, [(0, 2, 2, 1), (0, 3, 0, 0)]
    rng = np.random.default_rng(7)
    mix = ops.MtlMix(S, n_slots, gates)
    sl = R.gate_slots(mix.gates)
    H = np.maximum(rng.standard_normal((B, n_slots * S)), 0).astype(np.float32)
    logits = (2 * rng.standard_normal((B, mix.n_logit))).astype(np.float32)
    dmix = rng.standard_normal((B, mix.n_gates * S)).astype(np.float32)
    Hv, _ = _offset(H)
    Dv, _ = _offset(dmix)
    Lv = torch.as_tensor(logits).to(DEV)
    Mv, Mb = _offset(np.zeros((B, mix.n_gates * S)))
    prob, _ = ops.mtl_mix_fwd(mix, Hv, Lv, out=Mv)
    ref = {dt: R.mix_fwd(H, logits, S, n_slots, sl, dtype=dt) for dt in (np.float64, np.float32)}
    assert _offset_intact(Mb)
    _close(prob, ref[np.float64][0], ref[np.float32][0], "unaligned prob")
    _close(Mv, ref[np.float64][1], ref[np.float32][1], "unaligned mix")
    Gh, Ghb = _offset(np.full((B, n_slots * S), 7.0))
    _, dl = ops.mtl_mix_bwd(mix, Hv, prob, Dv, True, dH=Gh)
    pn = prob.cpu().numpy()
    refb = {dt: R.mix_bwd(H, pn, dmix, S, n_slots, sl, True, dtype=dt) for dt in (np.float64, np.float32)}
    assert _offset_intact(Ghb)
    _close(Gh, refb[np.float64][0], refb[np.float32][0], "unaligned dH")
    _close(dl, refb[np.float64][1], refb[np.float32][1], "unaligned dlogits")
    # the aligned (float4) form computes the same chains: bit-identical
    prob4, mix4 = ops.mtl_mix_fwd(mix, torch.as_tensor(H).to(DEV), Lv)
    assert torch.equal(prob4, prob) and torch.equal(mix4, Mv)


@pytest.mark.parametrize("B,T,pad", [(1, 1, 0), (5, 2, 0), (257, 3, 0), (64, 2, 3)])
def test_head_kernel(engine_lib, B, T, pad):
    from paddlerec_amd import ops
    rng = np.random.default_rng(B + T)
    logits = (3 * rng.standard_normal((B, 2 * T))).astype(np.float32)
    label = rng.integers(0, 2, (B, T)).astype(np.float32)
    logits[0, :2] = (40.0, -40.0)                         # p1 below 1e-15: clipped, no gradient
    label[0, 0] = 1.0
    if B > 1:
        logits[1, :2] = (-40.0, 40.0)                     # p1 = 1 in float32: the upper bound, gradient passes (and is 0)
        label[1, 0] = 0.0
        logits[2, :2] = (36.0, -36.0)
        label[2, 0] = 0.0
    Lv, _ = _padded(logits, pad)
    Yv, _ = _padded(label, pad)
    for scale in (1.0, 1.0 / B):
        ref = {dt: R.head(logits, label, scale, dtype=dt) for dt in (np.float64, np.float32)}
        a, b = ops.mtl_head(Lv, Yv, scale), ops.mtl_head(Lv, Yv, scale)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        for i, what in enumerate(("pred", "cost", "dlogits")):
            _close(a[i], ref[np.float64][i], ref[np.float32][i], "head B%d T%d %s" % (B, T, what))
        assert float(a[0][0, 1]) == float(np.float32(1e-15)) and float(a[2][0, 1]) == 0.0 and float(a[2][0, 0]) == 0.0
        if B > 1:
            assert float(a[0][1, 1]) == 1.0
        assert bool((a[2][:, 0::2] == -a[2][:, 1::2]).all())                  # d z0 = -d z1 exactly
    pred, cost, none = ops.mtl_head(Lv, Yv, 1.0, want_grad=False)              # dlogits = NULL
    assert none is None and torch.equal(pred, a[0]) and torch.equal(cost, ops.mtl_head(Lv, Yv, 1.0)[1])


def test_refusals_return_before_any_launch(engine_lib):
    K.run_refusals(engine_lib)
    torch.cuda.synchronize()


class _CountingOps:
    """paddlerec_amd.ops with gemm() counted."""

    def __init__(self):
        from paddlerec_amd import ops
        self._ops, self.gemms = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name != "gemm":
            return fn

        def gemm(A, B, *a, **kw):
            self.gemms.append((tuple(A.shape), tuple(B.shape)))
            return fn(A, B, *a, **kw)

        return gemm


@pytest.mark.parametrize("name", ["mmoe_init.npz", "mmoe_rand.npz", "ple_init.npz", "ple_rand_l1.npz", "ple_rand_l2.npz"])
def test_one_train_step_on_every_golden(engine_lib, name):
    G = K.gold(name)
    k = _CountingOps()
    m = K.layer_of(G, DEV, k)
    m.set_dict(G["p"])
    x = torch.as_tensor(G["g"]["x_0"]).to(DEV)
    preds = m.forward(x)
    images = [im["img"] for lev in m.levels for im in lev["images"]]
    assert len(k.gemms) == len(images) + 2 * m.tasks                       # one GEMM per image, two per tower
    assert [g[1] for g in k.gemms[:len(images)]] == [(im.K, im.N) for im in images]
    e = R.relerr(torch.cat(preds, 1).cpu().numpy(), G["r64"][0]["pred"])
    assert e <= K.bound_of(G["r32"][0]["pred"], G["r64"][0]["pred"]), e
    K.check_layer(G, m, "gpu " + name, steps=1)
    # bit-identical on a rerun from the same state
    m2 = K.layer_of(G, DEV, None)
    m2.set_dict(G["p"])
    y = torch.as_tensor(G["g"]["label_0"]).to(DEV)
    m2.train_step(x, y, G["lr"])
    for key, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[key]), key


@pytest.mark.parametrize("model", ["mmoe", "ple"])
def test_trainer_on_the_gpu_matches_the_cpu_kernel_run(engine_lib, tmp_path, model):
    from paddlerec_amd import trainer
    from paddlerec_amd.deepfm import auc_from_buckets
    from paddlerec_amd.din import NUM_THRESHOLDS
    runs = {}
    for dev, kern in (("cuda", None), ("cpu", mtl_cpu_kernels)):
        d = tmp_path / dev
        d.mkdir()
        cfg = K.census_config(d, model)
        out, m = trainer.train(cfg, model, device=dev, kernels=kern)
        res = trainer.infer(cfg, model, device=dev, kernels=kern)
        assert len(out) == 2 and out[1]["batches"] == 4 and [r["epoch"] for r in res] == [0, 1]
        dm = trainer._dygraph_model(model)
        metrics, names = dm.create_metrics(dev)
        preds = []
        for batch in trainer.create_data_loader(cfg, model, dev, "test")():
            dm.infer_forward(m, metrics, batch, cfg)
            preds.append(m.predict(batch[0]).cpu().numpy())
        runs[dev] = dict(metrics=[(a.cpu(), b.cpu()) for a, b in metrics], preds=np.concatenate(preds), infer=res[1], names=names)
    g, c = runs["cuda"], runs["cpu"]
    assert g["names"] == ["auc_income", "auc_marital"]
    # a bucket is int(pred * num_thresholds): it cannot move while the prediction stays clear of a bucket edge by more
    # than the two float32 trainings can differ (1e-3 of a bucket is 2.4e-7 in the prediction, above their rounding only
    # for unsaturated predictions; the census net saturates, so expect the AUC branch for it)
    err = np.abs(g["preds"] - c["preds"]).max()
    for t, n in enumerate(g["names"]):
        pos = c["preds"][:, 2 * t + 1].astype(np.float64) * NUM_THRESHOLDS
        clear = np.minimum(pos - np.floor(pos), np.ceil(pos) - pos).min() > max(2 * err * NUM_THRESHOLDS, 1e-3)
        if clear:
            print("%s %s: integer buckets compared exactly (max prediction difference %.3g)" % (model, n, err))
            assert torch.equal(g["metrics"][t][0], c["metrics"][t][0]) and torch.equal(g["metrics"][t][1], c["metrics"][t][1])
        else:
            print("%s %s: a prediction sits within %.3g of a bucket edge: AUC compared within 1e-6" % (model, n, err))
        a, b = auc_from_buckets(*g["metrics"][t]), auc_from_buckets(*c["metrics"][t])
        assert abs(a - b) <= 1e-6 and abs(g["infer"][n] - c["infer"][n]) <= 1e-6, (n, a, b)
