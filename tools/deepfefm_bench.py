#!/usr/bin/env python3
"""DeepFEFM (paddlerec_amd/deepfefm.py, csrc/fefm_ops.hip) at the reference's shapes: S 26 sparse slots, Dn 13 dense
fields (39 fields, 741 pairs), 1 100 005 table rows; D 9 with the [512, 256, 128, 32] tower (config.yaml) and D 48 with
[1024, 1024, 1024] (config_bigdata.yaml).  Prints ONE JSON line:
  * ms per train step (DeepFEFMLayer.train_step, dropout on) at B 4096 and 65 536 for D 9 and at B 5120 for D 48, lazy
    and non-lazy Adam, frozen and trained pair matrices;
  * rec_fefm_fwd / rec_fefm_bwd alone (HIP events around back-to-back calls, median of 5) with their algorithmic bytes
    and flops as fractions of 8 TB/s and of the 157 Tflop/s f32 rate;
  * the same forward + backward written in eager torch on the same GPU (tests/deepfefm_ref.kernel_reference's arithmetic
    on device tensors) — the only outside yardstick for a model the engine could not run before.

    python tools/deepfefm_bench.py [--steps 10] [--warmup 3] [--skip-d48]

Not part of bench.py: the project's flagship measurement stays as it is.
"""
import argparse
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

N, S, DN = 1100005, 26, 13
F = S + DN
P = F * (F - 1) // 2
PEAK_BW, PEAK_F32 = 8e12, 157e12


def _time(fn, reps=10, rounds=5):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts))


def _batch(B, rng, dev):
    ids = torch.as_tensor(rng.integers(1, 1000000, (B, S), dtype=np.int64), device=dev)
    dense = torch.as_tensor(rng.random((B, DN), dtype=np.float32), device=dev)
    label = torch.as_tensor((rng.random((B, 1)) < 0.25).astype(np.int64), device=dev)
    return ids, dense, label


def _eager(ids_all, dense, W, W1, w1, FE, dz, dd, D, pi, pj):
    """Forward + backward of the interaction in eager torch (autograd), on the device: one batched matmul over the P
    pair matrices ([P, B, D] x [P, D, D]) and an elementwise product-sum with x_j.  (Not one three-operand einsum: torch
    lowers its second contraction to a batched 1 x D x 1 matmul with B * P = millions of batches.)"""
    live = (ids_all != 0).to(torch.float32)
    x = (W[ids_all, :D] * live[..., None]).requires_grad_(True)
    w = w1.detach().clone().requires_grad_(True)
    fe = FE.detach().clone().requires_grad_(True)
    d1 = dense * w
    y1 = (W1.reshape(-1)[ids_all[:, :S]] * live[:, :S]).sum(1) + d1.sum(1)
    u = torch.bmm(x[:, pi].transpose(0, 1), fe + fe.transpose(1, 2)).transpose(0, 1)       # [B, P, D]
    t = (u * x[:, pj]).sum(-1)
    dnn_in = torch.cat([x[:, :S].reshape(len(x), S * D), d1, t], dim=1)
    (((y1 + t.sum(1)) * dz).sum() + (dnn_in * dd).sum()).backward()
    return x.grad, w.grad, fe.grad


def run_shape(out, D, fc, batches, args, rng, dev):
    from paddlerec_amd import ops
    from paddlerec_amd.deepfefm import DeepFEFMLayer
    key = "D%d" % D
    out["step_ms"][key], out["kernels"][key] = {}, {}
    for tfe in (False, True):
        m = DeepFEFMLayer(N, D, DN, S, fc, device=dev, dropout_rate=0.2, train_field_embeddings=tfe)
        for B in batches:
            ids, dense, label = _batch(B, rng, dev)
            for lazy in (True, False):
                m.lazy_mode = lazy
                for _ in range(args.warmup):
                    m.train_step(ids, dense, label, lr=1e-3)
                torch.cuda.synchronize()
                ms = _time(lambda: m.train_step(ids, dense, label, lr=1e-3), reps=args.steps, rounds=3)
                out["step_ms"][key]["B%d_%s_%s" % (B, "lazy" if lazy else "nonlazy", "trainedFE" if tfe else "frozenFE")] = \
                    round(ms, 4)
        print("step_ms %s: %s" % (key, json.dumps(out["step_ms"][key])), file=sys.stderr, flush=True)
        ops.raise_on_status(m.status, "deepfefm_bench")
        if tfe:
            break
        fe = m.dense.p["fefm.field_embeddings"]
        w1 = m.dense.p["fefm.dense_w_one"]
        pr = np.asarray(list(itertools.combinations(range(F), 2)), np.int64)
        pi, pj = torch.as_tensor(pr[:, 0], device=dev), torch.as_tensor(pr[:, 1], device=dev)
        for B in batches:
            ids, dense, _ = _batch(B, rng, dev)
            ws = ops.Workspace(dev)
            dz = torch.randn(B, device=dev) * 1e-3
            dd = torch.randn(B, m.input_size, device=dev) * 1e-3
            fo = ops.fefm_fwd(ids, dense, m.emb_table, m.embedding_one, w1, fe, D, ws, status=m.status)
            ids_all = fo[3]
            call_f = lambda: ops.fefm_fwd(ids, dense, m.emb_table, m.embedding_one, w1, fe, D, ws, status=m.status, out=fo[:4])
            res = {}
            for name, want in (("bwd", False), ("bwd_dFE", True)):
                bo = ops.fefm_bwd(ids_all, dense, m.emb_table, fe, dz, dd, S, D, ws, want_d_fe=want, status=m.status)
                res[name] = _time(lambda: ops.fefm_bwd(ids_all, dense, m.emb_table, fe, dz, dd, S, D, ws, want_d_fe=want,
                                                       out=bo, status=m.status))
            t_f = _time(call_f)
            Dp = m.row_pad
            rows = B * F * Dp * 4                                            # the F gathered rows of a sample
            fe_bytes = P * D * D * 4
            fwd_bytes = rows + B * S * 8 + B * DN * 4 + B * S * 4 + fe_bytes + B * m.input_size * 4 + B * F * 8 + 2 * B * 4
            bwd_bytes = rows + B * F * 8 + B * DN * 4 + fe_bytes + B * 4 + B * m.input_size * 4 + B * F * Dp * 4
            fwd_flops = B * P * (2 * D * D + 2 * D)
            bwd_flops = 2 * fwd_flops
            k = {"fwd_ms": round(t_f, 4), "bwd_ms": round(res["bwd"], 4), "bwd_with_dFE_ms": round(res["bwd_dFE"], 4),
                 "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes, "fwd_flops": fwd_flops, "bwd_flops": bwd_flops,
                 "fwd_frac_8TBs": round(fwd_bytes / (t_f * 1e-3) / PEAK_BW, 4),
                 "bwd_frac_8TBs": round(bwd_bytes / (res["bwd"] * 1e-3) / PEAK_BW, 4),
                 "fwd_frac_f32": round(fwd_flops / (t_f * 1e-3) / PEAK_F32, 4),
                 "bwd_frac_f32": round(bwd_flops / (res["bwd"] * 1e-3) / PEAK_F32, 4)}
            print("kernels %s B%d: %s" % (key, B, json.dumps(k)), file=sys.stderr, flush=True)
            if B * P * D * 4 < 1e9:                                          # the eager form materialises [B, P, D] several times
                _eager(ids_all, dense, m.emb_table, m.embedding_one, w1, fe, dz, dd, D, pi, pj)
                k["eager_torch_fwd_bwd_ms"] = round(_time(lambda: _eager(ids_all, dense, m.emb_table, m.embedding_one, w1,
                                                                         fe, dz, dd, D, pi, pj), reps=3, rounds=3), 4)
                k["eager_over_kernels"] = round(k["eager_torch_fwd_bwd_ms"] / (t_f + res["bwd_dFE"]), 2)
            out["kernels"][key]["B%d" % B] = k
        del m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-d48", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    out = {"model": "deepfefm", "shape": {"N": N, "S": S, "Dn": DN, "fields": F, "pairs": P},
           "device": torch.cuda.get_device_name(0), "step_ms": {}, "kernels": {}}
    run_shape(out, 9, [512, 256, 128, 32], (4096, 65536), args, rng, dev)
    if not args.skip_d48:
        run_shape(out, 48, [1024, 1024, 1024], (5120,), args, rng, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
