#!/usr/bin/env python3
"""AutoFIS (paddlerec_amd/autofis.py, csrc/autofis_ops.hip) at the reference's shape: S 39 fields, D 40, all P 741 pairs,
the tables of 1 178 909 rows.  Prints ONE JSON line; at B 2000 (the reference's batch) and B 65 536:
  * autofis_fwd (training) and autofis_bwd against the chain the engine offered before, out of existing ops only:
    forward  emb_gather (v rows into [B, S, D]) -> dot_interact_fwd -> batchnorm_fwd on its [B, P] block -> the GEMV
             gemm(Y, mask); the first-order sum of the w lookups is left out of the chain (in its favour);
    backward gemm(dz, mask^T) -> batchnorm_bwd -> dot_interact_bwd -> the add onto dX0 (torch add_), d_mask by
             gemm(Y^T, dz);
  * batchnorm_relu_fwd / _bwd against batchnorm_fwd + an in-place eager ReLU and relu_mask_ + batchnorm_bwd at [B, 700];
  * grda_step on 741 floats, and ms per train step (AutoDeepFMLayer.train_step, stage 0, width 700, depth 5).
Method: HIP events around `reps` back-to-back calls, after a warm-up; the candidates alternate round by round in one
process, so they see the same machine state; median of the rounds, with the spread (min .. max) printed beside it.  Bytes
come from the shapes (forward: ids 8 B, a v row 4 D and a w float read per lookup, X0 4 S D and L 4 P written per sample,
L read once more by the row pass; backward: L read twice, X0 read, dX0 read and written), and the share of the 8 TB/s HBM
peak they take in the median time.

    python tools/autofis_bench.py [--reps 20] [--rounds 7] [--warmup 5]

Not part of bench.py: the project's flagship measurement stays as it is.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

N, S, D, WIDTH, DEPTH = 1178909, 39, 40, 700, 5
P = S * (S - 1) // 2
PEAK = 8e12


def _once(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(fns, reps, rounds):
    """{name: fn} -> {name: [median, min, max] ms}; one round times every fn once."""
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(_once(fn, reps))
    return {k: [round(float(np.median(v)), 5), round(float(min(v)), 5), round(float(max(v)), 5)] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from paddlerec_amd import ops
    from paddlerec_amd.autofis import BN2, MASK, AutoDeepFMLayer
    dev = "cuda"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = AutoDeepFMLayer(S, N, D, WIDTH, DEPTH, P, 0, device=dev)
    p, bf = m.dense.p, m.buffers
    gamma, beta, mask = p[BN2 + ".weight"], p[BN2 + ".bias"], p[MASK].view(-1)
    out = {"model": "autofis", "shape": {"N": N, "S": S, "D": D, "P": P, "width": WIDTH, "depth": DEPTH},
           "device": torch.cuda.get_device_name(0), "method": {"reps": args.reps, "rounds": args.rounds,
                                                               "ms": "[median, min, max] over the rounds"},
           "step_ms": {}, "kernels": {}}
    f32 = dict(dtype=torch.float32, device=dev)
    for B in (2000, 65536):
        ids = torch.as_tensor(rng.integers(0, N, (B, S), dtype=np.int64), device=dev)
        label = torch.as_tensor((rng.random(B) < 0.25).astype(np.int64), device=dev)
        for _ in range(args.warmup):
            m.train_step(ids, label, lr=1e-3)
        torch.cuda.synchronize()
        out["step_ms"]["B%d" % B] = _alternate({"step": lambda: m.train_step(ids, label, lr=1e-3)}, args.reps, 3)["step"]
        ws, ws2, status = ops.Workspace(dev), ops.Workspace(dev), ops.new_status(dev)
        x0, L = torch.empty(B, S * D, **f32), torch.empty(B, P, **f32)
        rm, rv = bf[BN2 + "._mean"].clone(), bf[BN2 + "._variance"].clone()
        dz = torch.randn(B, 1, **f32) / B
        dx0 = torch.randn(B, S * D, **f32) * 1e-3
        dgr = (torch.empty(P, **f32), torch.empty(P, **f32), torch.empty(P, **f32))
        _, s, _, sm, si, _ = ops.autofis_fwd(ids, m.v_embeddings, m.w_embeddings, m.pairs, gamma, beta, mask, rm, rv, ws,
                                             True, status=status, out=(x0, L))
        # the composed chain
        T = torch.empty(B, S, D, **f32)
        R = torch.empty(B, D + P, **f32)
        Y = torch.empty(B, P, **f32)
        dR = torch.zeros(B, D + P, **f32)
        dT = torch.empty(B, S, D, **f32)
        maskc, dmask = mask.reshape(P, 1), torch.empty(P, 1, **f32)
        saved = {}

        def chain_fwd():
            ops.emb_gather(ids.reshape(-1), m.v_embeddings, None, status, out=T)
            ops.dot_interact_fwd(T, out=R)
            _, saved["m"], saved["i"] = ops.batchnorm_fwd(R[:, D:], gamma, beta, rm, rv, ws2, True, out=Y)
            return ops.gemm(Y, maskc, ws2)

        def chain_bwd():
            ops.gemm(Y, dz, ws2, trans_a=True, out=dmask)
            dY = ops.gemm(dz, maskc, ws2, trans_b=True)
            ops.batchnorm_bwd(R[:, D:], dY, gamma, saved["m"], saved["i"], ws2, out=dR[:, D:])
            ops.dot_interact_bwd(T, dR, out=dT)
            dx0.add_(dT.view(B, S * D))

        X = torch.randn(B, WIDTH, **f32)
        dYb = torch.randn(B, WIDTH, **f32)
        Yb, dXb = torch.empty(B, WIDTH, **f32), torch.empty(B, WIDTH, **f32)
        g1, b1 = torch.ones(WIDTH, **f32), torch.zeros(WIDTH, **f32)
        r1, r2 = torch.zeros(WIDTH, **f32), torch.ones(WIDTH, **f32)
        _, bm, bi = ops.batchnorm_relu_fwd(X, g1, b1, r1, r2, ws2, True, out=Yb)
        dYc = dYb.clone()

        def bn_then_relu():
            ops.batchnorm_fwd(X, g1, b1, r1, r2, ws2, True, out=Yb)
            torch.relu_(Yb)                              # relu_mask_ needs a second buffer: the eager ReLU is the cheaper rival

        def relu_then_bn_bwd():
            ops.relu_mask_(dYc, Yb)
            ops.batchnorm_bwd(X, dYc, g1, bm, bi, ws2, out=dXb)

        acc, gg = torch.zeros(P, **f32), torch.zeros(P, **f32)
        cands = {
            "autofis_fwd": lambda: ops.autofis_fwd(ids, m.v_embeddings, m.w_embeddings, m.pairs, gamma, beta, mask, rm, rv,
                                                   ws, True, status=status, out=(x0, L)),
            "chain_fwd": chain_fwd,
            "autofis_bwd": lambda: ops.autofis_bwd(dz, L, x0, m.pairs, sm, si, gamma, beta, mask, dx0, ws, out=dgr),
            "chain_bwd": chain_bwd,
            "autofis_fwd_eval": lambda: ops.autofis_fwd(ids, m.v_embeddings, m.w_embeddings, m.pairs, gamma, beta, mask, rm,
                                                        rv, ws, False, status=status, out=(x0, None)),
            "batchnorm_relu_fwd": lambda: ops.batchnorm_relu_fwd(X, g1, b1, r1, r2, ws2, True, out=Yb),
            "batchnorm_fwd_plus_relu": bn_then_relu,
            "batchnorm_relu_bwd": lambda: ops.batchnorm_relu_bwd(X, Yb, dYb, g1, bm, bi, ws2, out=dXb),
            "relu_mask_plus_batchnorm_bwd": relu_then_bn_bwd,
            "grda_step": lambda: ops.grda_step(mask.clone(), acc, gg, 1.0, 0.01, 0),
        }
        for _ in range(args.warmup):
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        tm = _alternate(cands, args.reps, args.rounds)
        n = B * S
        nbytes = {"autofis_fwd": n * (8 + 4 * D + 4 + 4 * D) + B * 4 * P * 2,
                  "autofis_bwd": B * 4 * P * 2 + n * 4 * D * 3,
                  "batchnorm_relu_fwd": B * WIDTH * 4 * 4, "batchnorm_relu_bwd": B * WIDTH * 4 * 8}
        med = {k: v[0] for k, v in tm.items()}
        out["kernels"]["B%d" % B] = {
            "ms": tm, "bytes": nbytes,
            "frac_8TBs": {k: round(nbytes[k] / (med[k] * 1e-3) / PEAK, 4) for k in nbytes},
            "chain_over_fused": {"fwd": round(med["chain_fwd"] / med["autofis_fwd"], 2),
                                 "bwd": round(med["chain_bwd"] / med["autofis_bwd"], 2),
                                 "bn_relu_fwd": round(med["batchnorm_fwd_plus_relu"] / med["batchnorm_relu_fwd"], 2),
                                 "bn_relu_bwd": round(med["relu_mask_plus_batchnorm_bwd"] / med["batchnorm_relu_bwd"], 2)}}
        del T, R, Y, dR, dT, X, dYb, Yb, dXb, dYc
    ops.raise_on_status(m.status, "autofis_bench")
    ops.raise_on_status(status, "autofis_bench")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
