#!/usr/bin/env python3
"""FLEN (paddlerec_amd/flen.py, csrc/flen_ops.hip) at the reference's shape: S 22 lookups in the groups (13, 3, 6), D 32
(one 128-byte line per row), the table of 2 500 000 rows.  Prints ONE JSON line; at B 512 (the reference's batch) and
B 65 536:
  * rec_flen_fwd against the composition the engine offered before — rec_emb_gather into the [B, S*D] rows plus the
    field-wise bi-interaction as eager torch ops (three group sums, three pair products scaled by kernel_mf, their sum) —
    and rec_flen_bwd against the autograd backward of that eager interaction plus the add into dX0 (graph built once,
    backward timed);
  * rec_adagrad_rows against rec_sparse_adam_rows on the same grouping and gradient (segment partials included on both
    sides), and rec_adagrad_dense against rec_adam_dense on the layer's flat buffer and on 16 M floats;
  * ms per train step (FLENLayer.train_step, dropout 0.2).
Method: HIP events around `reps` back-to-back calls, after a warm-up; the candidates alternate round by round in one
process, so they see the same machine state; median of the rounds, with the spread (min .. max) printed beside it.  Bytes
come from the shapes (ids 8 B, a row 4 D read, X0 4 D written, FW and h_mf 4 D per group / sample, ...), and the share of
the 8 TB/s HBM peak they take in the median time.

    python tools/flen_bench.py [--reps 20] [--rounds 7] [--warmup 5]

Not part of bench.py: the project's flagship measurement stays as it is.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

N, S, D = 2500000, 22, 32
SIZES, TOWER = (13, 3, 6), [64, 32]
G = len(SIZES)
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
    from paddlerec_amd.flen import KMF, FLENLayer
    dev = "cuda"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = FLENLayer(N, D, S, G, TOWER, device=dev, dropout_rate=0.2)
    m._ensure_sparse_state()
    kmf = m.dense.p[KMF]
    gb = m.group_begin
    out = {"model": "flen", "shape": {"N": N, "S": S, "D": D, "groups": SIZES, "tower": TOWER},
           "device": torch.cuda.get_device_name(0), "method": {"reps": args.reps, "rounds": args.rounds,
                                                               "ms": "[median, min, max] over the rounds"},
           "step_ms": {}, "kernels": {}}
    f32 = dict(dtype=torch.float32, device=dev)
    M2 = torch.zeros_like(m.rec)[:, :D]                     # Adam's second table of moments
    for B in (512, 65536):
        ids23 = torch.as_tensor(rng.integers(0, N, (B, S + 1), dtype=np.int64), device=dev)
        label = torch.as_tensor((rng.random((B, 1)) < 0.25).astype(np.int64), device=dev)
        for _ in range(args.warmup):
            m.train_step(ids23, label, lr=0.04)
        torch.cuda.synchronize()
        out["step_ms"]["B%d" % B] = _alternate({"step": lambda: m.train_step(ids23, label, lr=0.04)}, args.reps, 3)["step"]
        ids = ids23[:, 1:].contiguous()
        ws, status = ops.Workspace(dev), ops.new_status(dev)
        x0, h, fw = torch.empty(B, S * D, **f32), torch.empty(B, D, **f32), torch.empty(B, G * D, **f32)
        dx0 = torch.randn(B, S * D, **f32) * 1e-3
        dh = torch.randn(B, D, **f32) * 1e-3
        dk = torch.empty(3, **f32)
        pairs = [(0, 1), (0, 2), (1, 2)]

        def interact(e):
            f = [e[:, gb[g]:gb[g + 1]].sum(dim=1) for g in range(G)]
            return sum(kmf[p] * f[i] * f[j] for p, (i, j) in enumerate(pairs))

        def eager_fwd():
            ops.emb_gather(ids.reshape(-1), m.embedding, None, status, out=x0, out_group=S, out_group_stride=S * D)
            return interact(x0.view(B, S, D))

        e_leaf = m.embedding[ids].detach().requires_grad_(True)
        k_leaf = kmf.detach().clone().requires_grad_(True)
        fl = [e_leaf[:, gb[g]:gb[g + 1]].sum(dim=1) for g in range(G)]
        h_graph = sum(k_leaf[p] * fl[i] * fl[j] for p, (i, j) in enumerate(pairs))

        def eager_bwd():
            de, dkk = torch.autograd.grad(h_graph, (e_leaf, k_leaf), dh, retain_graph=True)
            dx0.view(B, S, D).add_(de)
            return dkk

        groups, _ = ops.ids_group(ids, N, None, ws)
        grad = torch.randn(B, S * D, **f32) * 1e-3
        lay = dict(grad_group=S, grad_group_stride=S * D)
        st = m.sparse_state

        def adagrad_rows():
            pp = ops.segment_partials(groups, grad, D, **lay)
            ops.adagrad_rows(groups, grad, 1, m.embedding, st["m"], 0.04, 1e-6, partials=pp, **lay)

        def adam_rows():
            pp = ops.segment_partials(groups, grad, D, **lay)
            ops.sparse_adam_rows(groups, grad, 1, m.embedding, st["m"], M2, 1, 1e-3, partials=pp, **lay)

        d = m.dense
        big = [torch.randn(1 << 24, **f32) * 1e-3 for _ in range(2)] + [torch.full((1 << 24,), 1e-3, **f32) for _ in range(2)]
        cands = {
            "flen_fwd": lambda: ops.flen_fwd(ids, m.embedding, gb, kmf, status, out=(x0, h, fw)),
            "emb_gather_plus_eager_interaction": eager_fwd,
            "emb_gather_alone": lambda: ops.emb_gather(ids.reshape(-1), m.embedding, None, status, out=x0, out_group=S,
                                                       out_group_stride=S * D),
            "flen_bwd": lambda: ops.flen_bwd(ids, N, gb, kmf, fw, dh, dx0, ws, status, out=dk),
            "eager_interaction_autograd_bwd": eager_bwd,
            "adagrad_rows": adagrad_rows,
            "sparse_adam_rows": adam_rows,
            "adagrad_dense_layer": lambda: ops.adagrad_dense(d.data, d.m, d.grad, 0.04, 1e-6),
            "adam_dense_layer": lambda: ops.adam_dense(d.data, d.m, d.v, d.grad, 1, 1e-3),
            "adagrad_dense_16M": lambda: ops.adagrad_dense(big[0], big[2], big[1], 0.04, 1e-6),
            "adam_dense_16M": lambda: ops.adam_dense(big[0], big[2], big[3], big[1], 1, 1e-3),
        }
        for _ in range(args.warmup):
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        tm = _alternate(cands, args.reps, args.rounds)
        n, U = B * S, int(groups.n_uniq[0].item())
        nbytes = {"flen_fwd": n * (8 + 8 * D) + B * 4 * D * (G + 1),                 # ids, row read, X0 written; FW, h written
                  "flen_bwd": n * (8 + 8 * D) + B * 4 * D * (G + 1),                 # ids, dX0 read and written; FW, dH read
                  "adagrad_rows": n * (4 + 4 * D) + U * (8 + 16 * D),                # positions, gradient rows; P, acc read + written
                  "sparse_adam_rows": n * (4 + 4 * D) + U * (8 + 24 * D),
                  "adagrad_dense_16M": 5 * 4 * (1 << 24), "adam_dense_16M": 7 * 4 * (1 << 24)}
        med = {k: v[0] for k, v in tm.items()}
        out["kernels"]["B%d" % B] = {
            "ms": tm, "unique_rows": U, "bytes": nbytes,
            "frac_8TBs": {k: round(nbytes[k] / (med[k] * 1e-3) / PEAK, 4) for k in nbytes},
            "replaced_over_kernel": {
                "fwd": round(med["emb_gather_plus_eager_interaction"] / med["flen_fwd"], 2),
                "bwd": round(med["eager_interaction_autograd_bwd"] / med["flen_bwd"], 2),
                "adam_rows_over_adagrad_rows": round(med["sparse_adam_rows"] / med["adagrad_rows"], 2),
                "adam_dense_over_adagrad_dense_16M": round(med["adam_dense_16M"] / med["adagrad_dense_16M"], 2),
                "adam_dense_over_adagrad_dense_layer": round(med["adam_dense_layer"] / med["adagrad_dense_layer"], 2)}}
        del e_leaf, k_leaf, fl, h_graph, big
    ops.raise_on_status(m.status, "flen_bench")
    ops.raise_on_status(status, "flen_bench")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
