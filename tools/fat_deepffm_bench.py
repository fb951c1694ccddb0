#!/usr/bin/env python3
"""FAT-DeepFFM (paddlerec_amd/fat_deepffm.py, csrc/fatffm_ops.hip) at the reference's shape: S 26 sparse slots, Dn 13 dense
values, D 10 (F 39, rows of 390 floats kept at a stride of 392), the [1600, 1600] tower over the 7410 pair features, the
table of 1 000 001 rows.  Prints ONE JSON line; at batch B (default 8192: H alone is 29.6 KB per sample, 243 MB):
  * the four kernels against an eager torch composition of the same arithmetic on the same GPU, which materialises the
    B x F x F x D cube (60 KB per sample): gather + dense rows + max for pool_fwd, + the scaled cube, the pair products and
    the sum for inter_fwd, and ONE autograd backward of that graph (built once, backward timed) for attn_bwd + bwd
    together; HIP events around back-to-back calls, median of the rounds, the candidates alternating round by round;
  * each kernel's minimal traffic — the gathered rows (ids 8 B, the row 4 R per sparse field) plus a / dH read and pooled
    / H / d_a / row_grad written — and the share of 8 TB/s it takes in the measured time;
  * ms per train step (FAT_DeepFFMLayer.train_step, lazy and non-lazy Adam) and the share of it spent in the tower's
    GEMMs (the same eight ops.gemm calls timed alone on the step's own buffers' shapes);
  * pool_fwd's time again as `argmax_pass_upper_bound_ms`: the backward's argmax pre-pass scans the staged cube as
    pool_fwd does, minus the gather and the staging it shares with the rest of the backward — an upper bound of what one
    pass plus a stored argmax could save, before the index tensor's own traffic (B x F*F bytes each way).

    python tools/fat_deepffm_bench.py [--batch 8192] [--steps 10] [--warmup 3]

Not part of bench.py: the project's flagship measurement stays as it is.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

N, S, DN, D = 1000001, 26, 13, 10
FC = [1600, 1600]
F = S + DN
R, F2, NP = F * D, F * F, F * (F - 1) // 2
PD = NP * D
PEAK = 8e12


def _once(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(fns, reps=5, rounds=5):
    """{name: fn} -> {name: median ms}; one round times every fn once, so the candidates see the same machine state."""
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(_once(fn, reps))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from paddlerec_amd import ops
    from paddlerec_amd.fat_deepffm import FAT_DeepFFMLayer
    dev, B = "cuda", args.batch
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = FAT_DeepFFMLayer(N, D, DN, S, FC, device=dev, dropout_rate=0.5, l2_dnn=1e-7)
    m.emb_table.mul_(2.0)                      # the factors of tests/test_fat_deepffm_gpu.py: an unsaturated logit, so the
    m.dense.p["cen.dense_w"].mul_(0.02)        # step's gradients are live (timing does not depend on it)
    out = {"model": "fat_deepffm", "batch": B, "device": torch.cuda.get_device_name(0),
           "shape": {"N": N, "S": S, "Dn": DN, "D": D, "F": F, "row_stride": m.row_pad, "fc": FC, "ld_attn": m.ld_attn,
                     "ld_pair": m.ld_pair}, "step_ms": {}}
    f32 = dict(dtype=torch.float32, device=dev)
    ids = torch.as_tensor(rng.integers(0, N, (B, S), dtype=np.int64), device=dev)
    dense = torch.as_tensor(rng.random((B, DN), dtype=np.float32), device=dev)
    label = torch.as_tensor((rng.random((B, 1)) < 0.25).astype(np.int64), device=dev)
    for lazy in (False, True):
        m.lazy_mode = lazy
        for _ in range(args.warmup):
            m.train_step(ids, dense, label, lr=1e-4)
        torch.cuda.synchronize()
        ms = _alternate({"step": lambda: m.train_step(ids, dense, label, lr=1e-4)}, reps=args.steps, rounds=3)["step"]
        out["step_ms"]["lazy" if lazy else "nonlazy"] = round(ms, 4)
    # the tower's GEMMs alone: forward, dW and dX of every layer at the step's shapes
    ws = ops.Workspace(dev)
    W, b, dW, db = m._linears("dnn.linear_%d", len(FC) + 1)
    sizes = [PD] + FC + [1]
    xs = [torch.randn(B, m.ld_pair, **f32)[:, :PD]] + [torch.relu(torch.randn(B, n, **f32)) for n in FC]
    gs = [torch.randn(B, n, **f32) for n in sizes[1:]]
    dH = torch.empty(B, m.ld_pair, **f32)[:, :PD]

    def tower():
        for i in range(len(sizes) - 1):
            ops.gemm(xs[i], W[i], ws, epilogue="bias" if i == len(FC) else "bias_relu", bias=b[i])
            ops.gemm(xs[i], gs[i], ws, trans_a=True, out=dW[i], b_colsum=db[i])
            if i:
                ops.gemm(gs[i], W[i], ws, trans_b=True, epilogue="relu_mask", aux0=xs[i])
            else:
                ops.gemm(gs[0], W[0], ws, trans_b=True, out=dH)
    tower()
    torch.cuda.synchronize()
    t_tower = _alternate({"tower": tower}, reps=args.steps, rounds=3)["tower"]
    out["tower_gemms_ms"] = round(t_tower, 4)
    out["tower_gemms_share_of_step"] = {k: round(t_tower / v, 3) for k, v in out["step_ms"].items()}
    # the four kernels against eager torch
    status = ops.new_status(dev)
    tab, dw = m.emb_table, m.dense.p["cen.dense_w"]
    mat = lambda cols, ld: torch.randn(B, ld, **f32)[:, :cols]
    pooled, a, d_a, d_pooled = (mat(F2, m.ld_attn) for _ in range(4))
    a.copy_(torch.relu(a))
    H = mat(PD, m.ld_pair)
    dH.normal_()
    dz = torch.randn(B, 1, **f32)
    rg = torch.empty(B * S, m.row_pad, **f32)
    ddw = torch.empty(DN, R, **f32)
    wsb = ops.Workspace(dev)
    iu, ju = (torch.as_tensor(x, device=dev) for x in np.triu_indices(F, 1))

    def cube():
        return torch.cat([tab[ids][:, :, :R], dense[:, :, None] * dw.view(1, DN, R)], 1).view(B, F, F, D)

    def eager_inter():
        A = cube() * a.reshape(B, F, F, 1)
        return (A[:, iu, ju] * A[:, ju, iu]).reshape(B, PD), A.sum((1, 2, 3))

    E_leaf = cube().detach().requires_grad_(True)
    a_leaf = a.detach().clone().requires_grad_(True)
    A_g = E_leaf * a_leaf.view(B, F, F, 1)
    graph = ((A_g[:, iu, ju] * A_g[:, ju, iu]).reshape(B, PD), A_g.sum((1, 2, 3)), E_leaf.max(dim=3).values.reshape(B, F2))
    gouts = (dH.contiguous(), dz.reshape(B), d_pooled.contiguous())
    cands = {
        "pool_fwd": lambda: ops.fatffm_pool_fwd(ids, dense, tab, dw, D, status, out=pooled),
        "eager_pool_fwd": lambda: cube().amax(3),
        "inter_fwd": lambda: ops.fatffm_inter_fwd(ids, dense, tab, dw, a, D, status, out=(H, None)),
        "eager_inter_fwd": eager_inter,
        "attn_bwd": lambda: ops.fatffm_attn_bwd(ids, dense, tab, dw, a, dH, dz, D, status, out=d_a),
        "bwd": lambda: ops.fatffm_bwd(ids, dense, tab, dw, a, dH, dz, d_pooled, D, wsb, out=(rg, ddw), status=status),
        "eager_autograd_bwd": lambda: torch.autograd.grad(graph, (E_leaf, a_leaf), gouts, retain_graph=True),
    }
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    tm = _alternate(cands)
    rows = B * S * (8 + 4 * R) + B * DN * 4            # ids + the gathered rows + the dense values
    nbytes = {"pool_fwd": rows + B * F2 * 4, "inter_fwd": rows + B * (F2 + PD + 1) * 4,
              "attn_bwd": rows + B * (F2 + PD + 1 + F2) * 4,
              "bwd": rows + B * (2 * F2 + PD + 1) * 4 + B * S * m.row_pad * 4}
    out["kernels"] = {
        "ms": {k: round(v, 4) for k, v in tm.items()}, "min_bytes": nbytes,
        "frac_8TBs": {k: round(nbytes[k] / (tm[k] * 1e-3) / PEAK, 3) for k in nbytes},
        "eager_over_kernel": {"pool_fwd": round(tm["eager_pool_fwd"] / tm["pool_fwd"], 2),
                              "inter_fwd": round(tm["eager_inter_fwd"] / tm["inter_fwd"], 2),
                              "attn_bwd_plus_bwd": round(tm["eager_autograd_bwd"] / (tm["attn_bwd"] + tm["bwd"]), 2)},
        "argmax_pass_upper_bound_ms": round(tm["pool_fwd"], 4),
        "argmax_index_bytes_each_way": B * F2}
    ops.raise_on_status(m.status, "fat_deepffm_bench")
    ops.raise_on_status(status, "fat_deepffm_bench")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
