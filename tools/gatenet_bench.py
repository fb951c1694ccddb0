#!/usr/bin/env python3
"""GateNet (paddlerec_amd/gatenet.py, csrc/gate_ops.hip) at the reference's shape: S 26 sparse slots, D 9, Dn 13 raw dense
values (feature rows of 247 floats kept at a stride of 248), the [512, 256, 128, 32] tower with both gates, the table of
1 000 001 rows (record lines of 32 floats).  Prints ONE JSON line; at B 65536 and B 512:
  * rec_gate_emb_fwd against what it replaces — rec_emb_gather into a [B*S, D] tensor plus the gate as eager torch ops
    (sum, multiply by the field's scalar, sigmoid, multiply into the feature rows) — and rec_gate_emb_bwd against the
    autograd backward of that eager gate (graph built once, backward timed); HIP events around back-to-back calls, median
    of the rounds, the candidates alternating round by round;
  * rec_gate_hidden_fwd / rec_gate_hidden_bwd at n 512 against the same arithmetic as eager torch ops;
  * the lookups' bytes per lookup from the shapes (ids 8 B, the row 4 D, the slot read and / or written 4 D each; and the
    same with the whole 128-byte record line counted for the row) and the share of 8 TB/s they take in the measured time;
  * ms per train step (GateDNNLayer.train_step), non-lazy (the dygraph default) and lazy Adam.

    python tools/gatenet_bench.py [--steps 20] [--warmup 5]

Not part of bench.py: the project's flagship measurement stays as it is.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

N, S, DN, D = 1000001, 26, 13, 9
FC = [512, 256, 128, 32]
WIDTH = S * D + DN
LD = (WIDTH + 3) // 4 * 4
LINE = 128                    # bytes of a record line (32 floats)
PEAK = 8e12


def _once(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(fns, reps=20, rounds=5):
    """{name: fn} -> {name: median ms}; one round times every fn once, so the candidates see the same machine state."""
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(_once(fn, reps))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from paddlerec_amd import ops
    from paddlerec_amd.gatenet import GATE_VEC, GateDNNLayer
    dev = "cuda"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = GateDNNLayer(N, D, DN, S, FC, True, True, device=dev)
    gw = m.dense.p[GATE_VEC]
    out = {"model": "gatenet", "shape": {"N": N, "S": S, "Dn": DN, "D": D, "row_stride": LD, "fc": FC},
           "device": torch.cuda.get_device_name(0), "step_ms": {}, "kernels": {}}
    f32 = dict(dtype=torch.float32, device=dev)
    for B in (65536, 512):
        ids = torch.as_tensor(rng.integers(0, N, (B, S), dtype=np.int64), device=dev)
        dense = torch.as_tensor(rng.random((B, DN), dtype=np.float32), device=dev)
        label = torch.as_tensor((rng.random((B, 1)) < 0.25).astype(np.int64), device=dev)
        for lazy in (False, True):
            m.lazy_mode = lazy
            for _ in range(args.warmup):
                m.train_step(ids, dense, label, lr=1e-4)
            torch.cuda.synchronize()
            ms = _alternate({"step": lambda: m.train_step(ids, dense, label, lr=1e-4)}, reps=args.steps, rounds=3)["step"]
            out["step_ms"]["B%d_%s" % (B, "lazy" if lazy else "nonlazy")] = round(ms, 4)
        ws = ops.Workspace(dev)
        status = ops.new_status(dev)
        buf = torch.zeros(B, LD, **f32)
        slots = torch.as_strided(buf, (B, S, D), (LD, D, 1))
        gbuf = torch.randn(B, LD, **f32) * 1e-3
        dwv = torch.empty(S, **f32)
        flat = torch.empty(B * S, D, **f32)
        w3 = gw.view(1, S, 1)

        def eager_fwd():
            ops.emb_gather(ids.reshape(-1), m.embedding, None, status, out=flat)
            e = flat.view(B, S, D)
            torch.mul(e, torch.sigmoid(e.sum(dim=2, keepdim=True) * w3), out=slots)

        e_leaf = m.embedding[ids].detach().requires_grad_(True)
        w_leaf = gw.detach().clone().requires_grad_(True)
        o_graph = e_leaf * torch.sigmoid(e_leaf.sum(dim=2, keepdim=True) * w_leaf.view(1, S, 1))
        g3 = torch.as_strided(gbuf, (B, S, D), (LD, D, 1)).contiguous()
        n512 = FC[0]
        y = torch.relu(torch.randn(B, n512, **f32))
        t0 = torch.randn(B, n512, **f32)
        t = t0.clone()
        u = torch.randn(B, n512, **f32)
        x, dt, uh = torch.empty(B, n512, **f32), torch.empty(B, n512, **f32), torch.empty(B, n512, **f32)
        h = torch.tanh(t0)
        cands = {
            "gate_emb_fwd": lambda: ops.gate_emb_fwd(ids, m.embedding, gw, None, status, out=buf[:, :S * D]),
            "emb_gather_plus_eager_gate": eager_fwd,
            "emb_gather_alone": lambda: ops.emb_gather(ids.reshape(-1), m.embedding, None, status, out=buf, out_group=S,
                                                       out_group_stride=LD),
            "gate_emb_bwd": lambda: ops.gate_emb_bwd(ids, m.embedding, gw, gbuf[:, :S * D], ws, None, status, out=dwv),
            "eager_gate_autograd_bwd": lambda: torch.autograd.grad(o_graph, (e_leaf, w_leaf), g3, retain_graph=True),
            "gate_hidden_fwd": lambda: ops.gate_hidden_fwd(y, t, out=x),
            "eager_hidden_fwd": lambda: torch.mul(y, torch.tanh(t0), out=x),
            "gate_hidden_bwd": lambda: ops.gate_hidden_bwd(u, y, h, out=(dt, uh)),
            "eager_hidden_bwd": lambda: (torch.mul(u * y, 1 - h * h, out=dt), torch.mul(u, h, out=uh)),
        }
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        tm = _alternate(cands)
        n = B * S
        mat = B * n512 * 4
        nbytes = {"gate_emb_fwd": n * (8 + 8 * D), "gate_emb_bwd": n * (8 + 12 * D),
                  "gate_hidden_fwd": 4 * mat, "gate_hidden_bwd": 5 * mat}          # y, t read, t, x written; u, y, h, dt, uh
        lines = {"gate_emb_fwd": n * (8 + LINE + 4 * D), "gate_emb_bwd": n * (8 + LINE + 8 * D)}
        out["kernels"]["B%d" % B] = {
            "ms": {k: round(v, 4) for k, v in tm.items()}, "bytes": nbytes,
            "bytes_per_lookup": {"fwd": 8 + 8 * D, "bwd": 8 + 12 * D, "fwd_whole_lines": 8 + LINE + 4 * D,
                                 "bwd_whole_lines": 8 + LINE + 8 * D},
            "frac_8TBs": {k: round(nbytes[k] / (tm[k] * 1e-3) / PEAK, 3) for k in nbytes},
            "frac_8TBs_whole_lines": {k: round(lines[k] / (tm[k] * 1e-3) / PEAK, 3) for k in lines},
            "replaced_over_kernel": {"emb_fwd": round(tm["emb_gather_plus_eager_gate"] / tm["gate_emb_fwd"], 2),
                                     "emb_bwd": round(tm["eager_gate_autograd_bwd"] / tm["gate_emb_bwd"], 2),
                                     "hidden_fwd": round(tm["eager_hidden_fwd"] / tm["gate_hidden_fwd"], 2),
                                     "hidden_bwd": round(tm["eager_hidden_bwd"] / tm["gate_hidden_bwd"], 2)}}
        del e_leaf, w_leaf, o_graph, g3
    ops.raise_on_status(m.status, "gatenet_bench")
    ops.raise_on_status(status, "gatenet_bench")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
