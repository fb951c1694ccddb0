#!/usr/bin/env python3
"""Deep & Cross (paddlerec_amd/dcn.py, csrc/dcn_cross.hip) at the reference's shape: S 26 sparse slots, D 9, Dn 13 raw
dense values (feature rows of d = 247 floats kept at a stride of 248), cross_num 2, the [512, 256, 128] tower, the
bigdata table of 1 000 001 rows.  Prints ONE JSON line; at B 4096 and B 65536 (kernels also at B 262144, whose 0.5 - 0.8 GB
working sets do not fit the 256 MiB Infinity Cache the way the 130 - 195 MB of B 65536 do):
  * rec_dcn_cross_fwd (training form: saved scalars + l2) and rec_dcn_cross_bwd times — HIP events around back-to-back
    calls, median of the rounds — in the layer's own layout (x_0 at stride 248, x_L into columns [128, 375) of the
    [B, 376] fc input, dX_0 accumulated into a stride-248 buffer, the upstream gradient in the rank-1 form), plus the
    matrix form of the backward and both kernels on rows of 247 floats back to back (the scalar-access variants);
  * their algorithmic bytes from the shapes (every [B, d] matrix the call must read or write once, + the saved scalars)
    and the share of 8 TB/s those bytes take in the measured time;
  * the same cross stack restated with eager torch ops on the same device (forward; forward + hand-written backward),
    timed in the same process, alternating with the kernels round by round;
  * ms per train step (DeepCroLayer.train_step), lazy and non-lazy Adam.

    python tools/dcn_bench.py [--steps 20] [--warmup 5]
    python tools/dcn_bench.py --case fwd --batch 65536     # that one call 50 times and nothing else: for a kernel trace

Not part of bench.py: the project's flagship measurement stays as it is.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

N, S, DN, D, L = 1000001, 26, 13, 9, 2
FC = [512, 256, 128]
WIDTH = S * D + DN
LD = (WIDTH + 3) // 4 * 4
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


def eager_fwd(x0, w, b):
    x, l2, xs, ss = x0, None, [x0], []
    for _ in range(L):
        xw = x * w
        s = xw.sum(dim=1, keepdim=True)
        t = (xw * xw).sum()
        l2 = t if l2 is None else l2 + t
        x = x0 * s + b + x
        xs.append(x)
        ss.append(s)
    return x, l2, xs, ss


def eager_bwd(x0, w, xs, ss, g):
    dx0 = dw = db = None
    for l in reversed(range(L)):
        xl = xs[l]
        t = (g * x0).sum(dim=1, keepdim=True)
        d0 = g * ss[l]
        dx0 = d0 if dx0 is None else dx0 + d0
        gb = g.sum(dim=0)
        gw = (t * xl).sum(dim=0) + 2.0 * (xl * xl * w).sum(dim=0)
        db = gb if db is None else db + gb
        dw = gw if dw is None else dw + gw
        g = g + t * w + 2.0 * xl * w * w
    return dx0 + g, dw, db


def _batch(B, rng, dev):
    ids = torch.as_tensor(rng.integers(0, N, (B, S), dtype=np.int64), device=dev)
    dense = torch.as_tensor(rng.random((B, DN), dtype=np.float32), device=dev)
    label = torch.as_tensor((rng.random((B, 1)) < 0.25).astype(np.int64), device=dev)
    return ids, dense, label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", default=None, help="run only this candidate (a key of the ms table), 50 calls")
    ap.add_argument("--batch", type=int, default=65536, help="batch of --case")
    args = ap.parse_args()
    from paddlerec_amd import ops
    from paddlerec_amd.dcn import DeepCroLayer
    dev = "cuda"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = DeepCroLayer(N, D, DN, S, FC, L, device=dev)
    H = FC[-1]
    out = {"model": "dcn", "shape": {"N": N, "S": S, "Dn": DN, "D": D, "d": WIDTH, "row_stride": LD, "cross_num": L,
                                     "fc": FC}, "device": torch.cuda.get_device_name(0), "step_ms": {}, "kernels": {}}
    w, b = m.dense.p["layer_w"], m.dense.p["layer_b"]
    u = m.dense.p["fc.weight"][H:].reshape(-1)
    for B in ((args.batch,) if args.case else (4096, 65536, 262144)):
        ids, dense, label = _batch(B, rng, dev)
        for lazy in ((True, False) if B <= 65536 and not args.case else ()):
            m.lazy_mode = lazy
            for _ in range(args.warmup):
                m.train_step(ids, dense, label, lr=1e-4)
            torch.cuda.synchronize()
            ms = _alternate({"step": lambda: m.train_step(ids, dense, label, lr=1e-4)}, reps=args.steps, rounds=3)["step"]
            out["step_ms"]["B%d_%s" % (B, "lazy" if lazy else "nonlazy")] = round(ms, 4)
        ws = ops.Workspace(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        x0 = (torch.randn(B, LD, **f32))[:, :WIDTH]
        last = torch.empty(B, (H + WIDTH + 3) // 4 * 4, **f32)
        xl = last[:, H:H + WIDTH]
        saved, l2 = torch.empty(B, L, **f32), torch.empty(1, **f32)
        dz = torch.randn(B, 1, **f32) * 1e-3
        g = (torch.randn(B, LD, **f32) * 1e-3)[:, :WIDTH]
        dx0 = torch.zeros(B, LD, **f32)[:, :WIDTH]
        dw, db = torch.empty(WIDTH, **f32), torch.empty(WIDTH, **f32)
        x0c, gc = x0.contiguous(), g.contiguous()                       # rows of 247 floats back to back
        xlc, dx0c = torch.empty(B, WIDTH, **f32), torch.zeros(B, WIDTH, **f32)
        fwd = lambda: ops.dcn_cross_fwd(x0, w, b, L, ws, out=(xl, saved, l2))
        fwd_inf = lambda: ops.dcn_cross_fwd(x0, w, b, L, ws, want_saved=False, want_l2=False, out=(xl, None, None))
        fwd_c = lambda: ops.dcn_cross_fwd(x0c, w, b, L, ws, out=(xlc, saved, l2))
        bwd_r1 = lambda: ops.dcn_cross_bwd(x0, w, b, saved, None, ws, accumulate=True, out=(dx0, dw, db), dz=dz, u=u)
        bwd_mat = lambda: ops.dcn_cross_bwd(x0, w, b, saved, g, ws, out=(dx0, dw, db))
        bwd_c = lambda: ops.dcn_cross_bwd(x0c, w, b, saved, gc, ws, out=(dx0c, dw, db))
        _, _, xs, ss = eager_fwd(x0c, w, b)
        cands = {"fwd": fwd, "fwd_inference": fwd_inf, "fwd_stride247": fwd_c, "bwd_rank1_accumulate": bwd_r1,
                 "bwd_matrix": bwd_mat, "bwd_matrix_stride247": bwd_c,
                 "eager_fwd": lambda: eager_fwd(x0c, w, b), "eager_bwd": lambda: eager_bwd(x0c, w, xs, ss, gc)}
        if args.case:
            for _ in range(50):
                cands[args.case]()
            torch.cuda.synchronize()
            out["kernels"]["B%d" % B] = {"case": args.case, "calls": 50}
            continue
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        t = _alternate(cands)
        mat = B * WIDTH * 4                                              # one [B, d] matrix
        sv = B * L * 4
        nbytes = {"fwd": 2 * mat + sv, "fwd_inference": 2 * mat, "fwd_stride247": 2 * mat + sv,
                  "bwd_rank1_accumulate": 3 * mat + sv + B * 4,          # x_0, dX_0 read and written, saved, dz
                  "bwd_matrix": 3 * mat + sv, "bwd_matrix_stride247": 3 * mat + sv}   # x_0, dXL, dX_0 written, saved
        k = {"ms": {n: round(v, 4) for n, v in t.items()}, "bytes": nbytes,
             "frac_8TBs": {n: round(nbytes[n] / (t[n] * 1e-3) / PEAK, 3) for n in nbytes},
             "eager_over_kernel": {"fwd": round(t["eager_fwd"] / t["fwd"], 2),
                                   "bwd": round(t["eager_bwd"] / t["bwd_matrix"], 2)}}
        out["kernels"]["B%d" % B] = k
    ops.raise_on_status(m.status, "dcn_bench")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
