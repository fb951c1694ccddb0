#!/usr/bin/env python3
"""FFM (paddlerec_amd/ffm.py, csrc/ffm_ops.hip) at the reference's shape: S 26 sparse slots, Dn 13 dense fields, D 9
(rows of 351 floats kept at 352), the bigdata table of 1 000 001 rows.  Prints ONE JSON line:
  * ms per train step (FFMLayer.train_step) at B 4096 and B 65536, lazy and non-lazy Adam;
  * rec_ffm_fwd / rec_ffm_bwd times at those batches (HIP events around 20 back-to-back calls, median of 5);
  * their algorithmic bytes (the S row gathers of 352 floats, the row-gradient writes, ids / dense / outputs) and the
    fraction of 8 TB/s those bytes take in the measured time.

    python tools/ffm_bench.py [--steps 20] [--warmup 5]

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
R = (S + DN) * D
RP = (R + 3) // 4 * 4
PEAK = 8e12


def _time(fn, reps=20, rounds=5):
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
    ids = torch.as_tensor(rng.integers(0, N, (B, S), dtype=np.int64), device=dev)
    dense = torch.as_tensor(rng.random((B, DN), dtype=np.float32), device=dev)
    label = torch.as_tensor((rng.random((B, 1)) < 0.25).astype(np.int64), device=dev)
    return ids, dense, label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from paddlerec_amd import ops
    from paddlerec_amd.ffm import FFMLayer
    dev = "cuda"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = FFMLayer(N, D, DN, S + DN, device=dev)
    with torch.no_grad():          # keep the toy logits off the saturated Constant(1.0) start
        m.dense.p["ffm.dense_w"].mul_(0.05)
        m.dense.p["ffm.dense_w_one"].mul_(0.05)
    out = {"model": "ffm", "shape": {"N": N, "S": S, "Dn": DN, "D": D, "row_floats": R, "row_stride": RP},
           "device": torch.cuda.get_device_name(0), "step_ms": {}, "kernels": {}}
    for B in (4096, 65536):
        ids, dense, label = _batch(B, rng, dev)
        for lazy in (True, False):
            m.lazy_mode = lazy
            for _ in range(args.warmup):
                m.train_step(ids, dense, label, lr=1e-3)
            torch.cuda.synchronize()
            ms = _time(lambda: m.train_step(ids, dense, label, lr=1e-3), reps=args.steps, rounds=3)
            out["step_ms"]["B%d_%s" % (B, "lazy" if lazy else "nonlazy")] = round(ms, 4)
        ws = ops.Workspace(dev)
        dz = torch.randn(B, device=dev) * 1e-3
        y = ops.ffm_fwd(ids, dense, m.emb_table, m.embedding_one, m.dense.p["ffm.dense_w"], m.dense.p["ffm.dense_w_one"],
                        D, m.status)
        bo = ops.ffm_bwd(ids, dense, m.emb_table, m.dense.p["ffm.dense_w"], dz, D, ws, status=m.status)
        t_f = _time(lambda: ops.ffm_fwd(ids, dense, m.emb_table, m.embedding_one, m.dense.p["ffm.dense_w"],
                                        m.dense.p["ffm.dense_w_one"], D, m.status, out=y[:2]))
        t_b = _time(lambda: ops.ffm_bwd(ids, dense, m.emb_table, m.dense.p["ffm.dense_w"], dz, D, ws, out=bo,
                                        status=m.status))
        common = B * S * 8 + B * DN * 4                                   # ids + dense
        fwd_bytes = B * S * RP * 4 + B * S * 4 + common + 2 * B * 4        # rows + W1 + ids/dense + y1, y2
        bwd_bytes = 2 * B * S * RP * 4 + common + B * 4                    # rows re-gathered + row_grad written + dz
        out["kernels"]["B%d" % B] = {
            "fwd_ms": round(t_f, 4), "bwd_ms": round(t_b, 4),
            "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
            "fwd_frac_8TBs": round(fwd_bytes / (t_f * 1e-3) / PEAK, 3),
            "bwd_frac_8TBs": round(bwd_bytes / (t_b * 1e-3) / PEAK, 3),
            "pair_frac_8TBs": round((fwd_bytes + bwd_bytes) / ((t_f + t_b) * 1e-3) / PEAK, 3)}
    ops.raise_on_status(m.status, "ffm_bench")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
