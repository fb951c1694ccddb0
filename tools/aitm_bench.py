#!/usr/bin/env python3
"""Times of the AITM kernels (csrc/aitm_ops.hip) against the torch-op chains they replace, and of a whole AITM train step.
Needs a GPU; not part of bench.py; there is no pass mark — the numbers go to DESIGN.md, wins and losses.

    python tools/aitm_bench.py [--out result.json]

Sizes: B 2000 (the reference's config_bigdata) and B 65 536, the shipped net otherwise (the 18 real vocabularies, 1 352 390
rows in all, D 5, dims [128, 64, 32], drop_prob [0.1, 0.3, 0.3]); ids uniform over each field's table.  Inputs are device
resident; every shape is warmed up; a figure is the median over 20 windows of device-event time, each window REPS
back-to-back calls (a launch-bound call is timed as it runs in a step: queued behind its predecessor).
  * gather_us: rec_field_gather_fwd into a packed [B, 90] buffer, rows_out included; gather_torch_us: the reference's
    expression, torch.cat([W_f[ids[:, f]] for f in fields], 1) over the 18 per-field views (no bounds check, no rows);
  * ait_fwd_us, ait_fwd_bwd_us: rec_ait_fwd, and rec_ait_fwd + rec_ait_bwd, from QKV [2B, 96]; ait_torch_fwd_us,
    ait_torch_fwd_bwd_us: Attention.forward's ops from the same QKV (slices, multiply, sum, scale, softmax, unsqueeze,
    multiply, sum) and autograd's backward of them to d(QKV);
  * head_us: rec_aitm_head with dz; head_torch_us: the two [B, 32] x [32, 1] products and biases, sigmoid,
    binary_cross_entropy twice, maximum / sum, the weighted total, and autograd's backward to the two logits;
  * auc_wide_us: rec_auc_histogram_wide (100 000 thresholds) on a column of pred [B, 2]; auc_torch_us: the bucket
    arithmetic and two index_add_ into the int64 histograms;
  * step_us: AITMLayer.train_step (train mode: Dropout on)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlerec_amd import ops                     # noqa: E402
from paddlerec_amd.aitm import AITMLayer          # noqa: E402

WINDOWS = 20
NAMES = "101 121 122 124 125 126 127 128 129 205 206 207 216 508 509 702 853 301".split()
SIZES = [238635, 98, 14, 3, 8, 4, 4, 3, 5, 467298, 6929, 263942, 106399, 5888, 104830, 51878, 37148, 4]
D, DIM, T = 5, 32, 100000


def timed(fn, reps, r=None, key=None):
    """Median microseconds per call over WINDOWS windows of `reps` calls; with r and key, r[key] = the median and
    r[key + "_min"], r[key + "_max"] = the fastest and slowest window (the spread)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    if r is not None:
        r[key], r[key + "_min"], r[key + "_max"] = statistics.median(out), min(out), max(out)
    return statistics.median(out)


def batch(B, dev="cuda"):
    g = torch.Generator().manual_seed(B)
    ids = torch.stack([torch.randint(0, n, (B,), generator=g) for n in SIZES], 1)
    click = torch.randint(0, 2, (B,), generator=g)
    buy = click & torch.randint(0, 2, (B,), generator=g)
    return ids.to(dev).contiguous(), click.to(dev), buy.to(dev)


def torch_ait(qkv, B):
    x = qkv.reshape(B, 2, 3 * DIM)
    Q, K, V = x[:, :, :DIM], x[:, :, DIM:2 * DIM], x[:, :, 2 * DIM:]
    a = torch.softmax((Q * K).sum(-1) / (DIM ** 0.5), 1)
    return (a.unsqueeze(-1) * V).sum(1)


def torch_head(tc, ait, wc, bc, wv, bv, y, t):
    with torch.no_grad():
        z0, z1 = torch.matmul(tc, wc) + bc, torch.matmul(ait, wv) + bv
    z0, z1 = z0.requires_grad_(True), z1.requires_grad_(True)
    p0, p1 = torch.sigmoid(z0).squeeze(1), torch.sigmoid(z1).squeeze(1)
    F = torch.nn.functional
    loss = F.binary_cross_entropy(p0, y) + F.binary_cross_entropy(p1, t) + 0.6 * torch.maximum(p1 - p0, torch.zeros_like(y)).sum()
    return torch.autograd.grad(loss, [z0, z1])


def kernels(B):
    dev, reps = "cuda", 200 if B <= 4096 else 50
    torch.manual_seed(B)
    N = sum(SIZES)
    W = torch.rand(N, D, device=dev) * 2 - 1
    begin = [0]
    for n in SIZES:
        begin.append(begin[-1] + n)
    fb = torch.tensor(begin, dtype=torch.int64, device=dev)
    views = [W[begin[i]:begin[i + 1]] for i in range(len(SIZES))]
    ids, click, buy = batch(B)
    r = {"B": B}
    out, rows, status = ops.field_gather_fwd(ids, W, fb)
    ref = torch.cat([views[f][ids[:, f]] for f in range(len(SIZES))], 1)
    assert torch.equal(out, ref) and int(status.item()) == 0, "the two gather routes disagree"
    timed(lambda: ops.field_gather_fwd(ids, W, fb, out=out, rows_out=rows, status=status), reps, r, "gather_us")
    timed(lambda: torch.cat([views[f][ids[:, f]] for f in range(len(SIZES))], 1), reps, r, "gather_torch_us")
    qkv = torch.randn(2 * B, 3 * DIM, device=dev)
    g = torch.randn(B, DIM, device=dev)
    o, prob = ops.ait_fwd(qkv, 2)
    dq = ops.ait_bwd(qkv, prob, g, 2)
    assert torch.allclose(o, torch_ait(qkv, B), rtol=1e-4, atol=1e-5), "the two AIT routes disagree"
    timed(lambda: ops.ait_fwd(qkv, 2, out=o, prob=prob), reps, r, "ait_fwd_us")
    timed(lambda: (ops.ait_fwd(qkv, 2, out=o, prob=prob), ops.ait_bwd(qkv, prob, g, 2, out=dq)), reps, r, "ait_fwd_bwd_us")
    with torch.no_grad():
        timed(lambda: torch_ait(qkv, B), reps, r, "ait_torch_fwd_us")
    qg = qkv.clone().requires_grad_(True)
    timed(lambda: torch.autograd.grad(torch_ait(qg, B), qg, g), reps, r, "ait_torch_fwd_bwd_us")
    tc, ait = torch.randn(B, DIM, device=dev), torch.randn(B, DIM, device=dev)
    wc, wv = torch.randn(DIM, 1, device=dev) / DIM ** 0.5, torch.randn(DIM, 1, device=dev) / DIM ** 0.5
    bc, bv = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    timed(lambda: ops.aitm_head(tc, ait, wc, bc, wv, bv, click, buy, 0.6, 1.0 / B), reps, r, "head_us")
    y, t = click.float(), buy.float()
    timed(lambda: torch_head(tc, ait, wc, bc, wv, bv, y, t), reps, r, "head_torch_us")
    pred = ops.aitm_head(tc, ait, wc, bc, wv, bv, click, buy, 0.6, 1.0 / B)[0]
    pos, neg = (torch.zeros(T + 1, dtype=torch.int64, device=dev) for _ in range(2))
    timed(lambda: ops.auc_histogram_wide(pred[:, 1], buy, pos, neg, T), reps, r, "auc_wide_us")

    def torch_auc():
        bucket = (pred[:, 1] * float(T)).long().clamp_(0, T)
        pos.index_add_(0, bucket, (buy != 0).long())
        neg.index_add_(0, bucket, (buy == 0).long())

    timed(torch_auc, reps, r, "auc_torch_us")
    return r


def steps(B):
    torch.manual_seed(1)
    ids, click, buy = batch(B)
    m = AITMLayer([[n, s] for n, s in zip(NAMES, SIZES)], D, [128, 64, 32], [0.1, 0.3, 0.3], device="cuda")
    r = {"B": B}
    timed(lambda: m.train_step(ids, click, buy, 1e-4), 10, r, "step_us")
    assert int(m.status.item()) == 0
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/aitm_bench.py needs a GPU"
    res = dict(kernels=[kernels(2000), kernels(65536)], steps=[steps(2000), steps(65536)])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
