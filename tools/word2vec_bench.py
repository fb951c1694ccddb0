#!/usr/bin/env python3
"""Times of the word2vec kernels (csrc/w2v_ops.hip) against the torch-op chains they replace, and of a whole train step.
Needs a GPU; not part of bench.py; there is no pass mark — the numbers go to DESIGN.md, wins and losses.

    python tools/word2vec_bench.py [--out result.json] [--batches 100,65536] [--queries 1024]

Sizes: D 300, neg 5, V 354 051 (config_bigdata.yaml); B 100 (the shipped batch) and B 65 536; the negatives once SHARED by the
whole batch (what the reference's reader yields) and once drawn independently per sample; the search at Q 1024, k 4.  Input and
true ids are uniform over the table.  Inputs are device resident; every shape is warmed up; a figure is the median over 20
windows of device-event time, each window REPS back-to-back calls (min and max of the windows are kept as the spread).
  * fwd_bwd_us: rec_w2v_sgns_fwd_bwd; fwd_bwd_torch_us: Word2VecLayer.forward's ops (three embedding lookups, the row dot,
    the batched matmul, the adds), sigmoid, the two binary_cross_entropy, and autograd's backward to the three gathered
    tensors (which is where the torch chain's [B, 1 + neg, D] gradient appears);
  * update_us: rec_w2v_target_update on a grouping made ahead; update_bytes_per_s: the bytes the update needs — per
    occurrence one input row (4 D), per unique row one read and one write of emb_w (8 D) — over update_us; update_torch_us:
    g[..., None] * emb[in_ids][:, None, :] materialised as [B, 1 + neg, D], then index_add_ into emb_w, scaled by -lr;
  * topk_us: rec_w2v_analogy_topk; topk_torch_us: Word2VecInferLayer.forward's ops (normalize the whole table, matmul to
    [Q, V], topk);
  * step_us: Word2VecLayer.train_step (both groupings, the target update and the input rows' SGD included)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlerec_amd import ops                         # noqa: E402
from paddlerec_amd.word2vec import Word2VecLayer      # noqa: E402

WINDOWS = 20
V, D, NEG, K = 354051, 300, 5, 4


def timed(fn, reps, r, key):
    """r[key] = median microseconds per call over WINDOWS windows of `reps` calls; r[key + "_min" / "_max"]: the spread."""
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
    r[key], r[key + "_min"], r[key + "_max"] = statistics.median(out), min(out), max(out)
    return r[key]


def torch_fwd_bwd(m, in_ids, target_ids):
    """net.py:57-81 + dygraph_model.py:53-69 + backward to the gathered rows."""
    F = torch.nn.functional
    x = m.emb[in_ids].requires_grad_()
    w = m.emb_w[target_ids].requires_grad_()
    b = m.emb_b[target_ids].squeeze(-1).requires_grad_()
    true_logits = (x * w[:, 0]).sum(1, keepdim=True) + b[:, :1]
    neg_logits = torch.matmul(x.unsqueeze(1), w[:, 1:].transpose(1, 2)).reshape(-1, NEG) + b[:, 1:]
    loss = F.binary_cross_entropy(torch.sigmoid(true_logits), torch.ones_like(true_logits)) + \
        F.binary_cross_entropy(torch.sigmoid(neg_logits), torch.zeros_like(neg_logits))
    loss.backward()
    return x.grad, w.grad, b.grad


def torch_update(m, in_ids, target_ids, g, lr):
    dw = g.unsqueeze(-1) * m.emb[in_ids].unsqueeze(1)                       # [B, 1 + neg, D]
    m.emb_w.index_add_(0, target_ids.reshape(-1), dw.reshape(-1, D), alpha=-lr)
    m.emb_b.index_add_(0, target_ids.reshape(-1), g.reshape(-1, 1), alpha=-lr)


def bench_batch(B, shared, r):
    dev = "cuda"
    gen = torch.Generator(device="cpu").manual_seed(B + int(shared))
    m = Word2VecLayer(V, D, NEG, device=dev)
    m.emb_w.normal_(0.0, 0.05)
    in_ids = torch.randint(0, V, (B,), generator=gen).to(dev)
    neg = torch.randint(0, V, (1 if shared else B, NEG), generator=gen).expand(B, NEG)
    target_ids = torch.cat([torch.randint(0, V, (B, 1), generator=gen), neg], 1).contiguous().to(dev)
    tag = "B%d_%s" % (B, "shared" if shared else "indep")
    reps = 20 if B <= 1000 else 3
    st = ops.new_status(dev)
    timed(lambda: ops.w2v_sgns_fwd_bwd(in_ids, target_ids, m.emb, m.emb_w, m.emb_b, 1.0, st), reps, r, tag + "_fwd_bwd_us")
    timed(lambda: torch_fwd_bwd(m, in_ids, target_ids), reps, r, tag + "_fwd_bwd_torch_us")
    g = ops.w2v_sgns_fwd_bwd(in_ids, target_ids, m.emb, m.emb_w, m.emb_b, 1.0, st)[2]
    groups = ops.IdGroups(target_ids.numel(), dev)
    ops.ids_group(target_ids.reshape(-1), V, None, ops.Workspace(dev), None, None, groups)
    n_uniq = int(groups.n_uniq[0].item())
    us = timed(lambda: ops.w2v_target_update(groups, g, in_ids, m.emb, m.emb_w, m.emb_b, 1e-3), reps, r, tag + "_update_us")
    r[tag + "_update_bytes"] = 4 * D * target_ids.numel() + 8 * D * n_uniq
    r[tag + "_update_bytes_per_s"] = r[tag + "_update_bytes"] / (us * 1e-6)
    r[tag + "_unique_target_rows"] = n_uniq
    timed(lambda: torch_update(m, in_ids, target_ids, g, 1e-3), reps, r, tag + "_update_torch_us")
    timed(lambda: m.train_step(in_ids, target_ids, 1e-3), reps, r, tag + "_step_us")
    assert int(st.item()) == 0 and int(m.status.item()) == 0


def bench_topk(Q, r):
    dev = "cuda"
    W = torch.randn(V, D, device=dev) * 0.1
    a, b, c = (torch.randint(0, V, (Q,), device=dev) for _ in range(3))

    def hip():
        return ops.w2v_analogy_topk(a, b, c, W, K)

    def chain():
        target = W[b] - W[a] + W[c]
        return torch.topk(torch.matmul(target, torch.nn.functional.normalize(W, dim=1).t()), K)

    v1, i1 = hip()
    v2, i2 = chain()
    r["Q%d_topk_ids_equal_torch" % Q] = float((i1 == i2).float().mean().item())
    timed(hip, 3, r, "Q%d_topk_us" % Q)
    timed(chain, 3, r, "Q%d_topk_torch_us" % Q)
    r["Q%d_topk_flop_per_s" % Q] = 2.0 * Q * V * D / (r["Q%d_topk_us" % Q] * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="100,65536")
    ap.add_argument("--queries", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("word2vec_bench needs a GPU: nothing is measured without one")
    r = dict(V=V, D=D, neg=NEG, k=K, windows=WINDOWS)
    for B in (int(x) for x in args.batches.split(",")):
        for shared in (True, False):
            bench_batch(B, shared, r)
            print(json.dumps({k: v for k, v in r.items() if k.startswith("B%d_%s" % (B, "shared" if shared else "indep"))}), flush=True)
    bench_topk(args.queries, r)
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
