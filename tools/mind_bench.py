#!/usr/bin/env python3
"""Times of the MIND kernels (csrc/mind_ops.hip) against the torch-op chains they replace, and of a whole MIND train step.
Needs a GPU; not part of bench.py; there is no pass mark — the numbers go to DESIGN.md, wins and losses.

    python tools/mind_bench.py [--out result.json] [--batches 128,65536]

Sizes: B 128 (the reference's config.yaml) and B 65 536, the shipped net otherwise (367 983 items, embedding_dim = hidden_size
64, maxlen 20, k_max 4, iters 3, neg_samples 128, pow_p 1); history ids uniform over the table, seq_len uniform in 1..maxlen.
Inputs are device resident; every shape is warmed up; a figure is the median over 20 windows of device-event time, each window
REPS back-to-back calls (a launch-bound call is timed as it runs in a step: queued behind its predecessor).
  * routing_fwd_us: rec_mind_routing_fwd from low [B*T, H]; routing_torch_fwd_us: Mind_Capsual_Layer.forward's ops from the
    same low (net.py:186-229: the tile / reshape / transpose to [B, K, T, H], the mask, and per round where, softmax, two
    matmuls, squash);  routing_low_read_us: the time to read low once at the measured HBM copy rate (6.29 TB/s), the floor
    the forward is held against;
  * routing_bwd_us: rec_mind_routing_bwd; routing_torch_bwd_us: autograd's backward of the last W x low product and squash;
  * attn_us: rec_mind_label_attn_fwd + _bwd; attn_torch_us: label_aware_attention's ops (matmul, squeeze, pow, softmax,
    unsqueeze, matmul) and autograd's backward to caps2 and target;
  * head_us: rec_mind_ssm_head on S [B, n] with both row scalings; head_torch_us: net.py:86-112 from the same gathered rows
    and S (row dot, bias, equal / where, the two log_q subtractions, concat, soft-label cross entropy) and autograd's
    backward to S, user and true_w;
  * step_us: MindLayer.train_step with the negatives drawn ahead (the host's multinomial is not the device's time)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlerec_amd import ops                     # noqa: E402
from paddlerec_amd.mind import MindLayer          # noqa: E402

WINDOWS = 20
N, E, T, K, ITERS, NEG = 367983, 64, 20, 4, 3, 128
HBM = 6.29e12                                     # bytes / s, the measured float4 copy rate


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


def squash(Z):
    n2 = torch.sum(Z * Z, -1, keepdim=True)
    return n2 / (1 + n2) / torch.sqrt(n2 + 1e-8) * Z


def torch_routing(low, seq_len, logits, want_grad=False):
    """net.py:186-229 from low [B, T, H] (requires_grad when want_grad) -> caps [B, K, H]."""
    B = low.shape[0]
    mask = (torch.arange(T, device=low.device).unsqueeze(0).expand(B, T).reshape(B, -1, T) < seq_len.reshape(B, 1).repeat(1, K).unsqueeze(-1))
    pad = torch.ones_like(mask, dtype=torch.float32) * (-2 ** 32 + 1)
    tile = low.repeat(1, 1, K).reshape(-1, T, K, E).permute(0, 2, 1, 3).reshape(-1, K, T, E)
    nograd = tile.detach().clone()
    Bl = logits.repeat(B, 1, 1)
    for _ in range(ITERS - 1):
        W = torch.softmax(torch.where(mask, Bl, pad), 2).unsqueeze(2)
        high = squash(torch.matmul(W, nograd))
        Bl = Bl + torch.matmul(nograd, high.permute(0, 1, 3, 2)).reshape(-1, K, T)
    W = torch.softmax(torch.where(mask, Bl, pad), 1).unsqueeze(2)
    return squash(torch.matmul(W, tile)).reshape(-1, K, E)


def torch_attn(caps2, target):
    w = torch.matmul(caps2, target.reshape(-1, E, 1)).squeeze(-1)
    w = torch.softmax(torch.pow(w, 1.0), -1).unsqueeze(1)
    return torch.matmul(w, caps2).squeeze(1)


def torch_head(user, true_w, true_b, S, sample_b, labels, neg, lq_true, lq_neg):
    true = torch.sum(true_w.unsqueeze(1) * user.unsqueeze(1), -1) + true_b.reshape(-1, 1)
    s = S + sample_b
    s = torch.where(labels.reshape(-1, 1) == neg, torch.ones_like(s) * -1e30, s)
    true, s = true - lq_true.unsqueeze(1), s - lq_neg
    out = torch.cat([true, s], 1)
    lab = torch.cat([torch.ones_like(true), torch.zeros_like(s)], 1)
    return (-(lab * torch.log_softmax(out, -1)).sum(-1, keepdim=True)).mean()


def bench(B, dev="cuda"):
    r = {"batch": B}
    reps = 50 if B <= 4096 else 5
    g = torch.Generator(device="cpu").manual_seed(B)
    f32 = lambda *s: torch.randn(*s, generator=g).to(dev)
    low = (f32(B * T, E) / 8).contiguous()
    seq_len = torch.randint(1, T + 1, (B,), generator=g).to(dev)
    logits = f32(K, T)
    fwd = lambda: ops.mind_routing_fwd(low, seq_len, logits, ITERS)
    timed(fwd, reps, r, "routing_fwd_us")
    r["routing_low_read_us"] = low.numel() * 4 / HBM * 1e6
    low3 = low.view(B, T, E)
    with torch.no_grad():
        timed(lambda: torch_routing(low3, seq_len, logits), reps, r, "routing_torch_fwd_us")
    W, Z, caps = fwd()
    d_caps = f32(B, K, E)
    timed(lambda: ops.mind_routing_bwd(d_caps, Z, W), reps, r, "routing_bwd_us")
    Wc = W.unsqueeze(2)

    def torch_bwd():
        x = low3.detach().requires_grad_(True)
        tile = x.repeat(1, 1, K).reshape(-1, T, K, E).permute(0, 2, 1, 3).reshape(-1, K, T, E)
        squash(torch.matmul(Wc, tile)).reshape(-1, K, E).backward(d_caps)
        return x.grad

    timed(torch_bwd, reps, r, "routing_torch_bwd_us")          # forward of the last product + its backward
    with torch.no_grad():
        timed(lambda: squash(torch.matmul(Wc, low3.repeat(1, 1, K).reshape(-1, T, K, E).permute(0, 2, 1, 3))), reps, r,
              "routing_torch_last_fwd_us")                     # ... so that the backward alone is the difference
    caps2 = torch.relu(f32(B * K, E))
    target, d_user = f32(B, E) / 8, f32(B, E)

    def attn():
        user, a = ops.mind_label_attn_fwd(caps2, target, K, 1.0)
        return ops.mind_label_attn_bwd(caps2, target, a, d_user, 1.0)

    timed(attn, reps, r, "attn_us")
    c3 = caps2.view(B, K, E)

    def attn_torch():
        x, q = c3.detach().requires_grad_(True), target.detach().requires_grad_(True)
        torch_attn(x, q).backward(d_user)
        return x.grad, q.grad

    timed(attn_torch, reps, r, "attn_torch_us")
    user, true_w, S0 = f32(B, E) / 8, f32(B, E), f32(B, NEG)
    true_b, sample_b = f32(B), f32(NEG)
    neg = (torch.randperm(N - 1, generator=g)[:NEG] + 1).to(dev)
    labels = torch.randint(1, N, (B,), generator=g).to(dev)
    labels[0] = neg[0]
    lq_true, lq_neg = -torch.rand(B, generator=g).to(dev) - 1, -torch.rand(NEG, generator=g).to(dev) - 1
    S, dtw, du0 = S0.clone(), torch.empty(B, E, device=dev), torch.empty(B, E, device=dev)
    # the kernel overwrites S with its gradient: a gradient is a valid logit matrix, and the time does not depend on the values
    timed(lambda: ops.mind_ssm_head(user, true_w, true_b, S, sample_b, labels, neg, lq_true, lq_neg, 1.0 / B, dtw, du0), reps, r,
          "head_us")

    def head_torch():
        u, w, s = (t.detach().requires_grad_(True) for t in (user, true_w, S0))
        torch_head(u, w, true_b, s, sample_b, labels, neg, lq_true, lq_neg).backward()
        return u.grad, w.grad, s.grad

    timed(head_torch, reps, r, "head_torch_us")
    m = MindLayer(N, E, E, NEG, T, 1.0, ITERS, K, device=dev)
    hist = torch.randint(1, N, (B, T), generator=g).to(dev)
    hist = torch.where(torch.arange(T, device=dev)[None, :] < seq_len[:, None], hist, torch.zeros_like(hist))
    timed(lambda: m.train_step(hist, seq_len, labels, 0.005, neg=neg), max(reps // 5, 2), r, "step_us")
    assert int(m.status.item()) == 0
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="128,65536")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mind_bench.py needs a GPU: a CPU timing says nothing about the kernels")
    res = [bench(int(b)) for b in args.batches.split(",")]
    for r in res:
        print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
