#!/usr/bin/env python3
"""Times of the entire-space kernels (csrc/esm_ops.hip) against the routes they replace, and of a whole ESMM / ESCM2 train
step.  Needs a GPU; not part of bench.py; there is no pass mark — the numbers go to DESIGN.md, wins and losses.

    python tools/esm_bench.py [--out result.json]

Sizes: B 1024 (the reference's config_bigdata) and B 65 536, the shipped nets otherwise (737 946 x 12 table, 23 fields,
max_len 3, half of the ids padding).  Inputs are device resident; every shape is warmed up; a figure is the median over 20
windows of device-event time, each window REPS back-to-back calls (a launch-bound call is timed as it runs in a step: queued
behind its predecessor).
  * pool_us: rec_field_sumpool_fwd into a packed [B, F*D] buffer;
  * pool_lod_us: rec_emb_gather_sumpool over the same ids flattened to [B*F*L] with the arithmetic LoD 0, L, 2L, ... (its
    output [B*F, D] is the same memory; the LoD buffer is built once, outside the timing);
  * pool_torch_us: the torch expression (W[ids] * (ids != 0)[..., None]).sum(2).reshape(B, F*D);
  * head_<mode>_us against torch_head_<mode>_us: the reference's op chain (softmax, clip, slice, multiply, log_loss, the
    IPW / DR weighting under detach, mean) and autograd's backward of it;
  * esmm_step_us / escm2_dr_step_us / escm2_ipw_step_us: train_step of the host layers."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlerec_amd import ops                     # noqa: E402
from paddlerec_amd.escm2 import ESCMLayer         # noqa: E402
from paddlerec_amd.esmm import ESMMLayer          # noqa: E402

WINDOWS = 20
N, D, F, L = 737946, 12, 23, 3


def timed(fn, reps):
    """Median microseconds per call over WINDOWS windows of `reps` calls."""
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
    return statistics.median(out)


def batch(B, dev="cuda"):
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(1, N, (B, F, L), generator=g)
    ids[torch.rand(B, F, L, generator=g) < 0.5] = 0
    click = torch.randint(0, 2, (B,), generator=g)
    buy = click & torch.randint(0, 2, (B,), generator=g)
    return ids.to(dev), click.to(dev), buy.to(dev)


def torch_loss(z, click, buy, mode, gw, cw):
    """The reference's loss from the towers' logits, op by op."""
    B = z.shape[0]
    p = torch.softmax(z.reshape(B, -1, 2), 2)
    if mode != "ESMM":
        p = torch.clamp(p, 1e-15, 1 - 1e-15)
    ll = lambda x, t: -t * torch.log(x + 1e-4) - (1 - t) * torch.log(1 - x + 1e-4)
    y, t = click.float(), buy.float()
    p1, q1 = p[:, 0, 1], p[:, 1, 1]
    cost = ll(p1, y) + gw * ll(p1 * q1, t)
    if mode == "IPW":
        ips = (torch.clamp(1.0 / torch.clamp(p1 * click.sum().float(), min=1e-6), -15, 15) * float(B)).detach()
        cost = cost + cw * (ll(q1, t) * ips * y).mean()
    elif mode == "DR":
        i1 = p[:, 2, 1]
        e = ll(q1, t) - i1
        ips = torch.clamp(y / torch.clamp(p1, min=1e-6), -15, 15).detach()
        cost = cost + cw * (i1 + e * ips + e * e * ips).mean()
    return cost.mean()


def kernels(B):
    dev, reps = "cuda", 200 if B <= 4096 else 50
    torch.manual_seed(B)
    W = torch.rand(N, D, device=dev) * 2 - 1
    W[0].zero_()
    ids, click, buy = batch(B)
    r = {"B": B}
    out, status = ops.field_sumpool_fwd(ids, W, 0)
    r["pool_us"] = timed(lambda: ops.field_sumpool_fwd(ids, W, 0, out=out, status=status), reps)
    flat = ids.reshape(-1).contiguous()
    lod = torch.arange(0, B * F * L + 1, L, dtype=torch.int64, device=dev)
    bow = ops.emb_gather_sumpool(flat, lod, W, 0, status)[0]
    assert torch.allclose(bow.reshape(B, F * D), out, rtol=1e-5, atol=1e-6), "the two pool routes disagree"
    r["pool_lod_us"] = timed(lambda: ops.emb_gather_sumpool(flat, lod, W, 0, status), reps)
    r["pool_torch_us"] = timed(lambda: (W[ids] * (ids != 0).unsqueeze(-1)).sum(2).reshape(B, F * D), reps)
    for mode, G, gw, cw in (("ESMM", 2, 1.0, 0.0), ("IPW", 2, 1.0, 0.01), ("DR", 3, 1.0, 0.01)):
        z = torch.randn(B, 2 * G, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        r["head_%s_us" % mode.lower()] = timed(lambda: ops.esm_head(z, click, buy, mode, gw, cw, 1.0 / B, click_count=count), reps)
        zg = z.clone().requires_grad_(True)
        r["torch_head_%s_us" % mode.lower()] = timed(
            lambda: torch.autograd.grad(torch_loss(zg, click, buy, mode, gw, cw), zg), reps)
    return r


def steps(B):
    dev = "cuda"
    torch.manual_seed(1)
    ids, click, buy = batch(B)
    out = {"B": B}
    nets = (("esmm", lambda: ESMMLayer(N, D, F, [256, 64], [256, 64], device=dev)),
            ("escm2_dr", lambda: ESCMLayer(N, D, F, None, None, 8, 16, 8, "DR", F * D, global_w=1.0, counterfactual_w=0.01, device=dev)),
            ("escm2_ipw", lambda: ESCMLayer(N, D, F, None, None, 8, 16, 8, "IPW", F * D, global_w=1.0, counterfactual_w=0.01, device=dev)))
    for name, make in nets:
        m = make()
        out[name + "_step_us"] = timed(lambda: m.train_step(ids, click, buy, 1e-3), 10)
        assert int(m.status.item()) == 0
        del m
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/esm_bench.py needs a GPU"
    res = dict(kernels=[kernels(1024), kernels(65536)], steps=[steps(1024), steps(65536)])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
