#!/usr/bin/env python3
"""Times of the multitask kernels (csrc/mtl_ops.hip) against the same arithmetic written in torch ops, and of a whole MMoE /
PLE train step.  Needs a GPU; not part of bench.py; there is no pass mark — the numbers go to DESIGN.md, wins and losses.

    python tools/mtl_bench.py [--out result.json]

Kernel sizes: B 65 536 and B 512, E 8 experts of size S 16, G 2 gates (the shipped MMoE), and one wide shape, B 8192 with
E 16, S 256, G 4 (a whole wave per row).  Inputs are device resident; every shape is warmed up; a figure is the median over 20 windows of device-event time, each window REPS back-to-back calls (a
launch-bound call is timed as it runs in a step: queued behind its predecessor).  The torch side is the chain of small ops
over [B, E, S] intermediates the reference writes: softmax, reshape, multiply, sum — and autograd's backward of it, timed
with torch.autograd.grad on a retained graph."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlerec_amd import ops                     # noqa: E402
from paddlerec_amd.mmoe import MMoELayer          # noqa: E402
from paddlerec_amd.ple import PLELayer            # noqa: E402

WINDOWS = 20


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


def kernels(B, E=8, S=16, G=2):
    dev, reps = "cuda", 200 if B <= 4096 else 50
    torch.manual_seed(B)
    H = torch.relu(torch.randn(B, E * S, device=dev))
    logits = torch.randn(B, G * E, device=dev)
    dmix = torch.randn(B, G * S, device=dev)
    mix = ops.MtlMix(S, E, [(0, E, 0, 0)] * G)
    prob, out = ops.mtl_mix_fwd(mix, H, logits)
    dH, dl = ops.mtl_mix_bwd(mix, H, prob, dmix)
    r = {"B": B, "E": E, "S": S, "G": G}
    r["mix_fwd_us"] = timed(lambda: ops.mtl_mix_fwd(mix, H, logits, prob=prob, out=out), reps)
    r["mix_bwd_us"] = timed(lambda: ops.mtl_mix_bwd(mix, H, prob, dmix, True, dH=dH, dlogits=dl), reps)

    def torch_fwd(Hh, lg):
        Hr = Hh.reshape(B, E, S)
        return torch.cat([(Hr * torch.softmax(lg[:, g * E:(g + 1) * E], 1).reshape(B, E, 1)).sum(1) for g in range(G)], 1)

    r["torch_mix_fwd_us"] = timed(lambda: torch_fwd(H, logits), reps)
    Hg, lg = H.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    y = torch_fwd(Hg, lg)
    r["torch_mix_bwd_us"] = timed(lambda: torch.autograd.grad(y, (Hg, lg), dmix, retain_graph=True), reps)
    z = torch.randn(B, 4, device=dev)                   # the head: two tasks whatever the mixture's shape
    label = torch.randint(0, 2, (B, 2), device=dev).float()
    r["head_us"] = timed(lambda: ops.mtl_head(z, label, 1.0 / B), reps)

    def torch_head(zz):
        p = torch.clamp(torch.softmax(zz.reshape(B, 2, 2), 2), 1e-15, 1 - 1e-15)[:, :, 1]
        return (-label * torch.log(p + 1e-4) - (1 - label) * torch.log(1 - p + 1e-4)).mean(0).sum()

    zg = z.clone().requires_grad_(True)

    def torch_head_step():
        torch.autograd.grad(torch_head(zg), zg)

    r["torch_head_fwd_bwd_us"] = timed(torch_head_step, reps)
    return r


def steps(B=65536, F=499):
    dev = "cuda"
    torch.manual_seed(1)
    x = torch.randn(B, F, device=dev)
    label = torch.randint(0, 2, (B, 2), device=dev).float()
    out = {"B": B}
    for name, m in (("mmoe", MMoELayer(F, 8, 16, 8, 2, device=dev)), ("ple", PLELayer(F, 2, 3, 2, 16, 8, 1, device=dev))):
        with torch.no_grad():                               # the constant initialisers saturate on normal features
            for k, v in m.state_dict().items():
                v.copy_(0.05 * torch.randn_like(v))
        m.set_dict({})
        out[name + "_step_us"] = timed(lambda: m.train_step(x, label, 1e-3), 10)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/mtl_bench.py needs a GPU"
    res = dict(kernels=[kernels(65536), kernels(512), kernels(8192, 16, 256, 4)], steps=steps())
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
