#!/usr/bin/env python3
"""Time MatchPyramid's train step against the same net written as a torch chain on the same GPU (autograd + torch.optim.Adam),
and the two interaction entry points (rec_mpyr_fwd, rec_mpyr_bwd) against the torch ops they replace — embedding lookups, bmm,
conv2d over a SAME-padded image, relu, max_pool2d — and that chain's backward.

    python tools/match_pyramid_bench.py [--out match_pyramid_bench.json] [--rounds 5] [--iters 20]

Two shapes at B 128, the batch the loss fixes: "shipped" (config.yaml: sentences 20 x 500, emb 50, 8 filters of [2, 10], pool
[6, 50]) and "golden" (the fixtures' 7 x 21, emb 6, [2, 4], pool [2, 2]); vocab 193 368, ids uniform over the vocabulary with a
tenth of the words padding.  Every time is device time between two events around a window of back-to-back calls that lasts at
least 0.3 s (the call count comes from a probe, which is also the warm-up; `--iters` is its floor); the candidates alternate
within a round, and the spread over the rounds (min .. max of the per-round means) is reported beside the median.  The torch
backward is forward + backward minus the forward IN GRAD MODE (the graph recorded); it includes what autograd does that the
fused path never does: the dense [vocab, E] embedding gradient, zero-filled and scattered into.  "one_block_call" times a
one-block kernel (the hinge): what any single call costs from Python here, the floor under the small-shape kernel figures.
"fwd_kernel_channel_split" is the forward with the grid split by channel group (REC_MPYR_SPLIT=channel, read once by the
library, so a child process measures it) — the alternative DESIGN.md weighs.  A run without a GPU fails: there is no fallback.

The torch chain restates net.py's forward and dygraph_model.py's loss op by op because that is what a user of the reference
pays; it is written here and shares no text with the reference.  Its Adam is torch.optim.Adam over the whole table, as
Paddle's dygraph Adam is not lazy."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, PAD, B, HID, LR = 193368, 193367, 128, 20, 0.001
SHAPES = {"shipped": dict(Ll=20, Lr=500, E=50, K=8, filt=[2, 10], pool=[6, 50]),
          "golden": dict(Ll=7, Lr=21, E=6, K=8, filt=[2, 4], pool=[2, 2])}
WINDOW_S = 0.3           # every timed window runs at least this long: a shorter one measures the clock and the scheduler


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def calls_for(fn, floor):
    per_call_ms = max(timed(fn, max(floor, 5)), 1e-3)
    return int(min(max(floor, WINDOW_S * 1000.0 / per_call_ms), 100000))


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs))


class TorchChain(torch.nn.Module):
    def __init__(self, sh, dev):
        super().__init__()
        self.emb = torch.nn.Embedding(V, sh["E"], padding_idx=PAD, device=dev)
        self.conv = torch.nn.Conv2d(1, sh["K"], tuple(sh["filt"]), device=dev)
        self.fc1, self.fc2 = torch.nn.Linear(240, HID, device=dev), torch.nn.Linear(HID, 1, device=dev)
        kh, kw = sh["filt"]
        self.padding = ((kw - 1) // 2, kw - 1 - (kw - 1) // 2, (kh - 1) // 2, kh - 1 - (kh - 1) // 2)
        self.pool = tuple(sh["pool"])

    def interaction(self, left, right):
        cross = torch.bmm(self.emb(left), self.emb(right).transpose(1, 2)).unsqueeze(1)
        conv = torch.relu(self.conv(torch.nn.functional.pad(cross, self.padding)))
        return torch.nn.functional.max_pool2d(conv, self.pool, self.pool).reshape(left.shape[0], -1)

    def forward(self, left, right):
        pred = self.fc2(torch.relu(self.fc1(self.interaction(left, right))))
        return torch.clamp(1.0 - pred[0:64, 0:1] + pred[64:128, 0:1], min=0.0).mean()


def feeds(sh, seed, dev):
    rng = np.random.default_rng(seed)
    out = []
    for n in (sh["Ll"], sh["Lr"]):
        ids = rng.integers(0, PAD, (B, n))
        ids[rng.random(ids.shape) < 0.1] = PAD
        out.append(torch.as_tensor(ids.astype(np.int64)).to(dev))
    return out


def forward_only(name, dev, rounds, iters):
    """rec_mpyr_fwd alone at shape `name` -> stats (what a child process with REC_MPYR_SPLIT=channel runs)."""
    from paddlerec_amd import ops
    sh = SHAPES[name]
    torch.manual_seed(0)
    s = ops.MpyrShape(sh["Ll"], sh["Lr"], sh["E"], sh["K"], sh["filt"][0], sh["filt"][1], sh["pool"][0], sh["pool"][1],
                      sh["pool"][0], sh["pool"][1], 1)
    table = torch.randn(V, sh["E"], device=dev) * 0.1
    w, b = torch.randn(sh["K"] * sh["filt"][0] * sh["filt"][1], device=dev), torch.zeros(sh["K"], device=dev)
    left, right = feeds(sh, 1, dev)
    out = ops.mpyr_fwd(s, left, right, table, w, b, PAD)
    fn = lambda: ops.mpyr_fwd(s, left, right, table, w, b, PAD, out=out)
    n = calls_for(fn, iters)
    return dict(stats([timed(fn, n) for _ in range(rounds)]), calls=n)


def channel_split_forward(name, dev, rounds, iters):
    """The forward with the grid split by channel group instead of by pool-row band: the library reads REC_MPYR_SPLIT once, so
    a fresh child process measures it."""
    import subprocess
    env = dict(os.environ, REC_MPYR_SPLIT="channel")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-only", name, "--device", dev, "--rounds", str(rounds),
                        "--iters", str(iters)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("the channel-split child failed:\n" + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench_shape(name, sh, dev, rounds, iters):
    from paddlerec_amd import ops
    from paddlerec_amd.match_pyramid import MatchPyramidLayer
    torch.manual_seed(0)
    m = MatchPyramidLayer("", V, sh["E"], sh["K"], sh["filt"], "relu", HID, 1, sh["pool"], sh["pool"], "VALID", "max", "relu",
                          sh["Ll"], sh["Lr"], device=dev)
    chain = TorchChain(sh, dev)
    opt = torch.optim.Adam(chain.parameters(), lr=LR)
    left, right = feeds(sh, 1, dev)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        chain(left, right).backward()
        opt.step()
    p, T = m.store.view["p"], m.emb_store["p"]
    pooled, argmax = ops.mpyr_fwd(m.shape, left, right, T, p["conv.weight"], p["conv.bias"], PAD)
    d_pooled = torch.randn_like(pooled)
    rows = torch.empty(B * (sh["Ll"] + sh["Lr"]), sh["E"], device=dev)
    gw, gb, scratch = torch.empty_like(p["conv.weight"]).reshape(-1), torch.empty_like(p["conv.bias"]), {}
    out = (pooled, argmax)
    cands = {
        "step_fused": lambda: m.train_step([left, right], LR),
        "step_torch": torch_step,
        "fwd_kernel": lambda: ops.mpyr_fwd(m.shape, left, right, T, p["conv.weight"], p["conv.bias"], PAD, out=out),
        "bwd_kernel": lambda: ops.mpyr_bwd(m.shape, left, right, T, p["conv.weight"], p["conv.bias"], d_pooled, argmax,
                                           rows[:B * sh["Ll"]], rows[B * sh["Ll"]:], gw, gb, PAD, scratch=scratch),
    }

    def torch_fwd():
        with torch.no_grad():
            chain.interaction(left, right)

    def torch_fwd_grad():                                     # the forward as the backward needs it: the graph is recorded
        chain.interaction(left, right)
    pred = torch.randn(B, 1, device=dev)
    hinge_out = ops.mpyr_hinge(pred, 64)
    cands["fwd_grad_torch"] = torch_fwd_grad
    cands["one_block_call"] = lambda: ops.mpyr_hinge(pred, 64, out=hinge_out)      # a one-block kernel: what ANY call costs here

    def torch_fwd_bwd():
        chain.emb.weight.grad = None
        chain.conv.weight.grad = None
        chain.conv.bias.grad = None
        chain.interaction(left, right).backward(d_pooled)
    cands["fwd_torch"], cands["fwd_bwd_torch"] = torch_fwd, torch_fwd_bwd
    n_calls = {k: calls_for(f, iters) for k, f in cands.items()}
    per = {k: [] for k in cands}
    for _ in range(rounds):
        for k, f in cands.items():
            per[k].append(timed(f, n_calls[k]))
    res = {k: dict(stats(v), calls=n_calls[k]) for k, v in per.items()}
    res["bwd_torch"] = dict(median_ms=res["fwd_bwd_torch"]["median_ms"] - res["fwd_grad_torch"]["median_ms"])
    res["fwd_kernel_channel_split"] = channel_split_forward(name, dev, rounds, iters)
    res["shape"] = dict(sh, B=B, vocab=V)
    assert int(m.status.item()) == 0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--forward-only", default=None, metavar="SHAPE", help="time rec_mpyr_fwd alone at this shape and print its stats")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_pyramid_bench needs a GPU")
    if args.forward_only:
        print(json.dumps(forward_only(args.forward_only, args.device, args.rounds, args.iters)))
        return
    out = {name: bench_shape(name, sh, args.device, args.rounds, args.iters) for name, sh in SHAPES.items()}
    for name, r in out.items():
        print("%-8s fwd us by band %.1f by channel group %.1f | torch fwd in grad mode %.1f | a one-block call %.1f"
              % (name, 1e3 * r["fwd_kernel"]["median_ms"], 1e3 * r["fwd_kernel_channel_split"]["median_ms"],
                 1e3 * r["fwd_grad_torch"]["median_ms"], 1e3 * r["one_block_call"]["median_ms"]))
        print("%-8s step ms fused %.3f [%.3f .. %.3f] torch %.3f [%.3f .. %.3f] | fwd us kernel %.1f torch %.1f | bwd us kernel "
              "%.1f torch %.1f" % (name, r["step_fused"]["median_ms"], r["step_fused"]["min_ms"], r["step_fused"]["max_ms"],
                                   r["step_torch"]["median_ms"], r["step_torch"]["min_ms"], r["step_torch"]["max_ms"],
                                   1e3 * r["fwd_kernel"]["median_ms"], 1e3 * r["fwd_torch"]["median_ms"],
                                   1e3 * r["bwd_kernel"]["median_ms"], 1e3 * r["bwd_torch"]["median_ms"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
