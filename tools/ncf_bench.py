#!/usr/bin/env python3
"""Time NCF's train step on its two routes against the same net written as a torch chain on the same GPU (autograd +
torch.optim.Adam over dense tables), and rec_ncf_step / rec_ncf_score alone.

    python tools/ncf_bench.py [--out ncf_bench.json] [--rounds 5] [--iters 20] [--B 256 65536]

The shipped configuration (NeuMF, mf_dim 8, fc_layers [64, 32, 16, 8], 6040 users, 3706 items) at B 256 (config_bigdata.yaml's
batch) and at one large batch, B 65 536; ids and labels are uniform draws (full MovieLens is not available here).  Every time
is device time between two events around a window of back-to-back calls that lasts at least 0.3 s (the call count comes from
a probe, which is also the warm-up; `--iters` is its floor); the three steps alternate within a round, and the spread over
the rounds (min .. max of the per-round means) is reported beside the median.  A window of calls to ONE entry point of 10 -
20 us is paced by the host's enqueue rate as much as by the kernel: such a figure is an upper bound of the kernel's time.
Peak memory is torch's allocator peak above what was resident before the step.  A run without a GPU fails: there is no
fallback.

The torch chain restates net.py's NeuMF forward and dygraph_model.py's loss op by op (four nn.Embedding, the concat, three
Linear + ReLU, the head, sigmoid, the log loss with epsilon 1e-4) because that is what a user of the reference pays; it is
written here and shares no text with the reference."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

USERS, ITEMS, MF, LAYERS, LR = 6040, 3706, 8, [64, 32, 16, 8], 0.001
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
    """How many back-to-back calls fill WINDOW_S, from a short probe (which is also the warm-up of the shape)."""
    per_call_ms = max(timed(fn, max(floor, 5)), 1e-3)
    return int(min(max(floor, WINDOW_S * 1000.0 / per_call_ms), 100000))


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs))


class TorchChain(torch.nn.Module):
    def __init__(self, dev):
        super().__init__()
        emb = lambda n, d: torch.nn.Embedding(n, d, device=dev)
        self.mf_u, self.mf_i, self.mlp_u, self.mlp_i = emb(USERS, MF), emb(ITEMS, MF), emb(USERS, LAYERS[0] // 2), emb(ITEMS, LAYERS[0] // 2)
        self.tower = torch.nn.ModuleList(torch.nn.Linear(a, b, device=dev) for a, b in zip(LAYERS[:-1], LAYERS[1:]))
        self.prediction = torch.nn.Linear(MF + LAYERS[-1], 1, device=dev)

    def forward(self, u, i):
        x = torch.cat([self.mlp_u(u), self.mlp_i(i)], -1)
        for lin in self.tower:
            x = torch.relu(lin(x))
        return torch.sigmoid(self.prediction(torch.cat([self.mf_u(u) * self.mf_i(i), x], -1)))

    def loss(self, pred, y):
        return (-y * torch.log(pred + 1e-4) - (1 - y) * torch.log(1 - pred + 1e-4)).mean()


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20


def layer(dev, fused):
    from paddlerec_amd.ncf import NCFLayer
    old = os.environ.get("REC_NCF_FUSED")
    os.environ["REC_NCF_FUSED"] = "1" if fused else "0"
    try:
        m = NCFLayer(USERS, ITEMS, MF, LAYERS, "NCF_NeuMF", device=dev)
    finally:
        if old is None:
            del os.environ["REC_NCF_FUSED"]
        else:
            os.environ["REC_NCF_FUSED"] = old
    assert m.fused == fused
    return m


def bench_shape(B, rounds, iters, dev):
    from paddlerec_amd import ops
    g = torch.Generator().manual_seed(1)
    u, i, y = (torch.randint(0, n, (B,), generator=g).to(dev) for n in (USERS, ITEMS, 2))
    yf = y.float().view(-1, 1)
    mf, mg = layer(dev, True), layer(dev, False)
    chain = TorchChain(dev)
    opt = torch.optim.Adam(chain.parameters(), lr=LR)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        chain.loss(chain(u, i), yf).backward()
        opt.step()

    steps = {"fused": lambda: mf.train_step(u, i, y, LR), "general": lambda: mg.train_step(u, i, y, LR), "torch": torch_step}
    out = dict(B=B, peak_mb={k: peak_of(f, dev) for k, f in steps.items()})
    calls = {k: calls_for(f, iters if k != "torch" else 5) for k, f in steps.items()}
    out["calls_per_window"] = calls
    times = {k: [] for k in steps}
    for _ in range(rounds):                                   # alternate: other work shares the host
        for k, f in steps.items():
            times[k].append(timed(f, calls[k]))
    out["train_step"] = {k: stats(v) for k, v in times.items()}
    # the two fused entry points on their own, at this shape
    T, fl, sc = mf.packed["p"], mf.flat, {}
    pred, gu, gi, loss = ops.ncf_step(mf.desc, u, i, y, T["user"], T["item"], fl["p"], fl["g"], scratch=sc)
    entries = {
        "ncf_step": lambda: ops.ncf_step(mf.desc, u, i, y, T["user"], T["item"], fl["p"], fl["g"], pred=pred, g_user=gu, g_item=gi,
                                         loss=loss, scratch=sc),
        "ncf_score": lambda: ops.ncf_score(mf.desc, u, i, T["user"], T["item"], fl["p"], pred=pred),
        "torch_forward": lambda: chain(u, i),
    }
    out["entries_us"] = {}
    with torch.no_grad():
        for name, fn in entries.items():
            n = calls_for(fn, iters)
            out["entries_us"][name] = {k.replace("_ms", "_us"): v * 1000 for k, v in stats([timed(fn, n) for _ in range(rounds)]).items()}
            out["entries_us"][name]["calls_per_window"] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--B", type=int, nargs="*", default=[256, 65536])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ncf_bench needs a GPU: there is no CPU measurement path")
    dev = torch.device("cuda")
    res = dict(net=dict(users=USERS, items=ITEMS, mf_dim=MF, fc_layers=LAYERS, mode="NCF_NeuMF"), ids="uniform draws",
               results=[bench_shape(B, args.rounds, args.iters, dev) for B in args.B])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
