#!/usr/bin/env python3
"""Time DSSM's train step on its two routes against the same net written as a torch chain on the same GPU (autograd +
torch.optim.Adam), layer 0 on the sparse kernels against rec_gemm_f32 and its weight-gradient form, and the head kernel
against the torch ops it replaces.

    python tools/dssm_bench.py [--out dssm_bench.json] [--rounds 5] [--iters 20] [--B 8 128 1024] [--neg 1 4]

"sparse" is the step on a batch as reader.DssmReader yields it (CSR with row_of and the entries grouped by column, made on the
host where the lines are parsed); "sparse_device_group" the same step on a bare CSR feed, which sorts on the device.

The shipped configuration (trigram_d 2900, fc_sizes [300, 300, 128], all ReLU, slice_end 8) with one and four negatives at
B 8 (config.yaml's batch), 128 and 1024.  A row sets 3 to 13 distinct columns to 1.0, uniform draws (the reference's sample
files hold 1 to 37 a field, 6.9 on average).  Every time is device time between two events around a window of back-to-back
calls that lasts at least 0.3 s (the call count comes from a probe, which is also the warm-up; `--iters` is its floor); the
candidates alternate within a round, and the spread over the rounds (min .. max of the per-round means) is reported beside
the median.  A window of calls to ONE entry point of 10 - 20 us is paced by the host's enqueue rate as much as by the kernel:
such a figure is an upper bound of the kernel's time.  Peak memory is torch's allocator peak above what was resident before
the step.  A run without a GPU fails: there is no fallback.

The torch chain restates net.py's forward and dygraph_model.py's loss op by op (two towers of Linear + ReLU over dense
[B, 2900] inputs, the document tower called once per field, the clamped cosine, concat, softmax, slice, -log, mean) because
that is what a user of the reference pays; it is written here and shares no text with the reference."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, SIZES, SLICE_END, LR = 2900, [300, 300, 128], 8, 0.001
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


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20


class TorchChain(torch.nn.Module):
    def __init__(self, dev):
        super().__init__()
        h = [T] + SIZES
        tower = lambda: torch.nn.ModuleList(torch.nn.Linear(a, b, device=dev) for a, b in zip(h[:-1], h[1:]))
        self.query, self.doc = tower(), tower()

    @staticmethod
    def run(tower, x):
        for lin in tower:
            x = torch.relu(lin(x))
        return x

    @staticmethod
    def cosine(x, y):
        return (x * y).sum(1) / torch.sqrt(torch.clamp((x * x).sum(1) * (y * y).sum(1), min=1e-16))

    def head(self, q, docs):
        prob = torch.softmax(torch.stack([self.cosine(q, d) for d in docs], 1), 1)
        return (-torch.log(prob[:SLICE_END, 0:1]).sum(-1)).mean()

    def forward(self, fields):
        return self.head(self.run(self.query, fields[0]), [self.run(self.doc, f) for f in fields[1:]])


def make_fields(B, neg, seed):
    """(2 + neg) fields of B multi-hot rows with 3 to 13 entries -> (dense float32 arrays, [query, docs] CSR numpy tuples with the
    reader's row_of and column grouping)."""
    from paddlerec_amd.reader import dssm_csr, dssm_group
    rng = np.random.default_rng(seed)
    fields = []
    for _ in range(2 + neg):
        x = np.zeros((B, T), np.float32)
        for r in range(B):
            x[r, rng.choice(T, int(rng.integers(3, 14)), replace=False)] = 1.0
        fields.append(x)
    csr = [dssm_csr(list(fields[0])), dssm_csr([r for f in fields[1:] for r in f])]
    return fields, [c + dssm_group(c[0], T) for c in csr]               # as reader.DssmReader yields a batch


def layer(dev):
    from paddlerec_amd.dssm import DSSMLayer
    return DSSMLayer(T, 1, SLICE_END, SIZES, ["relu"] * 3, device=dev)


def entry_times(entries, rounds, iters):
    out = {}
    with torch.no_grad():
        calls = {k: calls_for(f, iters) for k, f in entries.items()}
        times = {k: [] for k in entries}
        for _ in range(rounds):
            for k, f in entries.items():
                times[k].append(timed(f, calls[k]))
    for k in entries:
        out[k] = {n.replace("_ms", "_us"): v * 1000 for n, v in stats(times[k]).items()}
        out[k]["calls_per_window"] = calls[k]
    return out


def bench_shape(B, neg, rounds, iters, dev):
    from paddlerec_amd import ops
    fields, csr = make_fields(B, neg, B * 10 + neg)
    dense = [torch.from_numpy(f).to(dev) for f in fields]
    sparse = [tuple(torch.from_numpy(a).to(dev) for a in x) for x in csr]
    nnz = int(csr[0][0].size + csr[1][0].size)
    bare = [x[:3] for x in sparse]                                # a feed without row_of and grouping: both made on the device
    ms, md, mg = layer(dev), layer(dev), layer(dev)
    chain = TorchChain(dev)
    opt = torch.optim.Adam(chain.parameters(), lr=LR)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        chain(dense).backward()
        opt.step()

    steps = {"sparse": lambda: ms.train_step(sparse, LR), "sparse_device_group": lambda: md.train_step(bare, LR),
             "general": lambda: mg.train_step(dense, LR), "torch": torch_step}
    out = dict(B=B, neg=neg, nnz=nnz, peak_mb={k: peak_of(f, dev) for k, f in steps.items()})
    assert ms._last["sparse"] and not mg._last["sparse"]
    calls = {k: calls_for(f, iters if k != "torch" else 5) for k, f in steps.items()}
    out["calls_per_window"] = calls
    times = {k: [] for k in steps}
    for _ in range(rounds):                                   # alternate: other work shares the host
        for k, f in steps.items():
            times[k].append(timed(f, calls[k]))
    out["train_step"] = {k: stats(v) for k, v in times.items()}
    # layer 0 of the document tower alone: the sparse kernels against the GEMM and its weight-gradient form
    p, g = ms.store.view["p"], ms.store.view["g"]
    W, b, gW, gb = p["pos_linear_0.weight"], p["pos_linear_0.bias"], g["pos_linear_0.weight"], g["pos_linear_0.bias"]
    cols, vals, lod, row_of = sparse[1][:4]
    host_groups = ops.IdGroups(0, dev)
    host_groups.n, host_groups.sorted_pos, host_groups.uniq_rows, host_groups.seg_offset, host_groups.n_uniq = cols.numel(), *sparse[1][4:]
    X = torch.cat(dense[1:], 0)
    R = X.shape[0]
    y = torch.empty(R, SIZES[0], device=dev)
    dY = torch.randn(R, SIZES[0], device=dev)
    ws, wsg = ops.Workspace(dev), ops.Workspace(dev)
    groups = ops.IdGroups(cols.numel(), dev)
    status = ops.new_status(dev)

    def sparse_bwd():
        ops.colsum(dY, ws, out=gb)
        ops.ids_group(cols, T, None, wsg, None, status, groups)
        ops.dssm_sparse_linear_bwd(vals, row_of, groups, dY, gW)

    entries = {
        "layer0_fwd_sparse": lambda: ops.dssm_sparse_linear_fwd(cols, vals, lod, W, b, relu=True, status=status, out=y),
        "layer0_fwd_gemm": lambda: ops.gemm(X, W, ws, epilogue="bias_relu", bias=b, out=y),
        "layer0_bwd_sparse_device_group": sparse_bwd,
        "layer0_bwd_sparse_reader_group": lambda: (ops.colsum(dY, ws, out=gb), ops.dssm_sparse_linear_bwd(vals, row_of, host_groups, dY, gW)),
        "layer0_bwd_sparse_kernel_alone": lambda: ops.dssm_sparse_linear_bwd(vals, row_of, groups, dY, gW),
        "layer0_bwd_gemm": lambda: ops.gemm(X, dY, ws, trans_a=True, out=gW, b_colsum=gb),
    }
    q = torch.relu(torch.randn(B, SIZES[-1], device=dev))
    d = torch.relu(torch.randn((1 + neg) * B, SIZES[-1], device=dev))
    head_out = ops.dssm_head_step(q, d, SLICE_END, relu_mask=True)
    entries["head_kernel"] = lambda: ops.dssm_head_step(q, d, SLICE_END, relu_mask=True, out=head_out)
    out["entries_us"] = entry_times(entries, rounds, iters)
    qg, dg = q.clone().requires_grad_(True), d.clone().requires_grad_(True)

    def torch_head():
        qg.grad = dg.grad = None
        chain.head(qg, list(dg.view(1 + neg, B, -1).unbind(0))).backward()

    n = calls_for(torch_head, 5)
    out["entries_us"]["head_torch_fwd_bwd"] = {k.replace("_ms", "_us"): v * 1000
                                               for k, v in stats([timed(torch_head, n) for _ in range(rounds)]).items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--B", type=int, nargs="*", default=[8, 128, 1024])
    ap.add_argument("--neg", type=int, nargs="*", default=[1, 4])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dssm_bench needs a GPU: there is no CPU measurement path")
    dev = torch.device("cuda")
    res = dict(net=dict(trigram_d=T, fc_sizes=SIZES, slice_end=SLICE_END), inputs="3 to 13 uniform columns a row, all 1.0",
               results=[bench_shape(B, neg, args.rounds, args.iters, dev) for neg in args.neg for B in args.B])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
