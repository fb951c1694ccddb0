#!/usr/bin/env python3
"""Time ENSFM's entry points and its whole train step against the reference's formulation written as a torch chain on the
same GPU (autograd + torch.optim.Adagrad over dense tables), and the dense alternative for the positives.

    python tools/ensfm_bench.py [--out ensfm_bench.json] [--rounds 5] [--iters 20]

Shapes: B 512, D 64, Fu 4, Fi 2, I 3706, tables sized by the shipped config_bigdata.yaml (6069 / 3953), with P 256 and
P 2048.  The positive lists are SYNTHETIC (uniform lengths in [P / 8, P], uniform items): full ML-1M is not available, so the
real I and P are not measured.  Every time is device time between two events around a window of back-to-back calls that
lasts at least 0.3 s (the call count comes from a probe, which is also the warm-up; `--iters` is its floor); the fused step
and the torch chain alternate within a round, and the spread over the rounds (min .. max of the per-round means) is reported
beside the median.  A window of calls to ONE entry point of 10 - 20 us is paced by the host's enqueue rate as much as by the
kernel: such a figure is an upper bound of the kernel's time, and comparisons between two of them carry that uncertainty.  Peak memory is torch's allocator peak above what was resident before
the step.  A run without a GPU fails: there is no fallback.

The torch chain (`TorchChain`) restates net.py:63-98 and dygraph_model.py:40-51 op by op — the [B, I+1, C] `dot`, the three
[B, P, C] tensors, the two outer-product stacks — because that is the cost a user of the reference pays; it is written here
and shares no text with the reference.
The dense alternative for entry points 4-5 (`dense_positives`): a [B, I+1] count matrix of the lists, pre = (p o h) q^T and
two more GEMMs (rocBLAS through torch.matmul), which is what the list form competes with when P is a large part of I."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, D, FU, FI, I, USERS, ITEMS, W, LR = 512, 64, 4, 2, 3706, 6069, 3953, 0.5, 0.05


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


def feeds(P, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, USERS, (B, FU), generator=g)
    attr = torch.randint(0, ITEMS, (I + 1, FI), generator=g)
    attr[I] = attr[0]
    ur = torch.randint(0, I, (B, P), generator=g)
    ur[torch.arange(P)[None, :] >= torch.randint(P // 8, P + 1, (B, 1), generator=g)] = I
    return u.to(dev), attr.to(dev), ur.to(dev)


class TorchChain(torch.nn.Module):
    def __init__(self, dev):
        super().__init__()
        tn = lambda *sh: torch.nn.Parameter(torch.nn.init.trunc_normal_(torch.empty(*sh, device=dev), std=0.01, a=-0.02, b=0.02))
        self.U, self.V, self.ub, self.ib = tn(USERS, D), tn(ITEMS + 1, D), tn(USERS, 1), tn(ITEMS, 1)
        self.H_i = torch.nn.Parameter(torch.full((D, 1), 0.01, device=dev))
        self.H_s = torch.nn.Parameter(torch.full((D, 1), 0.01, device=dev))
        self.bias = torch.nn.Parameter(torch.zeros(1, device=dev))

    def forward(self, u, attr, ur):
        ue, ve = self.U[u], self.V[attr]
        su, sv = ue.sum(1), ve.sum(1)
        uc, ic = 0.5 * (su ** 2 - (ue ** 2).sum(1)), 0.5 * (sv ** 2 - (ve ** 2).sum(1))
        one = lambda n: torch.ones(n, 1, device=u.device)
        p = torch.cat([su, uc @ self.H_s + self.ub[u].sum(1) + self.bias, one(len(u))], 1)
        q = torch.cat([sv, one(len(attr)), ic @ self.H_s + self.ib[attr].sum(1)], 1)
        h = torch.cat([self.H_i, one(2)], 0)
        dot = torch.einsum("ac,bc->abc", p, q)
        pre = torch.einsum("ajk,kl->aj", dot, h)
        pos_item = torch.nn.functional.embedding(ur, q)
        pos_item = torch.einsum("ab,abc->abc", (ur != I).float(), pos_item)
        pos_r = torch.einsum("ac,abc->abc", p, pos_item)
        pos_r = torch.einsum("ajk,kl->ajl", pos_r, h).flatten(1)
        return pre, pos_r, q, p, h

    def loss(self, out):
        _, pos_r, q, p, h = out
        loss = W * ((torch.einsum("ab,ac->abc", q, q).sum(0) * torch.einsum("ab,ac->abc", p, p).sum(0) * (h @ h.t())).sum(0)).sum(0)
        return loss + ((1.0 - W) * pos_r ** 2 - 2.0 * pos_r).sum()


def dense_positives(p, q, h, cnt):
    """Entry points 4-5 in the dense form: g over ALL (b, i), weighted by the count matrix; three GEMMs."""
    ph = p * h
    pre = ph @ q.t()
    gm = cnt * (2.0 * (1.0 - W) * pre - 2.0)
    return (gm @ q) * h, (gm.t() @ p) * h, ((1.0 - W) * cnt * pre * pre - 2.0 * cnt * pre).sum()


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20


def bench_shape(P, rounds, iters, dev):
    from paddlerec_amd import ops
    from paddlerec_amd.ensfm import ENSFMLayer
    u, attr, ur = feeds(P, dev)
    m = ENSFMLayer(USERS, ITEMS, D, device=dev)
    chain = TorchChain(dev)
    opt = torch.optim.Adagrad(chain.parameters(), lr=LR, eps=1e-6, initial_accumulator_value=1e-8)

    def fused():
        m.train_step(u, attr, ur, lr=LR, negative_weight=W)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        chain.loss(chain(u, attr, ur)).backward()
        opt.step()

    out = dict(P=P, peak_fused_mb=peak_of(fused, dev), peak_torch_mb=peak_of(torch_step, dev))
    n_fused, n_torch = calls_for(fused, iters), calls_for(torch_step, 5)
    out["calls_per_window"] = dict(fused=n_fused, torch=n_torch)
    a, b = [], []
    for _ in range(rounds):                                   # alternate: other work shares the host
        a.append(timed(fused, n_fused))
        b.append(timed(torch_step, n_torch))
    out["train_step_fused"], out["train_step_torch"] = stats(a), stats(b)
    # the entry points on their own, at this shape
    k, t, pr = ops, m.tables, m.params
    p_emb, q_emb = m._towers(u, attr)
    G_p, G_q = k.ensfm_gram(p_emb), k.ensfm_gram(q_emb)
    gpos, dP, lp, dhp, _ = k.ensfm_pos_user(ur, p_emb, q_emb, pr["H_i"], G_q, W)
    groups, _ = k.ids_group(ur.view(-1), I + 1, I, k.Workspace(dev))
    ws, sc = k.Workspace(dev), {}
    dQ = k.ensfm_pos_item(groups, gpos, p_emb, q_emb, pr["H_i"], G_p, W)
    dHs, db = torch.empty(D, device=dev), torch.empty(1, device=dev)
    entries = {
        "tower_fwd_user": lambda: k.ensfm_tower_fwd(u, t["user_feature_emb.weight"], t["user_bias.weight"], pr["H_s"], pr["bias"], out=p_emb),
        "tower_fwd_item": lambda: k.ensfm_tower_fwd(attr, t["all_item_feature_emb.weight"], t["item_bias.weight"], pr["H_s"], None, True, out=q_emb),
        "gram_p": lambda: k.ensfm_gram(p_emb, sc, G_p), "gram_q": lambda: k.ensfm_gram(q_emb, sc, G_q),
        "pos_user": lambda: k.ensfm_pos_user(ur, p_emb, q_emb, pr["H_i"], G_q, W),
        "ids_group_ur": lambda: k.ids_group(ur.view(-1), I + 1, I, ws, None, None, groups),
        "pos_item": lambda: k.ensfm_pos_item(groups, gpos, p_emb, q_emb, pr["H_i"], G_p, W, out=dQ),
        "loss": lambda: k.ensfm_loss(G_p, G_q, pr["H_i"], lp, dhp, W, B),
        "tower_bwd_user": lambda: k.ensfm_tower_bwd(u, t["user_feature_emb.weight"], pr["H_s"], dP, dHs, db, scratch=sc),
        "tower_bwd_item": lambda: k.ensfm_tower_bwd(attr, t["all_item_feature_emb.weight"], pr["H_s"], dQ, dHs, None, True, scratch=sc),
        "score": lambda: k.ensfm_score(p_emb, q_emb, pr["H_i"]),
    }
    h = torch.cat([pr["H_i"].view(-1), torch.ones(2, device=dev)])
    cnt = torch.zeros(B, I + 1, device=dev)
    cnt.scatter_add_(1, ur, (ur != I).float())
    cnt[:, I] = 0

    def count_matrix():
        c = torch.zeros(B, I + 1, device=dev)
        c.scatter_add_(1, ur, (ur != I).float())

    torch_entries = {
        "score": lambda: torch.einsum("ajk,k->aj", torch.einsum("ac,bc->abc", p_emb, q_emb), h),
        "gram_q": lambda: torch.einsum("ab,ac->abc", q_emb, q_emb).sum(0),
        "positives_dense_form": lambda: dense_positives(p_emb, q_emb, h, cnt),
        "positives_dense_count_matrix": count_matrix,
    }
    out["entries_us"] = {}
    for name, fn in list(entries.items()) + [("torch_" + n, f) for n, f in torch_entries.items()]:
        calls = calls_for(fn, iters)
        out["entries_us"][name] = {kk.replace("_ms", "_us"): v * 1000 for kk, v in stats([timed(fn, calls) for _ in range(rounds)]).items()}
        out["entries_us"][name]["calls_per_window"] = calls
    e = out["entries_us"]
    out["positives_list_form_us"] = e["pos_user"]["median_us"] + e["ids_group_ur"]["median_us"] + e["pos_item"]["median_us"]
    out["positives_dense_form_us"] = e["torch_positives_dense_form"]["median_us"] + e["torch_positives_dense_count_matrix"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--P", type=int, nargs="*", default=[256, 2048])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensfm_bench needs a GPU: there is no CPU measurement path")
    dev = torch.device("cuda")
    res = dict(shape=dict(B=B, D=D, Fu=FU, Fi=FI, I=I), lists="synthetic", results=[bench_shape(P, args.rounds, args.iters, dev) for P in args.P])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
