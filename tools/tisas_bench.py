#!/usr/bin/env python3
"""Time TiSASRec's new entry points and its train step on the GPU against the torch chain that mirrors the reference
(models/recall/tisas/net.py: the relation tensors time_matrix_K / time_matrix_V materialised as [B, L, L, D], dropout applied
to them element by element, autograd for the backward, torch.optim.Adam), and report the peak memory of both.

    python tools/tisas_bench.py [--batch 128 1024] [--iters 30] [--out tisas_bench.json]

Shape: L 50, D 50, H 1, T 257 (the shipped big-data config), 2 blocks, with dropout 0.2 and without.  Times are device-event
times over `iters` calls after a warm-up, the median of 5 windows; the torch chain and the HIP path alternate window by window.
Peak memory is torch.cuda.max_memory_allocated during one train step minus what was allocated before it (parameters, optimizer
state and the batch are resident in both).  The masks differ between the two (torch's generator against the counter-based
streams) and so do the two random initialisations: the losses printed are a sanity figure, not a comparison.  One JSON line per
(batch, dropout) goes to stdout and, with --out, into a file."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, D, H, T, BLOCKS, ITEMS = 50, 50, 1, 257, 2, 3416
NEG = float(-2 ** 32 + 1)


def batch_of(B, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, ITEMS + 1, (B, L), generator=g)
    pad = torch.randint(0, L // 2, (B, 1), generator=g)
    seq = seq * (torch.arange(L)[None, :] >= pad)
    ts = torch.cumsum(torch.randint(0, 30, (B, L), generator=g), 1) * (seq != 0)
    tm = (ts[:, :, None] - ts[:, None, :]).abs().clamp(max=T - 1)
    pos = torch.randint(1, ITEMS + 1, (B, L), generator=g) * (seq != 0)
    neg = torch.randint(1, ITEMS + 1, (B, L), generator=g) * (seq != 0)
    return [t.to(dev).contiguous() for t in (seq, tm, pos, neg)]


class TorchChain(torch.nn.Module):
    """net.py's TiSASRecLayer with torch modules, H = 1 (no split / concat), relation tensors materialised."""

    def __init__(self, p_drop):
        super().__init__()
        nn = torch.nn
        self.item_emb = nn.Embedding(ITEMS + 1, D, padding_idx=0)
        self.pos_k, self.pos_v = nn.Embedding(L, D), nn.Embedding(L, D)
        self.time_k, self.time_v = nn.Embedding(T, D), nn.Embedding(T, D)
        self.drop = nn.Dropout(p_drop)
        self.ln_a = nn.ModuleList(nn.LayerNorm(D, eps=1e-8) for _ in range(BLOCKS))
        self.ln_f = nn.ModuleList(nn.LayerNorm(D, eps=1e-8) for _ in range(BLOCKS))
        self.qkv = nn.ModuleList(nn.ModuleList(nn.Linear(D, D) for _ in range(3)) for _ in range(BLOCKS))
        self.conv = nn.ModuleList(nn.ModuleList(nn.Conv1d(D, D, 1) for _ in range(2)) for _ in range(BLOCKS))
        self.last = nn.LayerNorm(D, eps=1e-8)

    def attention(self, n, Q, S, pad_row, causal, TK, TV, PK, PV):
        q, k, v = self.qkv[n][0](Q), self.qkv[n][1](S), self.qkv[n][2](S)
        w = q @ k.transpose(1, 2) + q @ PK.transpose(1, 2) + (TK @ q.unsqueeze(-1)).squeeze(-1)
        w = w / math.sqrt(D // H)
        w = torch.where(pad_row, torch.full_like(w, NEG), w)
        w = torch.where(causal, torch.full_like(w, NEG), w)
        w = self.drop(torch.softmax(w, -1))
        return w @ v + w @ PV + (w.unsqueeze(2) @ TV).squeeze(2)

    def forward(self, seq, tm, pos, neg):
        B = seq.shape[0]
        keep = (seq != 0).unsqueeze(-1).float()
        x = self.drop(self.item_emb(seq) * math.sqrt(D)) * keep
        ar = torch.arange(L, device=seq.device).unsqueeze(0).expand(B, -1)
        PK, PV = self.drop(self.pos_k(ar)), self.drop(self.pos_v(ar))
        TK, TV = self.drop(self.time_k(tm)), self.drop(self.time_v(tm))           # the two [B, L, L, D] relation tensors
        pad_row = (seq == 0).unsqueeze(-1).expand(-1, -1, L)
        causal = (torch.tril(torch.ones(L, L, device=seq.device)) == 0).unsqueeze(0).expand(B, -1, -1)
        for n in range(BLOCKS):
            Q = self.ln_a[n](x)
            x = Q + self.attention(n, Q, x, pad_row, causal, TK, TV, PK, PV)
            x = self.ln_f[n](x)
            y = self.drop(self.conv[n][1](torch.relu(self.drop(self.conv[n][0](x.transpose(1, 2)))))).transpose(1, 2)
            x = (y + x) * keep
        f = self.last(x)
        pl, nl = (f * self.item_emb(pos)).sum(-1), (f * self.item_emb(neg)).sum(-1)
        m = pos != 0
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        return bce(pl[m], torch.ones_like(pl[m])) + bce(nl[m], torch.zeros_like(nl[m]))


def windows(fns, iters, reps=5):
    """{name: median ms per call} — the functions alternate window by window.  A call that takes long gets fewer calls per
    window (a window is about 0.2 s at the most, at least one call)."""
    import time
    n_of = {}
    for k, f in fns.items():
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        t0 = time.time()
        f()
        torch.cuda.synchronize()
        n_of[k] = max(1, min(iters, int(0.2 / max(time.time() - t0, 1e-6))))
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            iters = n_of[k]
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / iters)
    return {k: statistics.median(v) for k, v in times.items()}


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20


def entry_points(B, p, dev, iters):
    """Each new entry point alone against the torch ops it replaces (forward and backward of that piece)."""
    from paddlerec_amd import ops
    seq, tm, pos, neg = batch_of(B, dev)
    n = B * L
    f = lambda *s: torch.randn(*s, device=dev)
    q, k, v, d_out = f(n, D), f(n, D), f(n, D), f(n, D)
    tables = [0.1 * f(L, D), 0.1 * f(L, D), 0.1 * f(T, D), 0.1 * f(T, D)]
    d_tables = [torch.empty_like(t) for t in tables]
    probs, scale, scratch = (p, p, p), 1.0 / math.sqrt(D // H), {}
    out, lse = ops.tisas_attn_fwd(q, k, v, tables, tm, seq, H, scale, probs, 1, (1, 2, 3, 4, 5))
    table = 0.1 * f(ITEMS + 1, D)
    gamma, beta, dg, db = torch.ones(D, device=dev), torch.zeros(D, device=dev), torch.empty(D, device=dev), torch.empty(D, device=dev)
    ids = seq.view(-1)
    y, mean, rstd = ops.affine_layer_norm_fwd(q, gamma, beta, 1e-8, r=k, row_ids=ids, sum_out=v.clone())
    # torch counterparts of the attention: relation tensors, dropout, autograd
    tq, tk, tv = (t.view(B, L, D).clone().requires_grad_() for t in (q, k, v))
    tt = [t.clone().requires_grad_() for t in tables]
    drop = torch.nn.Dropout(p)
    pad_row = (seq == 0).unsqueeze(-1).expand(-1, -1, L)
    causal = (torch.tril(torch.ones(L, L, device=dev)) == 0).unsqueeze(0).expand(B, -1, -1)

    def torch_attn_fwd():
        PK, PV = drop(tt[0].unsqueeze(0).expand(B, -1, -1)), drop(tt[1].unsqueeze(0).expand(B, -1, -1))
        TK, TV = drop(torch.nn.functional.embedding(tm, tt[2])), drop(torch.nn.functional.embedding(tm, tt[3]))
        w = (tq @ tk.transpose(1, 2) + tq @ PK.transpose(1, 2) + (TK @ tq.unsqueeze(-1)).squeeze(-1)) * scale
        w = torch.where(causal, torch.full_like(w, NEG), torch.where(pad_row, torch.full_like(w, NEG), w))
        w = drop(torch.softmax(w, -1))
        return w @ tv + w @ PV + (w.unsqueeze(2) @ TV).squeeze(2)

    def torch_attn_fwd_bwd():
        torch.autograd.grad(torch_attn_fwd(), [tq, tk, tv] + tt, d_out.view(B, L, D))

    ln = torch.nn.LayerNorm(D, eps=1e-8).to(dev)
    xq = q.clone().requires_grad_()
    keep = (ids != 0).unsqueeze(-1).float()

    def torch_ln_fwd_bwd():
        torch.autograd.grad(ln((xq + k) * keep), [xq] + list(ln.parameters()), d_out)

    emb_w = table.clone().requires_grad_()

    def torch_embed_fwd_bwd():
        o = drop(torch.nn.functional.embedding(seq, emb_w, padding_idx=0) * math.sqrt(D)) * (seq != 0).unsqueeze(-1)
        torch.autograd.grad(o, emb_w, d_out.view(B, L, D))

    feats = q.clone().requires_grad_()
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def torch_head():
        pe, ne = torch.nn.functional.embedding(pos, emb_w, padding_idx=0), torch.nn.functional.embedding(neg, emb_w, padding_idx=0)
        pl, nl = (feats.view(B, L, D) * pe).sum(-1), (feats.view(B, L, D) * ne).sum(-1)
        m = pos != 0
        loss = bce(pl[m], torch.ones_like(pl[m])) + bce(nl[m], torch.zeros_like(nl[m]))
        torch.autograd.grad(loss, [feats, emb_w])

    G = torch.empty(2 * n, D, device=dev)
    fns = {
        "attn_fwd hip": lambda: ops.tisas_attn_fwd(q, k, v, tables, tm, seq, H, scale, probs, 1, (1, 2, 3, 4, 5), out=out),
        "attn_fwd torch": lambda: torch_attn_fwd(),
        "attn_fwd+bwd hip": lambda: (ops.tisas_attn_fwd(q, k, v, tables, tm, seq, H, scale, probs, 1, (1, 2, 3, 4, 5), out=out),
                                     ops.tisas_attn_bwd(q, k, v, tables, tm, seq, H, scale, lse, d_out, d_tables, probs, 1,
                                                        (1, 2, 3, 4, 5), scratch=scratch)),
        "attn_fwd+bwd torch": torch_attn_fwd_bwd,
        "layer_norm fwd+bwd hip": lambda: (ops.affine_layer_norm_fwd(q, gamma, beta, 1e-8, r=k, row_ids=ids, sum_out=v, out=y),
                                           ops.affine_layer_norm_bwd(v, mean, rstd, gamma, d_out, dg, db, row_ids=ids, out=out)),
        "layer_norm fwd+bwd torch": torch_ln_fwd_bwd,
        "embed fwd+bwd hip": lambda: (ops.tisas_embed_fwd(ids, table, math.sqrt(D), p, 1, 9, out=y),
                                      ops.tisas_embed_bwd(ids, d_out, ITEMS + 1, math.sqrt(D), p, 1, 9, out=out)),
        "embed fwd+bwd torch": torch_embed_fwd_bwd,
        "head hip": lambda: ops.tisas_head(q, pos.view(-1), neg.view(-1), table, d_pos_rows=G[:n], d_neg_rows=G[n:]),
        "head torch": torch_head,
    }
    res = windows(fns, iters)
    res["attn_fwd+bwd peak MB hip"] = peak_of(fns["attn_fwd+bwd hip"], dev)
    res["attn_fwd+bwd peak MB torch"] = peak_of(fns["attn_fwd+bwd torch"], dev)
    return res


def attn_fwd_only(B, p, dev, iters):
    from paddlerec_amd import ops
    seq, tm, _, _ = batch_of(B, dev)
    f = lambda *s: torch.randn(*s, device=dev)
    q, k, v, out = f(B * L, D), f(B * L, D), f(B * L, D), f(B * L, D)
    tables = [0.1 * f(L, D), 0.1 * f(L, D), 0.1 * f(T, D), 0.1 * f(T, D)]
    fn = lambda: ops.tisas_attn_fwd(q, k, v, tables, tm, seq, H, 1.0 / math.sqrt(D // H), (p, p, p), 1, (1, 2, 3, 4, 5), out=out)
    return windows({"attn_fwd": fn}, iters)["attn_fwd"]


def train_steps(B, p, dev, iters):
    from paddlerec_amd.tisas import TiSASRecLayer
    feeds = batch_of(B, dev)
    torch.manual_seed(5)
    m = TiSASRecLayer(6040, ITEMS, D, L, T - 1, BLOCKS, H, dropout_rate=p, device=dev)
    t = TorchChain(p).to(dev)
    opt = torch.optim.Adam(t.parameters(), lr=0.001, betas=(0.9, 0.98))

    def torch_step():
        opt.zero_grad(set_to_none=True)
        loss = t(*feeds)
        loss.backward()
        opt.step()
        return loss

    hip_step = lambda: m.train_step(*feeds)[0]
    res = {"train_step peak MB hip": peak_of(hip_step, dev), "train_step peak MB torch": peak_of(torch_step, dev)}
    res.update(windows({"train_step hip": hip_step, "train_step torch": torch_step}, iters))
    res["loss hip"], res["loss torch"] = float(hip_step().item()), float(torch_step().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[128, 1024])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--dropout", type=float, nargs="*", default=[0.0, 0.2])
    ap.add_argument("--only-attn-fwd", action="store_true", help="time rec_tisas_attn_fwd alone (comparing two builds)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tisas_bench measures on the GPU; none found")
    dev = torch.device("cuda")
    lines = []
    for B in args.batch:
        for p in args.dropout:
            if args.only_attn_fwd:
                print(json.dumps(dict(batch=B, dropout=p, attn_fwd_ms=round(attn_fwd_only(B, p, dev, args.iters), 4))), flush=True)
                continue
            rec = dict(batch=B, L=L, D=D, H=H, T=T, blocks=BLOCKS, dropout=p, relation_tensors_MB=2 * B * L * L * D * 4 / 2 ** 20)
            rec.update({k: round(v, 4) for k, v in entry_points(B, p, dev, args.iters).items()})
            rec.update({k: round(v, 4) for k, v in train_steps(B, p, dev, args.iters).items()})
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
