#!/usr/bin/env python3
"""BST's encoder kernels at the reference's shape — bst/config.yaml: batch 256, 6 heads of width 48 (d_model 288) — at
L 21, 102 (the sample data's longest history + 1) and 431, against torch's composition on the same GPU:
  * rec_mha_fwd / rec_mha_bwd on q, k, v as column ranges of one packed [B L, 864] projection against matmul, softmax,
    matmul on [B, H, L, d] views of the same buffer (forward; forward + autograd backward from a gradient on the output);
  * rec_add_layer_norm_fwd / _bwd on [B L, 288] against F.layer_norm(x + r) (forward; forward + autograd backward);
and one whole train step of paddlerec_amd.bst at the YAML's sizes (B 256, L 102, dropout 0.2, fc_sizes [1024, 512, 256]).
Times are device events around `n` back-to-back calls after a warm-up of the same shape; every figure is the median of
ROUNDS such windows with min .. max.  A run without a GPU fails.  Prints one JSON line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from paddlerec_amd import ops  # noqa: E402
from paddlerec_amd.bst import BSTLayer  # noqa: E402

DEV = "cuda"
B, H, D, ROUNDS = 256, 6, 48, 5
LENGTHS = (21, 102, 431)


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    return dict(ms=round(statistics.median(out), 4), min=round(min(out), 4), max=round(max(out), 4))


def bench_mha(L, res):
    g = torch.Generator(device=DEV).manual_seed(L)
    W = H * D
    qkv = torch.randn(B * L, 3 * W, device=DEV, generator=g) * 0.3
    q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
    d_out = torch.randn(B * L, W, device=DEV, generator=g)
    dqkv = torch.empty_like(qkv)
    grads = (dqkv[:, :W], dqkv[:, W:2 * W], dqkv[:, 2 * W:])
    out, lse = ops.mha_fwd(q, k, v, B, L, H)
    n = 20 if L < 400 else 5
    res["mha fwd fused L%d" % L] = timeit(lambda: ops.mha_fwd(q, k, v, B, L, H, out=out), n)
    res["mha bwd fused L%d" % L] = timeit(lambda: ops.mha_bwd(q, k, v, B, L, H, out, lse, d_out, grads=grads), n)
    res["mha fwd fused dropout 0.2 L%d" % L] = timeit(lambda: ops.mha_fwd(q, k, v, B, L, H, 1.0, 0.2, 1, 2, out=out), n)
    heads = lambda t: t.reshape(B, L, H, D).transpose(1, 2)

    def base(t):
        qq, kk, vv = heads(t[:, :W]), heads(t[:, W:2 * W]), heads(t[:, 2 * W:])
        return (torch.softmax(qq @ kk.transpose(-1, -2), -1) @ vv).transpose(1, 2).reshape(B * L, W)

    with torch.no_grad():
        res["mha fwd torch matmul softmax matmul L%d" % L] = timeit(lambda: base(qkv), n)
    tg = qkv.clone().requires_grad_(True)

    def base_fwd_bwd():
        tg.grad = None
        (base(tg) * d_out).sum().backward()

    res["mha fwd + bwd torch L%d" % L] = timeit(base_fwd_bwd, n)


def bench_ln(L, res):
    g = torch.Generator(device=DEV).manual_seed(L + 1)
    n = H * D
    x, r, dy = (torch.randn(B * L, n, device=DEV, generator=g) for _ in range(3))
    y, _, rstd = ops.add_layer_norm_fwd(x, r)
    dx = torch.empty_like(x)
    res["add+ln fwd fused L%d" % L] = timeit(lambda: ops.add_layer_norm_fwd(x, r, out=y))
    res["add+ln bwd fused L%d" % L] = timeit(lambda: ops.add_layer_norm_bwd(y, rstd, dy, out=dx))
    with torch.no_grad():
        res["add+ln fwd torch F.layer_norm(x + r) L%d" % L] = timeit(lambda: torch.nn.functional.layer_norm(x + r, (n,)))
    xg = x.clone().requires_grad_(True)

    def base_fwd_bwd():
        xg.grad = None
        (torch.nn.functional.layer_norm(xg + r, (n,)) * dy).sum().backward()

    res["add+ln fwd + bwd torch L%d" % L] = timeit(base_fwd_bwd)


def bench_step(res, L=102):
    torch.manual_seed(1)
    m = BSTLayer(192403, 96, 96, 96, "relu", True, True, 63001, 801, 5001, 1, 288, D, D, H, 0.2, "da", "da", 0.2, 512, 0.2,
                 [1024, 512, 256], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    T = L - 1
    ri = lambda hi, w: torch.randint(0, hi, (B, w), device=DEV, generator=g)
    feeds = [ri(192403, 1), ri(63001, T), ri(801, T), ri(5001, T), ri(63001, 1), ri(801, 1), ri(5001, 1)]
    label = ri(2, 1)
    res["train step B%d L%d" % (B, L)] = timeit(lambda: m.train_step(feeds, label), n=5)
    m.eval()
    res["infer step B%d L%d" % (B, L)] = timeit(lambda: m(*feeds), n=5)
    assert int(m.status.item()) == 0


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bst_bench needs a GPU")
    res = {}
    for L in LENGTHS:
        bench_mha(L, res)
        bench_ln(L, res)
    bench_step(res)
    for k, v in res.items():
        print("%-52s %9.4f ms  (%.4f .. %.4f)" % (k, v["ms"], v["min"], v["max"]), flush=True)
    print(json.dumps({"tool": "bst_bench", "B": B, "H": H, "d": D, "rounds": ROUNDS, "ms": res}))


if __name__ == "__main__":
    main()
