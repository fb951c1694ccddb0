#!/usr/bin/env python3
"""The fused GRU recurrence (rec_gru_seq_fwd / rec_gru_seq_bwd: one launch per time loop) at DIEN's shipped shape —
dien/config.yaml: batch 32, its sample file's longest history 152, H = 64 + 64 = 128 — and at one larger batch, against
  (a) the same recurrence as per-step launches of the existing GEMM: one rec_gemm_f32 per step (h W_hh^T + b_hh forward,
      dGh W_hh backward) timed ALONE — a lower bound of that form, which also needs a gate kernel per step — and, forward,
      with the gates as torch element-wise kernels on top;
  (b) torch.nn.GRU on the device (forward; forward + backward).
The input projection Gi = X W_ih^T + b_ih (one GEMM over B*T rows) is outside every fused / per-step figure and inside
torch.nn.GRU's.  Prints one line per measurement; device events around `n` back-to-back calls after a warm-up."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from paddlerec_amd import ops  # noqa: E402

DEV = "cuda"


def timeit(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def bench(B, T, H):
    g = torch.Generator(device=DEV).manual_seed(B)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    s = H ** -0.5
    X, W_ih, W_hh = rnd(B, T, H), rnd(3 * H, H) * s, rnd(3 * H, H) * s
    b_ih, b_hh, dH, dhT = rnd(3 * H) * s, rnd(3 * H) * s, rnd(B, T, H), rnd(B, H)
    ws = ops.Workspace(DEV)
    Gi = ops.gemm(X.view(B * T, H), W_ih, ws, trans_b=True, epilogue="bias", bias=b_ih).view(B, T, 3 * H)
    H_out, saved = ops.gru_seq_fwd(Gi, W_hh, b_hh)
    res = {}
    res["fused fwd (training: saves 5H per step)"] = timeit(lambda: ops.gru_seq_fwd(Gi, W_hh, b_hh))
    res["fused fwd (inference)"] = timeit(lambda: ops.gru_seq_fwd(Gi, W_hh, b_hh, want_saved=False))
    res["fused bwd (dH_out and dh_T)"] = timeit(lambda: ops.gru_seq_bwd(saved, W_hh, dH, dhT))
    res["input projection GEMM (B*T rows)"] = timeit(
        lambda: ops.gemm(X.view(B * T, H), W_ih, ws, trans_b=True, epilogue="bias", bias=b_ih))
    gh, h0 = torch.empty(B, 3 * H, device=DEV), torch.zeros(B, H, device=DEV)

    def step_gemms():
        for _ in range(T):
            ops.gemm(h0, W_hh, ws, trans_b=True, epilogue="bias", bias=b_hh, out=gh)

    def step_gemms_gates():
        h = h0
        for t in range(T):
            ops.gemm(h, W_hh, ws, trans_b=True, epilogue="bias", bias=b_hh, out=gh)
            rz = torch.sigmoid(Gi[:, t, :2 * H] + gh[:, :2 * H])
            c = torch.tanh(Gi[:, t, 2 * H:] + rz[:, :H] * gh[:, 2 * H:])
            h = torch.lerp(c, h, rz[:, H:])

    dgh, dh = torch.randn(B, 3 * H, device=DEV, generator=g), torch.empty(B, H, device=DEV)

    def step_gemms_bwd():
        for _ in range(T):
            ops.gemm(dgh, W_hh, ws, out=dh)

    few = dict(n=5, warm=2)
    res["(a) per-step GEMM launches alone, fwd"] = timeit(step_gemms, **few)
    res["(a) per-step GEMM + torch gates, fwd"] = timeit(step_gemms_gates, **few)
    res["(a) per-step GEMM launches alone, bwd"] = timeit(step_gemms_bwd, **few)
    gru = torch.nn.GRU(H, H, batch_first=True).to(DEV)
    with torch.no_grad():
        res["(b) torch.nn.GRU fwd (no grad)"] = timeit(lambda: gru(X), **few)
    Xg = X.clone().requires_grad_(True)

    def torch_fwd_bwd():
        out, hn = gru(Xg)
        (out * dH).sum().backward()

    res["(b) torch.nn.GRU fwd + bwd"] = timeit(torch_fwd_bwd, **few)
    for k, v in res.items():
        print("GRU B=%d T=%d H=%d  %-42s %8.3f ms" % (B, T, H, k, v), flush=True)


if __name__ == "__main__":
    for B in (32, 1024):
        bench(B, 152, 128)
