"""What TiSASRec's kernels (csrc/tisas_ops.hip) and its train step may use.

  * Build time, no GPU: hipcc cross-compiles gfx950 and reports each kernel's resource usage.  Every kernel of the file has
    zero scratch bytes (private segment size 0) — the condition: the only per-thread arrays are the two-element per-lane
    key arrays of the attention kernels, indexed by fully unrolled loops.  The two query-row attention kernels hold a dot
    partial, the lane's two scores / weights / gradients and the mask hash: at most 96 registers, 5 waves per SIMD
    [77 / 92, 6 / 5 waves]; everything else at most 64, 8 waves.  Their LDS is dynamic and sized by the shape, within a
    plain launch's 64 KiB at the limits (REC_TISAS_MAX_TILE, REC_TISAS_MAX_TIME_TILE).  Resource report only: the
    generated code is not inspected.
  * On the GPU: one train step at B 64, L 50, D 50, T 257, 2 blocks, dropout on.  The reference materialises time_matrix_K
    and time_matrix_V, two [B, L, L, D] float tensors: 2 * B * L * L * D * 4 bytes = 64 MB here.  The step's peak
    allocation above what was allocated before it must stay BELOW that — a condition derived from the goal (the relation
    tensors are never formed), not a measurement."""
import os
import re
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "tisas_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "tisas_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "tisas.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_tisas_kernels_no_scratch_and_occupancy(tmp_path):
    from paddlerec_amd import _lib
    occ, scratch, vgpr, lds, name = {}, {}, {}, {}, None
    for line in _remarks(tmp_path).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for pat, dst in ((r"Occupancy \[waves/SIMD\]: (\d+)", occ), (r"ScratchSize \[bytes/lane\]: (\d+)", scratch),
                         (r" VGPRs: (\d+)", vgpr), (r"LDS Size \[bytes/block\]: (\d+)", lds)):
            m = re.search(pat, line)
            if m and name:
                dst[name] = int(m.group(1))
    kernels = ("ts_attn_fwd_kernel", "ts_attn_bwd_q_kernel", "ts_attn_bwd_kv_kernel", "ts_pos_grad_kernel", "ts_time_partial_kernel",
               "ts_time_fold_kernel", "aln_fwd_kernel", "aln_bwd_kernel", "aln_param_kernel", "ts_embed_kernel",
               "ts_head_count_kernel", "ts_head_rows_kernel", "ts_head_loss_kernel")
    assert len(occ) == len(kernels), sorted(occ)                           # every kernel of the file
    assert all(scratch[k] == 0 for k in occ), scratch                      # private segment size 0
    for k in occ:
        (kind,) = [b for b in kernels if b in k]
        regs, waves = (96, 5) if kind in ("ts_attn_fwd_kernel", "ts_attn_bwd_q_kernel") else (64, 8)
        assert vgpr[k] <= regs and occ[k] >= waves and lds[k] <= 2048, (k, vgpr[k], occ[k], lds[k])
    # the dynamic LDS of the attention kernels at the limits stays within a plain launch's 64 KiB
    per_wave = 2 * _lib.REC_TISAS_MAX_HEAD + 2 * _lib.REC_TISAS_MAX_L
    assert (2 * _lib.REC_TISAS_MAX_TILE + 4 * per_wave) * 4 <= 64 << 10
    assert _lib.REC_TISAS_MAX_TIME_TILE * 4 <= 64 << 10 and 2 * _lib.REC_TISAS_MAX_L * _lib.REC_TISAS_MAX_HEAD * 4 <= 64 << 10
    assert 50 * 51 <= _lib.REC_TISAS_MAX_TILE and 70 * 51 <= _lib.REC_TISAS_MAX_TILE and 257 * 50 <= _lib.REC_TISAS_MAX_TIME_TILE
    src = open(os.path.join(CSRC, "tisas_ops.hip")).read()
    assert "atomicAdd" not in src and src.count("atomicOr(status") == 3     # integer status flags are the only atomics


@pytest.mark.gpu
def test_train_step_stays_below_the_relation_tensors():
    from paddlerec_amd.tisas import TiSASRecLayer
    B, L, D, T, items = 64, 50, 50, 257, 3416
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    m = TiSASRecLayer(6040, items, D, L, T - 1, 2, 1, dropout_rate=0.2, device=dev)
    seq = torch.randint(1, items + 1, (B, L), generator=g)
    seq[:, :7] = 0
    seq[3] = 0
    ts = torch.cumsum(torch.randint(0, 40, (B, L), generator=g), 1) * (seq != 0)
    tm = (ts[:, :, None] - ts[:, None, :]).abs().clamp(max=T - 1)
    pos = torch.randint(1, items + 1, (B, L), generator=g) * (seq != 0)
    neg = torch.randint(1, items + 1, (B, L), generator=g) * (seq != 0)
    feeds = [t.to(dev).contiguous() for t in (seq, tm, pos, neg)]
    torch.cuda.synchronize()                                # the FIRST step: its scratch buffers and workspaces count too
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss, _ = m.train_step(*feeds)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    relation = 2 * B * L * L * D * 4
    print("train step peak above the resident state: %.2f MB; the two relation tensors: %.2f MB" % (peak / 2 ** 20, relation / 2 ** 20))
    assert torch.isfinite(loss.value()).all() and int(m.status.item()) == 0
    assert 0 < peak < relation
