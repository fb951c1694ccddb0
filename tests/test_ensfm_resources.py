"""What ENSFM's kernels (csrc/ensfm_ops.hip) and its train step may use.

  * Build time, no GPU: hipcc cross-compiles gfx950 and reports each kernel's resource usage.  Every kernel of the file has
    zero scratch bytes (private segment size 0) — the condition: the per-lane arrays (at most 3 columns of a [., D + 2] row,
    times the 4 gathers in flight of the two positives kernels) are indexed by fully unrolled loops.  The budget is 64
    registers and 8 waves per SIMD for every kernel: the widest, the tower backward and the user-owned positives, hold
    4 x 3 gathered values, 3 accumulators, 3 operand values and the addresses of 4 rows [62 / 58]; the gathers are served from
    L2, so what hides their latency is waves in flight, and 8 per SIMD is the most the hardware offers.  Static LDS is at
    most a [4][130] fold tile (2.6 KB); the dynamic LDS at the limits — the Gram tile 64 x 130 floats, the score tile
    64 x 131 + 16 x 130 floats — stays within a plain launch's 64 KiB.  Resource report only: the generated code is not
    inspected.
  * On the GPU: one FIRST train step at B 128, P 1024, I 3706, D 64 with random lists.  The reference keeps three [B, P, C]
    float tensors for the positives and a [B, I+1, C] `dot`; ONE [B, P, C] tensor is B * P * C * 4 bytes = 34.6 MB, which is
    also below B * (I+1) * C * 4.  The step's peak allocation above what was allocated before it must stay BELOW that — a
    condition derived from the goal (no (b, j, c)-shaped array exists at any point), not a measurement."""
import os
import re
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")
KERNELS = ("ef_tower_fwd_kernel", "ef_tower_bwd_kernel", "ef_fold_cols_kernel", "ef_gram_kernel", "ef_gram_fold_kernel",
           "ef_pos_user_kernel", "ef_item_gram_kernel", "ef_pos_item_kernel", "ef_loss_kernel", "ef_score_kernel")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "ensfm_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "ensfm_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "ensfm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_ensfm_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == len(KERNELS), sorted(occ)                           # every kernel of the file
    assert all(scratch[k] == 0 for k in occ), scratch                      # private segment size 0
    for k in occ:
        (kind,) = [b for b in KERNELS if b in k]
        assert vgpr[k] <= 64 and occ[k] >= 8 and lds[k] <= 4 * (_lib.REC_ENSFM_MAX_DIM + 2) * 4 + 1024, (k, vgpr[k], occ[k], lds[k])
    C = _lib.REC_ENSFM_MAX_DIM + 2
    assert 64 * C * 4 <= 64 << 10 and (64 * (C | 1) + 16 * C) * 4 <= 64 << 10          # the dynamic LDS at the limits
    assert _lib.REC_ENSFM_MAX_DIM >= 128
    src = open(os.path.join(CSRC, "ensfm_ops.hip")).read()
    assert "atomicAdd" not in src and src.count("atomicOr(status") == 2     # integer status flags are the only atomics
    assert len(re.findall(r"\batomic\w*\(", src)) == 2


@pytest.mark.gpu
def test_train_step_stays_below_one_positives_tensor():
    from paddlerec_amd.ensfm import ENSFMLayer
    B, P, I, D, Fu, Fi = 128, 1024, 3706, 64, 4, 2
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    m = ENSFMLayer(6069, 3953, D, device=dev)
    u = torch.randint(0, 6069, (B, Fu), generator=g)
    attr = torch.randint(0, 3953, (I + 1, Fi), generator=g)
    attr[I] = attr[0]
    ur = torch.randint(0, I, (B, P), generator=g)
    ur[torch.arange(P)[None, :] >= torch.randint(1, P + 1, (B, 1), generator=g)] = I      # lists of random length, padded
    feeds = [t.to(dev).contiguous() for t in (u, attr, ur)]
    torch.cuda.synchronize()                                # the FIRST step: its scratch buffers and workspaces count too
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss = m.train_step(*feeds)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    one = B * P * (D + 2) * 4
    print("train step peak above the resident state: %.2f MB; one [B, P, C] tensor: %.2f MB; dot: %.2f MB"
          % (peak / 2 ** 20, one / 2 ** 20, B * (I + 1) * (D + 2) * 4 / 2 ** 20))
    assert torch.isfinite(loss).all() and int(m.status.item()) == 0
    assert one < B * (I + 1) * (D + 2) * 4 and 0 < peak < one
