"""Register / scratch / LDS budget of the word2vec kernels (csrc/w2v_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.  Resource report only: the generated code is not inspected.

Planned figures (from the kernels' design; the compiler's report was read afterwards and is quoted in brackets):
  * 10 kernels: the fused forward / backward (VEC 4 and VEC 1), the loss fold, the target update's wave-per-row and
    block-per-slice kernels (each VEC 4 and VEC 1), the search's tile kernel (VEC 4 and VEC 1) and its merge;
  * zero scratch bytes for every kernel — the condition: the only per-thread arrays are the VEC-wide load / store registers
    and the search's 8 x 4 accumulators with their 8 + 4 operands, all indexed by fully unrolled loops;
  * fused forward / backward — a dot partial, one VEC load in flight, three LDS addresses and the row pointers: at most 64,
    8 waves per SIMD; its LDS is DYNAMIC, 3 rows of round4(D) floats per wave: 14.4 KB a block at D 300, 48 KB at the limit
    D 1024 [64 / 64, 8 waves, 0 static];
  * loss fold — two sums and an index: at most 32, 8 waves; static LDS 2 x 1024 floats = 8192 bytes [24, 8 waves, 8192];
  * update, wave per row — a VEC accumulator, one VEC load, the lane's g and input id: at most 48, 8 waves [30 / 26, 8 waves];
  * update, block per slice — a VEC accumulator, g's sum, one VEC load and the index chain sorted_pos -> in_ids -> row:
    planned at most 64.  The report has 108 for VEC 4: the compiler unrolls the occurrence loop and keeps several rows'
    16-byte loads in flight, which is what a latency-bound gather wants.  Kept: the block has 1024 threads, so a CU holds
    two of them, 4 waves per SIMD, at anything up to 128 registers; the bound asserted is 128 (4 waves).  Static LDS: 16
    waves x 16 chunks x VEC floats of partials, 16 sums, the list of a scan step (1024 ints + its count): 8260 / 5188 bytes
    [108 / 57, 4 / 8 waves, 8260 / 5188];
  * search tile — 32 accumulators, 12 operands, four staged 16-byte loads and their addresses: at most 96; static LDS is the
    larger of the staging image (32 x 129 + 32 x 65 floats) and the score tile (64 x 129 floats) plus 128 norms: 33 536
    bytes, so four blocks = 4 waves per SIMD fit the 160 KiB and the registers (5 waves at 96) take no occupancy away
    [88 / 84, 4 waves, 33 536];
  * search merge — a best (score, id) pair, the last one and an index: at most 48, 8 waves [34, 8 waves]."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "w2v_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "w2v_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "w2v.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_w2v_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 10, sorted(occ)                                     # every kernel of the file
    assert all(scratch[k] == 0 for k in occ), scratch
    # (registers, waves per SIMD, static LDS bytes at most)
    budget = {"w2v_sgns_kernel": (64, 8, 0), "w2v_loss_fold_kernel": (32, 8, 8192), "w2v_update_short_kernel": (48, 8, 0),
              "w2v_update_long_kernel": (128, 4, 8260), "w2v_topk_tile_kernel": (96, 4, 33536), "w2v_topk_merge_kernel": (48, 8, 0)}
    seen = dict.fromkeys(budget, 0)
    for k in occ:
        (kind,) = [b for b in budget if b in k]
        seen[kind] += 1
        assert vgpr[k] <= budget[kind][0] and occ[k] >= budget[kind][1] and lds[k] <= budget[kind][2], (k, vgpr[k], occ[k], lds[k])
    assert seen == {"w2v_sgns_kernel": 2, "w2v_loss_fold_kernel": 1, "w2v_update_short_kernel": 2, "w2v_update_long_kernel": 2,
                    "w2v_topk_tile_kernel": 2, "w2v_topk_merge_kernel": 1}
    src = open(os.path.join(CSRC, "w2v_ops.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*?)\);", src, flags=re.S)
    assert len(launches) == 10 and sum("dim3(kBlock), lds," in a for a in launches) == 2          # only the fused kernel: dynamic
    assert "const int per_wave = 3 * ((D + 3) / 4 * 4);" in src and 4 * 3 * 1024 * 4 <= 64 << 10   # within a plain launch's 64 KiB
    assert "atomicAdd(&s_cnt" in src and src.count("atomicAdd") == 1 and "atomicOr(status" in src  # integer atomics only
