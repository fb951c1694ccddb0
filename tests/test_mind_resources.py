"""Register / scratch / LDS budget of the MIND kernels (csrc/mind_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.  Resource report only: the generated code is not inspected.

Planned figures (from the kernels' design; the compiler's report was read afterwards and is quoted in brackets):
  * 8 kernels: the routing forward (VEC 4 and VEC 1 staging of low into LDS), the routing backward, the label attention
    forward and backward (each VEC 4 and VEC 1) and the sampled-softmax head;
  * zero scratch bytes for every kernel — the condition: the per-capsule values (at most REC_MIND_MAX_K = 8 routing logits,
    2 x 8 capsule columns, 8 scores / weights / score gradients) are arrays indexed ONLY by loops that are fully unrolled and
    guarded by k < k_max, and the VEC-wide load / store registers are indexed by unrolled loops too;
  * static LDS 0 bytes for all eight: only the routing forward uses LDS and it is DYNAMIC, sized by the launch — per wave
    W^T [T][8], caps^T [H][8] and low [T][H | 1], (8 (T + H) + T (H | 1)) floats rounded up to 16 bytes: 39 168 bytes at the
    limits T 64, H 128, and as many waves per block (at most 4) as stay within the 64 KiB a launch gets without an opt-in:
    4 waves / 30.8 KiB per block at the config's T 20, H 64, so 5 blocks = 20 waves per CU fit the 160 KiB; 1 wave /
    38.3 KiB at the limits, 4 waves per CU [0 static for all];
  * registers: head — one accumulator, the running maximum and sum, five addresses: at most 48, 8 waves [32, 8 waves];
    label attention forward — 8 scores, a VEC accumulator, two VEC loads in flight: at most 64, 8 waves [64 / 50, 8 waves];
    routing backward — 2 x 8 dZ columns, 8 weights, 2 x 2 loads per capsule in flight: planned at most 64; the report has 72,
    7 waves: the bound asserted is 80 (6 waves) [72, 7 waves];
    routing forward — 8 logits, 2 x 8 capsule columns and 8 B_delta sums live across the rounds, 40 in all, plus addresses:
    planned at most 64.  The report has 92 registers, 5 waves per SIMD: with the k loop unrolled the compiler keeps the
    16-byte broadcast reads of several t steps in flight beside the sixteen sums.  Kept: the LDS admits 5 waves per SIMD at
    the config's shape (5 blocks x 4 waves) and fewer at every larger one, so the registers take no occupancy away; the
    bound asserted is 96 (5 waves) [92 / 92, 5 waves];
    label attention backward — 8 weights, 8 score gradients, 8 pow factors, and per capsule three VEC loads and two VEC
    stores: planned at most 96 (5 waves).  The report has 126 / 116 registers, 4 waves: the unrolled capsule loop holds every
    capsule's loads of a column chunk at once, and powf is expanded in line.  Kept: one streaming pass ((2 K + 3) H floats
    read, (K + 1) H written per sample) in which 16 resident waves per CU with 3 K 16-byte loads each cover the memory
    latency; the bound asserted is 128 (4 waves) [126 / 116, 4 waves]."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "mind_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "mind_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "mind.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_mind_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 8, sorted(occ)                                      # every kernel of the file
    assert all(scratch[k] == 0 and lds[k] == 0 for k in occ), {k: (scratch[k], lds[k]) for k in occ}
    budget = {"mind_routing_fwd_kernel": (96, 5), "mind_routing_bwd_kernel": (80, 6), "mind_label_attn_fwd_kernel": (64, 8),
              "mind_label_attn_bwd_kernel": (128, 4), "mind_ssm_head_kernel": (48, 8)}      # (registers, waves per SIMD)
    seen = dict.fromkeys(budget, 0)
    for k in occ:
        (kind,) = [b for b in budget if b in k]
        seen[kind] += 1
        assert vgpr[k] <= budget[kind][0] and occ[k] >= budget[kind][1], (k, vgpr[k], occ[k])
    assert seen == {"mind_routing_fwd_kernel": 2, "mind_routing_bwd_kernel": 1, "mind_label_attn_fwd_kernel": 2,
                    "mind_label_attn_bwd_kernel": 2, "mind_ssm_head_kernel": 1}
    src = open(os.path.join(CSRC, "mind_ops.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*?)\);", src, flags=re.S)
    assert len(launches) == 8 and sum("dim3(kBlock), 0," in a for a in launches) == 6       # 256 threads, no dynamic LDS ...
    assert sum("dim3(waves * kWave), waves * per," in a for a in launches) == 2            # ... but the routing forward
    assert src.count("__launch_bounds__(kBlock)") == 5 and src.count("__shared__") == 1
    # the routing forward's LDS at the limits and at the config's shape (the formula of the launch)
    per = lambda T, H: (8 * (T + H) + T * (H | 1) + 3) // 4 * 4 * 4
    assert per(64, 128) == 39168 and (64 << 10) // per(64, 128) == 1 and 4 * per(20, 64) == 31552 and 5 * 31552 <= 160 << 10
    assert "(size_t)(T + H) * 8 + (size_t)T * (H | 1) + 3) / 4 * 4" in src
