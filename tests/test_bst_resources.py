"""Register / scratch budget of the BST kernels (csrc/bst_ops.hip), checked at build time: hipcc cross-compiles gfx950 and
reports each kernel's resource usage, no GPU needed.

Planned figures (from the kernels' design; where a figure of the compiler's report is quoted, it was read afterwards):
  * zero scratch bytes for every kernel of the file — the condition: the per-row register arrays of the attention kernels
    (4 float4 each: the lane's chunks of q / dO / the accumulator, or of k, v, dK, dV) are indexed by fully unrolled loops
    only; no other kernel holds an array;
  * 12 kernels, no templates: attention forward, dQ pass, dK / dV pass; add + layer norm forward / backward; LeakyReLU
    forward / backward; add; embed forward / backward; position sum forward / backward;
  * every block is 256 threads.  Attention: two LDS tiles of 64 rows x 16 float4 = 32 768 bytes static in each of the three
    kernels, plus 2 x 64 floats (lse, delta) = 33 280 in the dK / dV pass — below the 64 KB a block may take; nothing
    dynamic.  Registers: the forward holds 2 arrays (q, acc) = 32 VGPRs plus (m, l, the tile row being read, addresses) —
    planned at most 96; the dQ pass holds 3 arrays (q, dO, dq) — planned at most 112; the dK / dV pass holds 4 (k, v, dK,
    dV) — planned at most 128, the last figure that still gives 4 waves per SIMD (512 / 128), which is also what the LDS
    allows (160 KB / 32.5 KB = 4 blocks of 4 waves on 4 SIMDs).  Planned occupancy: at least 4 for all three (reported 66 /
    82 / 110 VGPRs, occupancy 5 / 5 / 4);
  * the other nine are streaming or per-row kernels with a handful of live values: planned at most 64 VGPRs, i.e. the full
    8 waves per SIMD (reported 10 .. 30), no LDS except the 256-float buffer of the fixed-order bias-gradient fold in the
    position-sum backward (1024 bytes)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "bst_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "bst_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "bst.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_bst_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 12, sorted(occ)                                     # every kernel of the file
    assert all(scratch[k] == 0 for k in occ), {k: scratch[k] for k in occ if scratch[k]}
    one = lambda s: [k for k in occ if s in k]
    plan = {"mha_fwd_kernel": (96, 32768), "mha_dq_kernel": (112, 32768), "mha_dkv_kernel": (128, 33280)}
    mha = []
    for s, (regs, bytes_) in plan.items():
        (k,) = one(s)
        mha.append(k)
        assert vgpr[k] <= regs and lds[k] == bytes_ <= 65536 and occ[k] >= 4, (k, vgpr[k], lds[k], occ[k])
    plain = [k for k in occ if k not in mha]
    assert len(plain) == 9 and all(occ[k] == 8 and vgpr[k] <= 64 for k in plain), {k: (occ[k], vgpr[k]) for k in plain}
    (fold,) = one("bst_possum_bwd_kernel")
    assert all(lds[k] == (1024 if k == fold else 0) for k in plain), {k: lds[k] for k in plain}
