"""What DSSM's kernels (csrc/dssm_ops.hip) may use — build time, no GPU: hipcc cross-compiles gfx950 and reports each kernel's
resource usage.  Resource report only: the generated code is not inspected.

  * Every kernel of the file has zero scratch bytes.  The condition: no per-lane array is indexed at run time; a lane's
    accumulators are VEC (1 or 4) floats whose loops unroll, and the per-document values of the head live one in each lane.
  * Every kernel streams: a few loads per multiply-add, latency hidden by other waves and not by registers.  All are held to
    the project's figure for such kernels, 64 VGPRs and 8 waves per SIMD — the column walk of the sparse backward, a chain
    of dependent loads, by its launch bounds.
  * LDS.  Static LDS is 0 everywhere.  Only dssm_sparse_bwd_kernel stages, dynamically: REC_DSSM_BWD_WAVES partial rows of n
    floats, 4 * 8 * n bytes.  The shipped layer (n 300) takes 9 600 bytes a block, so a CU's 160 KB holds 17 blocks of 8 waves
    where its wave slots (4 SIMDs x 8) hold 4: the registers and wave slots bind, not the LDS.  At the widest layer the entry
    admits, REC_DSSM_MAX_WIDTH 2048, it is 64 KiB, a plain launch's maximum: 2 blocks = 16 waves a CU, 4 waves per SIMD.
  * No float atomics: the source has no atomicAdd and exactly one atomicOr(status...) site, the out-of-range column of the
    sparse forward (one site, both instantiations), and no other atomic call."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")
KERNELS = ("dssm_lod_rows_kernel", "dssm_sparse_fwd_kernelILi4", "dssm_sparse_fwd_kernelILi1", "dssm_sparse_bwd_kernelILi4",
           "dssm_sparse_bwd_kernelILi1", "dssm_head_kernelILi4", "dssm_head_kernelILi1", "dssm_loss_fold_kernel",
           "dssm_cos_kernelILi4", "dssm_cos_kernelILi1")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "dssm_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "dssm_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "dssm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_dssm_kernels_no_scratch_and_budget(tmp_path):
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
        print("%-28s VGPRs %3d  waves/SIMD %d  static LDS %d" % (kind, vgpr[k], occ[k], lds[k]))
        assert lds[k] == 0, (k, lds[k])                                    # dynamic only, and only the sparse backward
        assert vgpr[k] <= 64 and occ[k] >= 8, (k, vgpr[k], occ[k])
    # the sparse backward's dynamic LDS: waves x n floats
    per_block = lambda n: 4 * _lib.REC_DSSM_BWD_WAVES * n
    assert per_block(300) == 9600 and (160 << 10) // per_block(300) == 17 > 4
    assert per_block(_lib.REC_DSSM_MAX_WIDTH) == 64 << 10 and (160 << 10) // (64 << 10) == 2
    src = open(os.path.join(CSRC, "dssm_ops.hip")).read()
    assert "atomicAdd" not in src and src.count("atomicOr(status") == 1     # the integer status flag is the only atomic
    assert len(re.findall(r"\batomic\w*\(", src)) == 1
    assert src.count("extern __shared__") == 1 and "__shared__ float" not in src.replace("extern __shared__", "")
