"""What NCF's kernels (csrc/ncf_ops.hip) may use — build time, no GPU: hipcc cross-compiles gfx950 and reports each kernel's
resource usage.  Resource report only: the generated code is not inspected.

  * Every kernel of the file has zero scratch bytes.  The condition: no per-lane array exists; the plan (offsets and widths,
    indexed by the layer) is a kernel argument, read with scalar loads.
  * LDS is dynamic only; at the constants' limits it is REC_NCF_LDS_BYTES = 64 KiB, a plain launch's maximum: the
    eligibility query admits a net only when 4 (2 P + REC_NCF_TILE S) fits (tests/test_ncf.py restates the formula).
  * The step kernel's budget follows from its LDS, not from its registers.  The shipped net needs 48.5 KB a block, so a CU's
    160 KB holds 3 blocks = 12 waves = 3 waves per SIMD; at the 64 KiB limit it is 2 blocks, 2 waves per SIMD.  Registers
    must not bind before the LDS does: the register-limited occupancy has to be at least 4 waves per SIMD, i.e. at most
    512 / 4 = 128 VGPRs.  The kernel holds a handful of offsets, one accumulator and two operands per thread, so this
    leaves room; the score kernel is held to the same figures.  The fold and the two gather kernels stream: 64 VGPRs, 8
    waves per SIMD.
  * No float atomics: the source has no atomicAdd and exactly two atomicOr(status...) sites — the validated ids of the
    fused kernel (one site, both instantiations) and the gather forward — and no other atomic call."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")
KERNELS = ("ncf_net_kernelILb1", "ncf_net_kernelILb0", "ncf_fold_kernel", "ncf_gather_fwd_kernel", "ncf_gather_bwd_kernel")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "ncf_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "ncf_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "ncf.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_ncf_kernels_no_scratch_and_budget(tmp_path):
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
        assert lds[k] == 0, (k, lds[k])                                    # dynamic only: sized by the eligibility formula
        if kind.startswith("ncf_net_kernel"):
            assert vgpr[k] <= 128 and occ[k] >= 4, (k, vgpr[k], occ[k])
        else:
            assert vgpr[k] <= 64 and occ[k] >= 8, (k, vgpr[k], occ[k])
    assert _lib.REC_NCF_LDS_BYTES == 64 << 10
    # the shipped net: 2 * 2764 weights and accumulators + 32 samples of 206 floats = 48 480 bytes, 3 blocks in a CU's 160 KB
    assert 4 * (2 * 2764 + _lib.REC_NCF_TILE * 206) == 48480 and 3 * 48480 <= 160 << 10 < 4 * 48480
    src = open(os.path.join(CSRC, "ncf_ops.hip")).read()
    assert "atomicAdd" not in src and src.count("atomicOr(status") == 2     # integer status flags are the only atomics
    assert len(re.findall(r"\batomic\w*\(", src)) == 2
