"""Register / scratch budget of the DCN cross-network kernels (csrc/dcn_cross.hip), checked at build time: hipcc
cross-compiles gfx950 and reports each kernel's resource usage, no GPU needed.

Planned figures (a row lives in one wave's registers: x_0, x_l, w, b, and in the backward also g, d_w, d_b, the dX_0
accumulator and — rank-1 form — u; 4 floats each per lane at d <= 256, 8 at d <= 512):
  * zero scratch bytes for every kernel of the file;
  * forward (256-thread blocks, grid sized for 8 blocks per CU): 8 waves per SIMD in all four variants, i.e. <= 64 VGPRs;
  * backward at d <= 256 (768-thread blocks, 12 waves; grid sized for 2 blocks per CU): >= 6 waves per SIMD, i.e. <= 80
    VGPRs — what two resident blocks need;
  * backward at d <= 512 (1024-thread blocks, 16 waves; grid sized for 1 block per CU): >= 4 waves per SIMD, i.e. <= 128
    VGPRs — what one resident block needs;
  * the two fold kernels: 8 waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "dcn_cross.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "dcn_cross.resources.txt")      # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "dcn.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_dcn_kernels_no_scratch_and_occupancy(tmp_path):
    occ, scratch, vgpr, name = {}, {}, {}, None
    for line in _remarks(tmp_path).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for pat, dst in ((r"Occupancy \[waves/SIMD\]: (\d+)", occ), (r"ScratchSize \[bytes/lane\]: (\d+)", scratch),
                         (r" VGPRs: (\d+)", vgpr)):
            m = re.search(pat, line)
            if m and name:
                dst[name] = int(m.group(1))
    dcn = {k: v for k, v in occ.items() if "dcn_" in k}
    assert len(dcn) == 14, sorted(dcn)          # fwd x {d<=256, d<=512} x {vector, scalar}; bwd x those x {matrix, rank-1}; 2 folds
    assert all(scratch[k] == 0 for k in dcn), {k: scratch[k] for k in dcn}
    fwd = {k: v for k, v in dcn.items() if "dcn_cross_fwd_kernel" in k}
    bwd1 = {k: v for k, v in dcn.items() if "dcn_cross_bwd_kernelILi1E" in k}
    bwd2 = {k: v for k, v in dcn.items() if "dcn_cross_bwd_kernelILi2E" in k}
    fold = {k: v for k, v in dcn.items() if "fold_kernel" in k}
    assert (len(fwd), len(bwd1), len(bwd2), len(fold)) == (4, 4, 4, 2), sorted(dcn)
    assert all(v >= 8 for v in fwd.values()) and all(vgpr[k] <= 64 for k in fwd), (fwd, vgpr)
    assert all(v >= 6 for v in bwd1.values()) and all(vgpr[k] <= 80 for k in bwd1), (bwd1, vgpr)
    assert all(v >= 4 for v in bwd2.values()) and all(vgpr[k] <= 128 for k in bwd2), (bwd2, vgpr)
    assert all(v >= 8 for v in fold.values()), fold
