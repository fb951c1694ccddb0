"""Register / scratch budget of the FFM kernels (csrc/ffm_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.  The LDS fast path is sized for two 256-thread blocks per CU
(a 56 KB cube image each at the reference shape), i.e. two waves per SIMD: registers must not be what limits it."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "ffm_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "ffm_ops.resources.txt")       # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "ffm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_ffm_kernels_no_scratch_and_occupancy(tmp_path):
    occ, scratch, name = {}, {}, None
    for line in _remarks(tmp_path).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            occ[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    ffm = {k: v for k, v in occ.items() if "ffm_" in k}
    assert len(ffm) == 5, sorted(ffm)                        # fwd / bwd x {LDS, L2} + the fold
    assert all(scratch[k] == 0 for k in ffm), {k: scratch[k] for k in ffm}
    fwd_lds = [v for k, v in ffm.items() if "ffm_fwd_kernelILb1E" in k]
    bwd_lds = [v for k, v in ffm.items() if "ffm_bwd_kernelILb1E" in k]
    assert fwd_lds and bwd_lds, sorted(ffm)
    assert fwd_lds[0] >= 4 and bwd_lds[0] >= 2, (fwd_lds, bwd_lds)
