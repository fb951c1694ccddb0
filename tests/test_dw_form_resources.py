"""Register budget of the eight-wave weight-gradient kernel (csrc/gemm_bf16x3.h, gemm_bf16x3_dw_kernel_w8), checked at
build time: it is designed for TWO waves per SIMD (<= 256 registers: 4 x 7 accumulator tiles, four X tiles' fragments,
two G tiles', a 32-register patch) and must not spill — at one wave per SIMD it is the old form with twice the waves."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _remarks(tmp_path):
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "gemm_f32.resources.txt")     # written by paddlerec_amd.build
    csrc = os.path.join(REPO, "paddlerec_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("gemm_f32.hip", "gemm_bf16x3.h", "gemm_epi.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps):
        return open(saved).read()
    lab = os.path.join(REPO, "tools", "gemm_lab", "bf16x3_lab.hip")                   # the header alone: a faster compile
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + csrc, "-DREC_X3_LAB_STANDALONE", "-c", lab, "-o", str(tmp_path / "x3.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_dw_kernel_w8_two_waves_per_simd_no_scratch(tmp_path):
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
    w8 = [k for k in occ if "gemm_bf16x3_dw_kernel_w8" in k]
    assert len(w8) == 2, sorted(occ)[:10]                     # PW 4 (13 / 12-tile blocks) and 3 (9..11)
    assert all(occ[k] >= 2 for k in w8), {k: occ[k] for k in w8}
    assert all(scratch[k] == 0 for k in w8), {k: scratch[k] for k in w8}
