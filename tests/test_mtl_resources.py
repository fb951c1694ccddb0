"""Register / scratch budget of the multitask kernels (csrc/mtl_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.

Planned figures (from the kernels' design; where a figure of the compiler's report is quoted, it was read afterwards):
  * 5 kernels: the mixture forward and backward, each instantiated for VEC 4 (float4 columns) and VEC 1, and the head;
  * zero scratch bytes for every kernel — the condition: the only per-thread arrays are the VEC-wide accumulator and load
    registers of the two mixture kernels (at most 3 x 4 floats live), indexed by fully unrolled loops only.  The slot map
    arrives by value in the kernel arguments and is indexed by the gate, a wave-uniform value (scalar loads, no copy to
    the stack); a gate's dp_j are not kept in registers (up to 64 per row): the lane that stores dp_j re-reads its own
    store once the gate's sum is known;
  * every block is 256 threads, no LDS anywhere (the softmax is per lane over broadcast loads — a whole-wave row shuffles each lane's
    probability to the others; the backward's dot products end in a shuffle butterfly over the row's lanes);
  * registers: a row pointer set of 4-5 addresses (2 VGPRs each), a VEC accumulator, a VEC or two of loaded values, the
    running max / sum / probability and loop counters — planned at most 48 for the mixture kernels and at most 32 for the
    head, i.e. the full 8 waves per SIMD for all five (reported: forward 36 / 30, backward 36 / 30 for VEC 4 / 1, head 23;
    occupancy 8)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "mtl_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "mtl_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "mtl.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_mtl_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 5, sorted(occ)                                      # every kernel of the file
    assert all(scratch[k] == 0 for k in occ), {k: scratch[k] for k in occ if scratch[k]}
    assert all(lds[k] == 0 and occ[k] == 8 for k in occ), {k: (lds[k], occ[k]) for k in occ}
    mixes = [k for k in occ if "mtl_mix_fwd_kernel" in k or "mtl_mix_bwd_kernel" in k]
    (head,) = [k for k in occ if "mtl_head_kernel" in k]
    assert len(mixes) == 4 and all(vgpr[k] <= 48 for k in mixes) and vgpr[head] <= 32, {k: vgpr[k] for k in occ}
    src = open(os.path.join(CSRC, "mtl_ops.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*?)\);", src, flags=re.S)
    assert len(launches) == 5 and all("dim3(kBlock)" in a for a in launches)
    assert src.count("__launch_bounds__(kBlock)") == 3 and "atomic" not in src.replace("atomics", "").replace("is atomic", "")
