"""Register / scratch budget of the entire-space kernels (csrc/esm_ops.hip), checked at build time: hipcc cross-compiles
gfx950 and reports each kernel's resource usage, no GPU needed.

Planned figures (from the kernels' design; the compiler's report was read afterwards and is quoted in brackets):
  * 4 kernels: the field sum-pool instantiated for VEC 4 (float4 columns) and VEC 1, the click count and the head;
  * zero scratch bytes for every kernel — the condition: the only per-thread arrays are the pool's VEC-wide accumulator and
    load registers (2 x 4 floats live), indexed by fully unrolled loops only; the head keeps its three tasks in named
    scalars (three small structs of five fields), never in an array indexed by the task; the head's descriptor arrives by
    value in the kernel arguments (scalar loads, no copy to the stack);
  * every block is 256 threads; LDS only in the click count: one int64 per wave of the block, 4 x 8 = 32 bytes, the hand-over
    between the waves' butterflies and thread 0; none in the pool (the ids of a pair are broadcast loads, every lane adds
    its own columns) and none in the head (one thread per sample) [32, 0, 0, 0];
  * registers: pool — a VEC accumulator, a VEC of loaded values, the id, three 64-bit addresses and loop counters: planned at
    most 32 [22 for VEC 4, 16 for VEC 1]; click count — four 64-bit sums and four loaded 64-bit values (four loads in
    flight), a 64-bit index and an address: 8 + 8 + 4 and some slack, at most 32 [24]; head —
    six logits, three softmaxes of five values, the labels, three costs and a handful of derivative terms, most of them dead
    before the stores: planned at most 64 [39]; i.e. the full 8 waves per SIMD for all four [8]."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "esm_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "esm_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "esm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_esm_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 4, sorted(occ)                                      # every kernel of the file
    assert all(scratch[k] == 0 and occ[k] == 8 for k in occ), {k: (scratch[k], occ[k]) for k in occ}
    pools = [k for k in occ if "field_sumpool_fwd_kernel" in k]
    (count,) = [k for k in occ if "esm_click_count_kernel" in k]
    (head,) = [k for k in occ if "esm_head_kernel" in k]
    assert len(pools) == 2 and all(vgpr[k] <= 32 and lds[k] == 0 for k in pools), {k: (vgpr[k], lds[k]) for k in pools}
    assert vgpr[count] <= 32 and lds[count] == 32 and vgpr[head] <= 64 and lds[head] == 0, {k: (vgpr[k], lds[k]) for k in occ}
    src = open(os.path.join(CSRC, "esm_ops.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*?)\);", src, flags=re.S)
    assert len(launches) == 4 and all("dim3(kBlock)" in a for a in launches)
    assert src.count("__launch_bounds__(kBlock)") == 3 and "atomic" not in src.replace("is atomic", "")
