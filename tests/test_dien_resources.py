"""Register / scratch budget of the DIEN kernels (csrc/dien_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.

Planned figures (from the kernels' design; where a figure of the compiler's report is quoted, it was read afterwards):
  * zero scratch bytes for every kernel of the file — the condition: every register array (the W_hh slice, the
    accumulators, the carried dh) is indexed by fully unrolled loops only;
  * the recurrent kernels run 512-thread blocks (8 waves, 2 per SIMD), one block per CU: their budget is 256 VGPRs a lane
    and the planned occupancy 2 waves per SIMD.  The registers-resident forms (H 128; template argument true) hold 96
    floats of W_hh per lane — forward 3 gates x 8 k-blocks x float4, backward 24 k-blocks x 4 — plus 12 accumulator
    registers forward (three chains) or 8 backward (two chains), 12 Gi values, the A fragment and addresses: estimated
    150-180 VGPRs when the kernels were written, and in any case above 128 and within the 256 of the budget, i.e.
    occupancy exactly 2 (the compiler's report: 226 forward, 232 backward).  The general forms hold no weights: planned
    at most 128 VGPRs (occupancy 4 by registers; reported 128 and 112);
  * the recurrent kernels' LDS is dynamic (forward 2 x 16 x (H + 4) floats: 33 KB at H 256; backward 16 x (3H + 4)
    floats: 48.3 KB at H 256 — both below the 64 KB a launch gets without an opt-in), so the static figure is 0;
  * the seven small kernels — aux forward, its fixed-order reduce, aux backward, the two feature kernels, the softmax
    forward and backward: 256-thread blocks, 8 waves per SIMD (<= 64 VGPRs); the reduce and the two softmax kernels hold
    one 256-float fold buffer (1 KB of LDS), the others none;
  * 11 kernels in all: 2 x 2 recurrent + 7."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "dien_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "dien_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "dien.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_dien_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 11, sorted(occ)                                     # every kernel the file instantiates
    assert all(scratch[k] == 0 for k in occ), {k: scratch[k] for k in occ}
    pick = lambda s: sorted(k for k in occ if s in k)
    regw = pick("gru_seq_fwd_kernelILb1") + pick("gru_seq_bwd_kernelILb1")
    general = pick("gru_seq_fwd_kernelILb0") + pick("gru_seq_bwd_kernelILb0")
    assert len(regw) == 2 and len(general) == 2, sorted(occ)
    for k in regw:
        assert occ[k] == 2 and 128 < vgpr[k] <= 256 and lds[k] == 0, (k, occ[k], vgpr[k], lds[k])
    for k in general:
        assert occ[k] >= 2 and vgpr[k] <= 128 and lds[k] == 0, (k, occ[k], vgpr[k], lds[k])
    small = [k for k in occ if k not in regw + general]
    assert len(small) == 7 and all(occ[k] >= 8 and vgpr[k] <= 64 for k in small), {k: (occ[k], vgpr[k]) for k in small}
    fold = pick("dien_aux_reduce_kernel") + pick("dien_attention_seq_fwd_kernel") + pick("dien_attention_seq_bwd_kernel")
    assert len(fold) == 3 and all(lds[k] == (1024 if k in fold else 0) for k in small), {k: lds[k] for k in small}
