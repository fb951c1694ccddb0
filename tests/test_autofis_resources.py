"""Register / scratch budget of the AutoFIS kernels (csrc/autofis_ops.hip), checked at build time: hipcc cross-compiles
gfx950 and reports each kernel's resource usage, no GPU needed.

Planned figures (written down with the kernels, before the compiler's report was read):
  * zero scratch bytes for every kernel of the file — the condition: the pair list and the per-field adjacency are read
    from memory by index, never held in registers; the per-sample accumulators of the eval forward are a 4-entry array
    that every loop over it unrolls fully (csrc: kAfMaxSb);
  * the lookup + pair kernel in the 14 row shapes of the lookup dispatch (1 or 4 floats per lane x 1 .. 64 lanes per row),
    once for training (Welford partials) and once for eval: 28 instantiations, 256-thread blocks, 8 waves per SIMD, i.e.
    <= 64 VGPRs.  A thread holds one row piece (<= 4 floats), a dot product, (mean, M2) of one pair and at most 4
    accumulators.  The kernel takes one struct of 14 pointers and 12 scalars: it is compiled with at most 96 SGPRs, as the
    FLEN backward is, so that the SGPR file does not take the eighth wave;
  * its static LDS is the fold buffer of the eval form (256 floats, 1 KB; the training form has none); the tile, the
    first-order weights and the two per-pair arrays are dynamic LDS sized by the host for at most 19 KB a block (csrc:
    kAfLdsFloats = 4864 floats) as long as one sample fits, which lets 8 blocks of 256 threads share a CU's 160 KB;
  * the six small kernels — merge (three [4][64] float arrays and the fold buffer: 4 KB of LDS), row pass, the backward's
    column reduction (2 KB), its finalize, its row kernel and the GRDA step: 8 waves per SIMD by registers.  The row
    kernel (11 pointers and 6 scalars: capped at 96 SGPRs like the lookup kernel; four accumulators per thread) has dynamic
    LDS only — the tile, dL and the adjacency — sized for at most 26 KB a block (csrc: kAfBwdLdsFloats), 6 blocks per CU;
  * 34 kernels in all: 28 + 6."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "autofis_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "autofis_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "autofis.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_autofis_kernels_no_scratch_and_occupancy(tmp_path):
    occ, scratch, vgpr, sgpr, lds, name = {}, {}, {}, {}, {}, None
    for line in _remarks(tmp_path).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for pat, dst in ((r"Occupancy \[waves/SIMD\]: (\d+)", occ), (r"ScratchSize \[bytes/lane\]: (\d+)", scratch),
                         (r" VGPRs: (\d+)", vgpr), (r"TotalSGPRs: (\d+)", sgpr), (r"LDS Size \[bytes/block\]: (\d+)", lds)):
            m = re.search(pat, line)
            if m and name:
                dst[name] = int(m.group(1))
    assert len(occ) == 34, sorted(occ)                                     # every kernel the file instantiates
    assert all(scratch[k] == 0 for k in occ), {k: scratch[k] for k in occ}
    pick = lambda s: {k: v for k, v in occ.items() if s in k}
    train, evalk = pick("autofis_fwd_kernelILi1ELi") | pick("autofis_fwd_kernelILi4ELi"), {}
    evalk = {k: v for k, v in train.items() if k.endswith("Lb0EEEvNS0_5AfFwdE")}
    train = {k: v for k, v in train.items() if k.endswith("Lb1EEEvNS0_5AfFwdE")}
    small = [pick(s) for s in ("autofis_merge_kernel", "autofis_rows_kernel", "autofis_bwd_reduce_kernel",
                               "autofis_bwd_finalize_kernel", "autofis_bwd_rows_kernel", "grda_kernel")]
    assert (len(train), len(evalk)) == (14, 14) and [len(s) for s in small] == [1] * 6, sorted(occ)
    for k in list(train) + list(evalk):
        assert occ[k] >= 8 and vgpr[k] <= 64 and sgpr[k] <= 96, (k, occ[k], vgpr[k], sgpr[k])
    assert all(lds[k] == 0 for k in train) and all(lds[k] == 1024 for k in evalk), lds
    assert all(v >= 8 for s in small for v in s.values()), small
    merge, _, reduce_, _, rows, _ = (next(iter(s)) for s in small)
    assert lds[merge] == 4096 and lds[reduce_] == 2048 and lds[rows] == 0, lds
