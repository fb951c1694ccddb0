"""Register / scratch budget of the FLEN and Adagrad kernels (csrc/flen_ops.hip), checked at build time: hipcc
cross-compiles gfx950 and reports each kernel's resource usage, no GPU needed.

Planned figures:
  * zero scratch bytes for every kernel of the file — the condition: the partition of the slots into field groups is a
    launch argument, and a thread never indexes registers by group (the bounds are copied to LDS once, the group sums are
    formed from the LDS tile of the block's lookups);
  * the forward and backward lookup kernels (a row group holds at most 4 floats of a row, 4 of dH and 4 of the per-group
    factor per lane; 256-thread blocks, the backward's grid sized for 8 blocks per CU): what the gate lookups reach,
    8 waves per SIMD, i.e. <= 64 VGPRs, in all 14 row shapes each (1 or 4 floats per lane x 1 .. 64 lanes per row).  The
    backward holds many uniform values (nine bounds, eight pointers, strides): it is compiled with at most 96 SGPRs, the
    surplus in VGPR lanes, so that the SGPR file does not take the eighth wave;
  * static LDS of the lookup kernels (bounds, kernel_mf, the pair partials) <= 2 KB; the tile and the group sums are
    dynamic LDS sized by the host for at most 16 KB a block (csrc: kFlenTileFloats), which lets 8 blocks share a CU;
  * the Adagrad row kernels (p, acc, g of one row piece per lane) in the 16 shapes of the wide row dispatch (14 + rows of
    257 .. 1024 floats in two more) and the dense kernel: 8 waves per SIMD;
  * 46 kernels: 14 + 14 lookups, the fold, 16 Adagrad row shapes and the dense Adagrad."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "flen_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "flen_ops.resources.txt")      # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(CSRC, "segment_sum.h"),
            os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "flen.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_flen_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 46, sorted(occ)                                     # every kernel the file instantiates
    assert all(scratch[k] == 0 for k in occ), {k: scratch[k] for k in occ}
    fwd = {k: v for k, v in occ.items() if "flen_fwd_kernel" in k}
    bwd = {k: v for k, v in occ.items() if "flen_bwd_kernel" in k}
    fold = {k: v for k, v in occ.items() if "flen_fold_kernel" in k}
    rows = {k: v for k, v in occ.items() if "adagrad_rows_kernel" in k}
    dense = {k: v for k, v in occ.items() if "adagrad_dense_kernel" in k}
    assert (len(fwd), len(bwd), len(fold), len(rows), len(dense)) == (14, 14, 1, 16, 1), sorted(occ)
    assert all(v >= 8 for v in fwd.values()) and all(vgpr[k] <= 64 for k in fwd), (fwd, vgpr)
    assert all(v >= 8 for v in bwd.values()) and all(vgpr[k] <= 64 for k in bwd), (bwd, vgpr)
    assert all(lds[k] <= 2048 for k in list(fwd) + list(bwd) + list(fold)), lds
    assert all(v >= 8 for v in rows.values()) and all(vgpr[k] <= 64 for k in rows), (rows, vgpr)
    assert all(v >= 8 for v in fold.values()) and all(v >= 8 for v in dense.values()), (fold, dense)
