"""Register / scratch budget of the GateNet kernels (csrc/gate_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.

Planned figures:
  * zero scratch bytes for every kernel of the file;
  * the forward and backward lookup kernels (a row group holds at most 4 floats of e, 4 of g and a few scalars per lane;
    256-thread blocks, the backward's grid sized for 8 blocks per CU): 8 waves per SIMD, i.e. <= 64 VGPRs, in all 14
    row shapes each (1 or 4 floats per lane x 1 .. 64 lanes per row);
  * the backward's LDS (field sums + two rows of per-lookup contributions) lets 8 blocks share a CU: <= 20 KB per block;
  * 35 kernels: 14 + 14 lookups, the fold, and {hidden fwd, hidden bwd, relu mask} x {vector, scalar}."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "gate_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "gate_ops.resources.txt")      # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "gate.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gate_kernels_no_scratch_and_occupancy(tmp_path):
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
    gate = {k: v for k, v in occ.items() if "gate_" in k}
    assert len(gate) == 35, sorted(gate)
    assert all(scratch[k] == 0 for k in gate), {k: scratch[k] for k in gate}
    fwd = {k: v for k, v in gate.items() if "gate_emb_fwd_kernel" in k}
    bwd = {k: v for k, v in gate.items() if "gate_emb_bwd_kernel" in k}
    rows = {k: v for k, v in gate.items() if "gate_hidden_" in k or "gate_relu_mask" in k}
    fold = {k: v for k, v in gate.items() if "gate_fold_kernel" in k}
    assert (len(fwd), len(bwd), len(rows), len(fold)) == (14, 14, 6, 1), sorted(gate)
    assert all(v >= 8 for v in fwd.values()) and all(vgpr[k] <= 64 for k in fwd), (fwd, vgpr)
    assert all(v >= 8 for v in bwd.values()) and all(vgpr[k] <= 64 for k in bwd), (bwd, vgpr)
    assert all(lds[k] <= 20 * 1024 for k in bwd), {k: lds[k] for k in bwd}
    assert all(v >= 8 for v in rows.values()) and all(v >= 8 for v in fold.values()), (rows, fold)
