"""Register / scratch budget of the DMR kernels (csrc/dmr_ops.hip), checked at build time: hipcc cross-compiles gfx950
and reports each kernel's resource usage, no GPU needed.

Planned figures (from the kernels' design; where a figure of the compiler's report is quoted, it was read afterwards):
  * zero scratch bytes for every kernel of the file — the condition: the match-loss register arrays (U_b or V_c and the
    gradient accumulators, K / 4 float4 each) are sized by the template argument and indexed by fully unrolled loops
    only; no other kernel holds an array;
  * 30 kernels: 12 plain (prefix pool forward / backward, PReLU forward / backward / fold, the match loss's lse, mean and
    two fold kernels, three tail kernels) and 3 match-loss templates x 6 register-array sizes (K / 4 rounded up to 1, 2,
    4, 8, 12, 16);
  * every block is 256 threads.  The 12 plain kernels are streaming or per-sample kernels with a handful of live values:
    planned at most 64 VGPRs, i.e. the full 8 waves per SIMD (reported 8 .. 41).  The kernels with a fixed-order block
    fold (prefix pool forward and backward, PReLU fold, the loss mean, the tail forward) hold one 256-float buffer: 1024
    bytes of static LDS; the others none.  The prefix-pool backward adds 2 x T floats of dynamic LDS (at most 32 KB at
    its limit T 4096), which the static figure does not show;
  * match-loss templates, array size A (float4): forward holds A float4 of U plus four chains — planned 4 A + about 16
    VGPRs; dU and dV hold two such arrays — planned 8 A + about 16.  At the net's K 32 (A 8) that is about 48 and 80:
    planned occupancy 8 and at least 5 (reported 46 / 76 / 74 VGPRs, occupancy 8 / 6 / 6).  The largest, A 16, was
    planned below 160 VGPRs — occupancy at least 3 (reported 140 and 139, occupancy 3); no LDS in any of them (the
    class row / batch row every lane shares is a uniform load)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")


def _remarks(tmp_path):
    src = os.path.join(CSRC, "dmr_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "dmr_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "dmr.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_dmr_kernels_no_scratch_and_occupancy(tmp_path):
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
    assert len(occ) == 30, sorted(occ)                                     # every kernel the file instantiates
    assert all(scratch[k] == 0 for k in occ), {k: scratch[k] for k in occ if scratch[k]}
    pick = lambda s: sorted(k for k in occ if s in k)
    templ = {t: pick(t + "_kernelILi") for t in ("match_fwd", "match_du", "match_dv")}
    assert all(len(v) == 6 for v in templ.values()), templ
    size = lambda k: int(re.search(r"kernelILi(\d+)E", k).group(1))
    for t, ks in templ.items():
        for k in ks:
            a = size(k)
            budget = (4 if t == "match_fwd" else 8) * a + 16
            assert vgpr[k] <= budget and lds[k] == 0, (k, vgpr[k], budget, lds[k])
            if a == 8:                                                      # the net's K 32
                assert occ[k] >= (8 if t == "match_fwd" else 5), (k, occ[k])
            assert occ[k] >= 3, (k, occ[k])
    plain = [k for k in occ if not any(k in v for v in templ.values())]
    assert len(plain) == 12 and all(occ[k] == 8 and vgpr[k] <= 64 for k in plain), {k: (occ[k], vgpr[k]) for k in plain}
    fold = pick("dmr_prefix_pool_fwd_kernel") + pick("dmr_prefix_pool_bwd_kernel") + pick("prelu_fold_kernel") + \
        pick("match_mean_kernel") + pick("dmr_tail_fwd_kernel")
    assert len(fold) == 5 and all(lds[k] == (1024 if k in fold else 0) for k in plain), {k: lds[k] for k in plain}
