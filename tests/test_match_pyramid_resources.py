"""What MatchPyramid's kernels (csrc/match_pyramid_ops.hip) may use — build time, no GPU: hipcc cross-compiles gfx950 and reports
each kernel's resource usage.  Resource report only: the generated code is not inspected.

  * Every kernel of the file has zero scratch bytes.  The condition: no per-lane array is indexed at run time; a lane's
    accumulators (kRT = 8 band rows, kKC = 8 channels with their best value and cell) are fixed-size and their loops unroll.
  * Registers.  mpyr_fwd_kernel (and its measurement twin mpyr_fwd_channel_kernel) and mpyr_gate_kernel hold 8 + 8 + 8 + 8 live values beside the tap loop and are held to 128
    VGPRs = 4 waves per SIMD; at the shipped shape their LDS (below) admits 4 blocks = 16 waves a CU, the same 4 per SIMD, so
    neither binds before the other.  mpyr_dcross_kernel, the fold and the hinge stream: 64 VGPRs, 8 waves per SIMD.
  * LDS, static: the forward and the gate kernel stage the right sentence's rows 16 embedding columns at a time — Rt
    [256][17] floats, Lc [8][16] floats, Rid [256] int64 = 19 968 bytes; the d_cross kernel folds 4 x 8 x 64 partial floats =
    8 192 bytes; the hinge 256 floats.
  * LDS, dynamic, from the exported constants.  Forward: weights [kh kw roundup(K, 8)] + bias + the band [(ph + kh - 1) (Lr +
    kw - 1)] floats: the shipped shape takes 4 (160 + 8 + 7 * 509) = 14 924 bytes, 34 892 with the static part: 4 blocks a CU.
    The largest shape the entries admit stays under a plain launch's 64 KiB in all three kernels (asserted below), which is
    what REC_MPYR_MAX_WEIGHTS / _BAND / _POOLED / _LEFT / _RIGHT / _EMB are set by.
  * No float atomics: the source has no atomicAdd and exactly one atomicOr(status...) site, the out-of-range id of the
    interaction band, and no other atomic call."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")
BUDGET = {"mpyr_fwd_kernel": (128, 4, 19968), "mpyr_fwd_channel_kernel": (128, 4, 19968), "mpyr_gate_kernel": (128, 4, 19968), "mpyr_fold_kernel": (64, 8, 0),
          "mpyr_dcross_kernel": (64, 8, 8192), "mpyr_hinge_kernel": (64, 8, 1024)}        # VGPRs, waves / SIMD, static LDS


def _remarks(tmp_path):
    src = os.path.join(CSRC, "match_pyramid_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "match_pyramid_ops.resources.txt")   # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "rec_common.h"), os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "mpyr.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_match_pyramid_kernels_no_scratch_and_budget(tmp_path):
    from paddlerec_amd import _lib
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
    assert len(occ) == len(BUDGET), sorted(occ)                            # every kernel of the file
    assert all(scratch[k] == 0 for k in occ), scratch                      # private segment size 0
    for k in occ:
        (kind,) = [b for b in BUDGET if b in k]
        max_vgpr, min_occ, static = BUDGET[kind]
        print("%-20s VGPRs %3d  waves/SIMD %d  static LDS %d" % (kind, vgpr[k], occ[k], lds[k]))
        assert vgpr[k] <= max_vgpr and occ[k] >= min_occ and lds[k] == static, (k, vgpr[k], occ[k], lds[k])
    # dynamic LDS at the shipped shape: Ll 20, Lr 500, E 50, K 8, filter [2, 10], pool [6, 50]
    K_ = _lib
    up8 = lambda k: (k + 7) // 8 * 8
    fwd = lambda K, kh, kw, ph, Lr: 4 * (kh * kw * up8(K) + up8(K) + (ph + kh - 1) * (Lr + kw - 1))
    assert fwd(8, 2, 10, 6, 500) == 14924 and (160 << 10) // (14924 + 19968) == 4
    gate = fwd(8, 2, 10, 6, 500) + 4 * 2 * 8 * 10
    dcross = 4 * (8 * 20 + 4 * 240 + max(500 * 8, 20 * 128 + 20 * 50))
    assert gate == 15564 and dcross == 20480 and (160 << 10) // (dcross + 8192) == 5
    # the largest admitted shape fits a plain launch (64 KiB) in every kernel
    W, P, Bd = K_.REC_MPYR_MAX_WEIGHTS, K_.REC_MPYR_MAX_POOLED, K_.REC_MPYR_MAX_BAND
    assert 4 * (W + W + Bd) + 19968 <= 64 << 10                            # forward: weights, bias (Kp <= W), band
    assert 4 * (W + W + 2 * P + Bd) + 19968 <= 64 << 10                    # gate: + the band's windows (K PW <= P), twice
    cells = max(K_.REC_MPYR_MAX_RIGHT * 8, K_.REC_MPYR_MAX_LEFT * (128 + K_.REC_MPYR_MAX_EMB))
    assert 4 * (W + 4 * P + cells) + 8192 <= 64 << 10                      # d_cross: weights, winners (4 arrays), the cells
    src = open(os.path.join(CSRC, "match_pyramid_ops.hip")).read()
    assert "atomicAdd" not in src and src.count("atomicOr(status") == 1     # the integer status flag is the only atomic
    assert len(re.findall(r"\batomic\w*\(", src)) == 1
    assert "asm" not in src
