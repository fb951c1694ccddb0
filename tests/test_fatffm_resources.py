"""Register / scratch / LDS budget of the FAT-DeepFFM kernels (csrc/fatffm_ops.hip), checked at build time: hipcc
cross-compiles gfx950 and reports each kernel's resource usage, no GPU needed.

Nine kernels: pool_fwd / inter_fwd / attn_bwd / bwd, each as the LDS-cube and the table-read instance, + the fold of the
d_dense_w partials.  None may use scratch.  On the LDS path a block's dynamic LDS is the cube image F * ffm_pitch(R, D)
floats (csrc/ffm_cube.h) + the sample's attention row a [F*F] + F*F floats of scratch (the pair sums of attn_bwd, the
argmax bytes of bwd); with the static LDS of the remarks, two blocks must fit a CU's 160 KiB at the reference shape
(S 26, Dn 13, D 10), and the registers must allow those two blocks (2 waves per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "paddlerec_amd", "csrc")
CU_LDS = 160 * 1024


def _remarks(tmp_path):
    src = os.path.join(CSRC, "fatffm_ops.hip")
    saved = os.path.join(REPO, "paddlerec_amd", "_obj", "fatffm_ops.resources.txt")    # written by paddlerec_amd.build
    deps = [src, os.path.join(CSRC, "ffm_cube.h"), os.path.join(CSRC, "rec_common.h"),
            os.path.join(REPO, "include", "recengine.h")]
    if os.path.exists(saved) and all(os.path.getmtime(d) <= os.path.getmtime(saved) for d in deps) \
            and "Occupancy" in open(saved).read():
        return open(saved).read()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                        "-I" + CSRC, "-c", src, "-o", str(tmp_path / "fatffm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def ffm_pitch(R, D):
    """csrc/ffm_cube.h: the smallest P >= round_up(R, 4) with P = D (mod 32)."""
    Rp = (R + 3) // 4 * 4
    return Rp + (D - Rp) % 32


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_fatffm_kernels_no_scratch_and_two_blocks_per_cu(tmp_path):
    occ, scratch, lds, name = {}, {}, {}, None
    for line in _remarks(tmp_path).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for pat, d in ((r"Occupancy \[waves/SIMD\]: (\d+)", occ), (r"ScratchSize \[bytes/lane\]: (\d+)", scratch),
                       (r"LDS Size \[bytes/block\]: (\d+)", lds)):
            m = re.search(pat, line)
            if m and name:
                d[name] = int(m.group(1))
    fat = sorted(k for k in occ if "fatffm_" in k)
    assert len(fat) == 9, fat
    for stem in ("pool_fwd", "inter_fwd", "attn_bwd", "bwd"):
        assert sum("fatffm_%s_kernelILb" % stem in k for k in fat) == 2, (stem, fat)
    assert all(scratch[k] == 0 for k in fat), {k: scratch[k] for k in fat}
    S, Dn, D = 26, 13, 10
    F = S + Dn
    assert ffm_pitch(F * D, D) == 394 and ffm_pitch(81, 9) == 105 and ffm_pitch(624, 16) == 624
    dynamic = (F * ffm_pitch(F * D, D) + 2 * F * F) * 4
    assert dynamic == 73632
    for k in fat:
        if "ILb1E" in k:                                     # the LDS-cube instances
            assert 2 * (lds[k] + dynamic) <= CU_LDS, (k, lds[k], dynamic)
            assert occ[k] >= 2, (k, occ[k])
