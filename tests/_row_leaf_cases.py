"""The row-shape rule of csrc/rec_common.h restated in Python, and the case table of tests/test_row_leaves_gpu.py.

dispatch_row_shape(D, stride) turns a row width and the stride a call site hands it into one kernel instantiation
<VEC, LANES>: float4 lanes when D % 4 == 0 and stride % 4 == 0, else one float per lane; LANES = the next power of two
of the lanes a row needs, at most 64.  dispatch_row_shape_wide adds float4 rows of 257..1024 floats on LANES 128 / 256.
A call site that cannot use float4 for another reason (a pointer 4 bytes into its buffer, a gradient pitch that is no
multiple of 4, ...) hands the rule an odd stride (`stride | 1`) or 1 instead of 4: every such condition is a `how` below.

Nothing here touches the GPU: the completeness tests run on the CPU."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest D that selects each leaf plus one that leaves a ragged tail in it
VEC_D = [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256]
WIDE_D = [260, 1024]
SCALAR_D = [1, 2, 3, 5, 9, 17, 33, 64]


def pow2_ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def leaf(D, stride_eff, wide=False):
    """The note dispatch_row_shape / dispatch_row_shape_wide leaves for (D, stride_eff); None: the shape is refused."""
    v4 = D % 4 == 0 and stride_eff % 4 == 0
    if wide and 256 < D <= 1024:
        return "rows<4,%d>" % (128 if D <= 512 else 256) if v4 else None
    lanes = pow2_ceil(D // 4 if v4 else D)
    return "rows<%d,%d>" % (4 if v4 else 1, lanes) if lanes <= 64 else None


class Site:
    """One dispatch_row_shape( / dispatch_row_shape_wide( call site.
    conds      the conditions of the site that push a float4-eligible D onto the scalar leaf (each a `how`)
    legal      legal(D, how): the public entry point reaches the call site with this width (some sites sit behind
               another router, some cap D)
    scalar_how the `how` of the widths that are scalar by themselves ("vec" = everything aligned; a site that routes
               such widths elsewhere unless something is misaligned names that misalignment)"""

    def __init__(self, name, file, entry, conds=(), wide=False, legal=None, scalar_how="vec"):
        self.name, self.file, self.entry, self.conds, self.wide = name, file, entry, tuple(conds), wide
        self.legal = legal or (lambda D, how: True)
        self.scalar_how = scalar_how

    def hows(self):
        return tuple(dict.fromkeys(("vec", self.scalar_how) + self.conds))

    def stride_eff(self, D, how):
        """What the site hands the rule: a multiple of 4 when everything is aligned, an odd value (or 1) otherwise."""
        return 4 if how == "vec" else 1

    def predict(self, D, how):
        return leaf(D, self.stride_eff(D, how), self.wide)

    def cases(self):
        out = [(D, "vec") for D in VEC_D + (WIDE_D if self.wide else [])]
        for D in SCALAR_D:
            out += [(D, self.scalar_how)] if D % 4 else [(D, c) for c in self.conds]
        return [(D, how) for D, how in out if self.legal(D, how) and self.predict(D, how) is not None]

    def reachable(self):
        """Every leaf the rule can produce over the site's legal widths and conditions."""
        got = set()
        for D in range(1, 1025):
            for how in self.hows():
                if self.legal(D, how):
                    got.add(self.predict(D, how))
        got.discard(None)
        return got


def _adam_rows_legal(D, how):       # rows without float4 groups of at most 16 floats take the lane-per-row kernels
    return not (D <= 16 and (D % 4 != 0 or how != "vec"))


def _fm_legal(D, how):              # the row kernels of the FM pair take at most 64 lanes of float4
    return D <= 256


G = ("grad_off4", "grad_pitch")
SITES = [
    Site("emb_gather", "emb_ops.hip", "rec_emb_gather", ("odd_stride", "out_pitch", "out_off4")),
    Site("emb_gather_sumpool", "emb_ops.hip", "rec_emb_gather_sumpool", ("odd_stride",)),
    Site("emb_sumpool_bwd", "emb_ops.hip", "rec_emb_sumpool_bwd"),
    Site("record_gather", "emb_ops.hip", "rec_record_gather", ("odd_stride", "rec_off4", "out_off4")),
    Site("segment_partials", "sparse_update.hip", "rec_segment_partials", G, wide=True),
    Site("sparse_adam_rows", "sparse_update.hip", "rec_sparse_adam_rows", ("odd_stride", "state_pitch") + G, wide=True,
         legal=_adam_rows_legal),
    # the two record forms also fall back when the gradient's group_stride is no multiple of 4; ops.sparse_adam_record /
    # ops.adam_record_all always pass the layout {1, 0, 0} (contiguous rows), so only a caller of the C ABI can meet it
    Site("sparse_adam_record", "sparse_update.hip", "rec_sparse_adam_record",
         ("odd_stride", "grad_off4", "state_pitch", "v_off", "rec_off4", "mv_off4")),
    Site("adam_record_all", "sparse_update.hip", "rec_adam_record_all",
         ("odd_stride", "grad_off4", "state_pitch", "v_off", "rec_off4", "mv_off4")),
    Site("sparse_rows_sumsq", "sparse_update.hip", "rec_sparse_rows_sumsq", G),
    Site("sparse_sgd_rows", "sparse_update.hip", "rec_sparse_sgd_rows", ("odd_stride", "p_off4") + G, wide=True),
    Site("adam_rows_all", "sparse_update.hip", "rec_adam_rows_all", ("odd_stride", "state_pitch") + G, wide=True),
    # widths that are no multiple of 4 take the tile kernels unless feat / row_grad starts off a 16-byte boundary
    Site("deepfm_fm_fwd", "deepfm_fm.hip", "rec_deepfm_fm_fwd", ("odd_stride",), legal=_fm_legal, scalar_how="feat_off4"),
    Site("deepfm_fm_bwd", "deepfm_fm.hip", "rec_deepfm_fm_bwd", legal=_fm_legal, scalar_how="rg_off4"),
    Site("flen_fwd", "flen_ops.hip", "rec_flen_fwd", ("odd_stride", "w_off4", "x0_off4", "x0_pitch")),
    Site("flen_bwd", "flen_ops.hip", "rec_flen_bwd", ("g_off4", "g_pitch")),
    Site("adagrad_rows", "flen_ops.hip", "rec_adagrad_rows",
         ("odd_stride", "state_pitch", "p_off4", "a_off4") + G, wide=True),
    Site("gate_emb_fwd", "gate_ops.hip", "rec_gate_emb_fwd", ("odd_stride", "w_off4", "out_off4", "out_pitch")),
    Site("gate_emb_bwd", "gate_ops.hip", "rec_gate_emb_bwd", ("odd_stride", "w_off4", "g_off4", "g_pitch")),
    Site("autofis_fwd_eval", "autofis_ops.hip", "rec_autofis_fwd", ("odd_stride", "v_off4", "x0_off4", "x0_pitch"),
         legal=lambda D, how: D <= 64),
    Site("autofis_fwd_train", "autofis_ops.hip", "rec_autofis_fwd", ("odd_stride", "v_off4", "x0_off4", "x0_pitch"),
         legal=lambda D, how: D <= 64),
]
BY_NAME = {s.name: s for s in SITES}


def call_sites():
    """[(file, line)] of every dispatch_row_shape( / dispatch_row_shape_wide( call in csrc/*.hip."""
    found = []
    for path in sorted(glob.glob(os.path.join(REPO, "paddlerec_amd", "csrc", "*.hip"))):
        with open(path) as f:
            for no, line in enumerate(f, 1):
                found += [(os.path.basename(path), no)] * len(re.findall(r"\bdispatch_row_shape(?:_wide)?\(", line))
    return found


# ---------------------------------------------------------------------------------------------- the hand-rolled routers
def adam_narrow_note(D, v4, l2):
    return "adam_rows_narrow<%d,%d,%d>" % ((D + 3) // 4, int(v4), int(l2))


ADAM_NARROW_CASES = [(D, v4, l2) for D in range(1, 17) for v4 in (True, False) for l2 in (False, True)]


def ms_note(S, D, stride, aligned=True, lane_on=True):
    """rec_multislot_sumpool_fwd in the default environment (REC_MS_CFG unset), a table below 2^32 rows, no lazy init."""
    dp = (D + 3) // 4 * 4
    v4 = stride % 4 == 0 and stride >= dp and aligned
    if lane_on and v4 and S > 8 and 8 <= D <= 11:
        return "ms_lane<%d>" % D
    lanes = pow2_ceil(dp // 4 if v4 else D)
    banded = lanes <= (4 if v4 else 16)             # the lane counts that choose slots-per-wave by (D, S)
    if banded and D <= 10 and S > 8:
        nsw, w = 2, 8
    elif banded and D <= 20 and S > 4:
        nsw, w = 1, 8
    else:
        nsw, w = 1, 4
    return "ms_rows<%d,%d,%d,%d>" % (4 if v4 else 1, lanes, nsw, w)


# (S, D, aligned): the four lane widths; S bands <= 4, 5..8, > 8 x every lane count of both lane kinds (float4: D 1..4 ->
# 1 lane, 5 -> 2, 10 / 12 -> 4, 20 / 24 -> 8, 33 / 64 -> 16; scalar: D 1, 2, 3..4, 5, 10 / 12, 20 / 24, 33 / 64 -> 1 .. 64
# lanes), which also walks the D bands <= 10, <= 20, wider
MS_CASES = [(12, D, True) for D in (8, 9, 10, 11)] + \
           [(S, D, al) for S in (3, 7, 12) for D in (1, 2, 3, 4, 5, 10, 12, 20, 24, 33, 64) for al in (True, False)]
MS_BANDS = {"1,4>", "1,8>", "2,8>"}                  # (NSW, WAVES) of the default environment
# every ms_rows leaf the default environment can launch: the lane counts that choose by (D, S) take all three bands (a
# lane count whose widths all exceed a band's D limit cannot take it), the wide ones only <1, 4>
MS_LEAVES = {"ms_rows<4,%d,%s" % (l, b) for l in (1, 2, 4) for b in MS_BANDS} | \
            {"ms_rows<4,%d,1,4>" % l for l in (8, 16)} | \
            {"ms_rows<1,%d,%s" % (l, b) for l in (1, 2, 4, 8) for b in MS_BANDS} | \
            {"ms_rows<1,16,%s" % b for b in MS_BANDS} | {"ms_rows<1,%d,1,4>" % l for l in (32, 64)}
