"""Shared by tests/test_grouping_plans.py, tests/test_grouping_sort_plans_gpu.py and tests/_rsort_env_worker.py: the plan
rules of the grouping sort restated in Python (csrc/sparse_update.hip key_bits / use_u32_keys / plan_group,
csrc/radix_sort.h make_plan), the ids every case sorts, and the small-n sweep that runs in process and in one child per
process-wide switch.  No GPU, no engine import: plain integers and NumPy."""
import numpy as np

MI = 1 << 20
SEG_LONG = 128                 # REC_SEG_LONG (include/recengine.h)
FOLD_ROWS = 4000               # half of every case's ids fall into this many rows: segments of >= SEG_LONG positions


# ------------------------------------------------------------------------------------------------ the rules, restated
def _atoi(v):
    """C atoi: optional sign and leading digits, 0 when there are none."""
    v, i, sign = v.strip(), 0, 1
    if v[:1] in ("+", "-"):
        sign, i = (-1 if v[0] == "-" else 1), 1
    j = i
    while j < len(v) and v[j].isdigit():
        j += 1
    return sign * int(v[i:j]) if j > i else 0


def key_bits(N):
    b = 1
    while b < 63 and (1 << b) <= N:          # keys take the values 0..N (N = the sentinel of the dropped lookups)
        b += 1
    return b


def restated_plan(n, N, env=None):
    """dict(passes, bits, waves, key_bytes, packed, drop) of rec_ids_group for n lookups of an N-row table under the
    process environment `env` (a mapping; None: no switch set)."""
    env = env or {}
    digit_env = _atoi(env["REC_RSORT_DIGIT"]) if env.get("REC_RSORT_DIGIT") else 0
    pack = _atoi(env["REC_RSORT_PACK"]) if env.get("REC_RSORT_PACK") else -1
    drop = not env.get("REC_GROUP_DROP", "").startswith("0")
    kb = key_bits(N)
    digit = digit_env if 9 <= digit_env <= 11 else 9
    passes = 1 if kb <= 11 else -(-kb // digit)
    bits, left = [], kb
    for i in range(passes):
        bits.append(-(-left // (passes - i)))
        left -= bits[-1]
    waves = 16 if n > 8 * MI and max(bits) <= 9 else 4
    u32 = N < 0xFFFFFFFF
    packed = u32 and passes >= 2 and (pack == 1 or (pack < 0 and n >= 4 * MI))
    return dict(passes=passes, bits=bits, waves=waves, key_bytes=4 if u32 else 8, packed=int(packed), drop=int(drop))


def restated_workspace_bytes(n, N, env=None):
    """rec_ids_group_workspace_bytes: keys_tmp | keys_dst | vals_tmp (n packed pairs when the keys are 32-bit) | histogram
    matrix [bins][tiles] | bin totals | live count | per-tile head counts, every region rounded up to 256 bytes."""
    if n == 0:
        return 256
    p = restated_plan(n, N, env)
    al = lambda x: (x + 255) // 256 * 256
    ks, nb = p["key_bytes"], 1 << max(p["bits"])
    nblk = max(1, -(-n // (p["waves"] * 512)))
    return (2 * al(n * ks) + al(n * (8 if ks == 4 else 4)) + al(nb * nblk * 4) + al(nb * 4) + 256 +
            al((-(-n // 2048) + 1) * 2 * 4))


def plan_of(lib, n, N):
    """rec_ids_group_plan as the dict restated_plan returns."""
    import ctypes as C
    from paddlerec_amd import _lib
    out = _lib.IdsGroupPlan()
    rc = lib.rec_ids_group_plan(int(n), int(N), C.byref(out))
    assert rc == 0, lib.rec_last_error()
    assert all(b == 0 for b in list(out.bits)[out.passes:])
    return dict(passes=out.passes, bits=list(out.bits)[:out.passes], waves=out.waves, key_bytes=out.key_bytes,
                packed=out.packed, drop=out.drop)


# ------------------------------------------------------------------------------------------------ the ids of a case
class IdsMaterial:
    """The random material of n lookups, drawn once per n and mapped onto any table size: ids(N) is 1-D int64, half of
    the lookups uniform over [1, N), half folded into the first min(FOLD_ROWS, N - 1) rows (so that some rows own
    >= SEG_LONG positions once n is large enough), 30 % set to the padding id 0, rows N - 1 and 1 present (n >= 1 / 2)."""

    def __init__(self, n, seed=0):
        rng = np.random.default_rng(1000003 * seed + n)
        self.n = n
        self.raw = rng.integers(0, 1 << 62, size=n, dtype=np.int64)
        self.folded = rng.random(n) < 0.5
        self.padded = rng.random(n) < 0.3
        self.where = rng.permutation(n)[:2]             # positions of rows N - 1 and 1

    def ids(self, N):
        N = int(N)
        assert N >= 2
        ids = 1 + self.raw % (N - 1)
        f = self.folded
        ids[f] = 1 + self.raw[f] % min(FOLD_ROWS, N - 1)
        ids[self.padded] = 0
        if self.n >= 1:
            ids[self.where[0]] = N - 1
        if self.n >= 2:
            ids[self.where[1]] = 1
        return ids


def oracle_grouping(ids, N, pad=0):
    """oracle.deepfm_ref.group_ids (stable NumPy argsort) of 1-D ids, padding and ids outside [0, N) left out; ->
    (sorted positions, unique rows, segment offsets, [U, n_valid, has_long])."""
    from oracle import deepfm_ref as R
    valid = (ids != pad) & (ids >= 0) & (ids < N)
    spos, uniq, offs = R.group_ids(ids, valid)
    has_long = int(len(offs) > 1 and int(np.diff(offs).max()) >= SEG_LONG)
    return spos, uniq, offs, [len(uniq), len(spos), has_long]


# ------------------------------------------------------------------------------------------------ the small-n sweep
# every tile edge of the 4-wave blocks (a wave owns 512 lookups, a block 2048), one element, more than one block
SWEEP_N = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193, 20011)
# one digit of 3 / 9 / 10 / 11 bits, 2 / 3 / 4 passes, the largest 32-bit table, the smallest 64-bit one, 33-bit keys
SWEEP_ROWS = (7, 500, 1000, 2047, 2048, 100_000, 26_000_000, 1_250_000_000, 0xFFFFFFFE, 0xFFFFFFFF, 5_000_000_000)
# N -> (key bytes, digit widths) with no switch set; n <= 20 011: always 4 waves, never packed
SWEEP_PLANS = {7: (4, [3]), 500: (4, [9]), 1000: (4, [10]), 2047: (4, [11]), 2048: (4, [6, 6]), 100_000: (4, [9, 8]),
               26_000_000: (4, [9, 8, 8]), 1_250_000_000: (4, [8, 8, 8, 7]), 0xFFFFFFFE: (4, [8, 8, 8, 8]),
               0xFFFFFFFF: (8, [8, 8, 8, 8]), 5_000_000_000: (8, [9, 8, 8, 8])}

_materials = {}


def sweep_ids(n, N):
    if n not in _materials:
        _materials[n] = IdsMaterial(n, seed=7)
    return _materials[n].ids(N)


def sweep_key(n, N):
    return "%d_%d" % (n, N)
