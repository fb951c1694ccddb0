"""rec_ids_group_plan (host-only) against a Python restatement of the grouping sort's plan rules, over a table of
(n, N) that straddles every threshold the plan depends on — so that moving a threshold in csrc/sparse_update.hip or
csrc/radix_sort.h shows up here, on a host without a GPU, and not as silently lost coverage of
tests/test_grouping_sort_plans_gpu.py (whose cases assert their plans through the same query).

rec_ids_group_workspace_bytes must equal the size that the restated plan implies."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from _grouping_cases import MI, key_bits, plan_of, restated_plan, restated_workspace_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("REC_RSORT_DIGIT", "REC_RSORT_PACK", "REC_GROUP_DROP")

# lookups: one, the 4-wave tile edge, both sides of the packed threshold (4 Mi) and of the 16-wave one (8 Mi), the
# slot_dnn benchmark's 40 M, the largest n the entry points take
TABLE_N = (1, 2048, 2049, 4 * MI - 1, 4 * MI, 4 * MI + 1, 8 * MI - 1, 8 * MI, 8 * MI + 1, 40_000_000, (1 << 31) - 2)
# rows: one digit of 1 .. 11 bits (2047 | 2048: the widest single digit), 2 -> 3 passes (2^18), 3 -> 4 (2^27), the
# benchmark's 1.25e9 (31 bits), the 32 / 64-bit key switch (0xFFFFFFFE | 0xFFFFFFFF), 4 -> 5 passes on 64-bit keys (2^36)
TABLE_ROWS = (1, 2, 7, 500, 511, 512, 1023, 1024, 2047, 2048, 100_000, (1 << 18) - 1, 1 << 18, 26_000_000, (1 << 27) - 1,
              1 << 27, 1_250_000_000, (1 << 31) - 1, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF, 1 << 32, 5_000_000_000,
              (1 << 36) - 1, 1 << 36, 1 << 45)


def _env():
    return {k: os.environ[k] for k in SWITCHES if k in os.environ}


def test_plan_query_equals_the_restated_rules(engine_lib):
    env = _env()
    for n in TABLE_N:
        for N in TABLE_ROWS:
            assert plan_of(engine_lib, n, N) == restated_plan(n, N, env), (n, N)


def test_workspace_bytes_equal_what_the_plan_implies(engine_lib):
    env = _env()
    for n in (0,) + TABLE_N:
        for N in TABLE_ROWS:
            got = C.c_size_t(0)
            assert engine_lib.rec_ids_group_workspace_bytes(n, N, C.byref(got)) == 0
            assert got.value == restated_workspace_bytes(n, N, env), (n, N)


def test_plan_query_validates_and_needs_no_device(engine_lib):
    from paddlerec_amd import _lib
    out = _lib.IdsGroupPlan()
    assert engine_lib.rec_ids_group_plan(5, 10, None) == -1
    assert engine_lib.rec_ids_group_plan(-1, 10, C.byref(out)) == -1
    assert engine_lib.rec_ids_group_plan(5, 0, C.byref(out)) == -1
    assert engine_lib.rec_ids_group_plan((1 << 31) - 1, 10, C.byref(out)) == -2          # REC_ESHAPE, as the entry points
    assert engine_lib.rec_ids_group_plan(0, 5_000_000_000, C.byref(out)) == 0
    assert (out.passes, out.waves, out.key_bytes, out.packed, out.drop) == (0, 0, 8, 0, 0)   # n == 0: nothing is sorted


_CHILD = """
import json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from paddlerec_amd import _lib
from _grouping_cases import plan_of
print(json.dumps([plan_of(_lib.lib(), n, N) for n, N in %r]))
"""


def _child_plans(switches, cases):
    """The plans a fresh process reports under exactly `switches` (the switches are read once per process); host only."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(HERE), HERE, cases)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plans_at_every_threshold(engine_lib):
    """The same edges as literal values (the restatement could be wrong in the way the C++ is), in a child process with no
    switch set."""
    big = 1_250_000_000                                            # a configs[4] per-GPU shard: 31-bit keys in uint32_t
    want = {
        (4 * MI - 1, big): (4, [8, 8, 8, 7], 4, 4, 0),
        (4 * MI, big): (4, [8, 8, 8, 7], 4, 4, 1),                 # packed from 4 Mi lookups on
        (8 * MI, big): (4, [8, 8, 8, 7], 4, 4, 1),
        (8 * MI + 1, big): (4, [8, 8, 8, 7], 16, 4, 1),            # 16-wave blocks above 8 Mi lookups
        (8 * MI + 1, 500): (1, [9], 16, 4, 0),                     # one pass: nothing to pack
        (8 * MI + 1, 2047): (1, [11], 4, 4, 0),                    # digits above 9 bits stay on 4 waves
        (8 * MI + 1, 1023): (1, [10], 4, 4, 0),
        (1, 2048): (2, [6, 6], 4, 4, 0),                           # 12 bits: two passes
        (4 * MI, 100_000): (2, [9, 8], 4, 4, 1),
        (4 * MI, (1 << 18) - 1): (2, [9, 9], 4, 4, 1),
        (4 * MI, 1 << 18): (3, [7, 6, 6], 4, 4, 1),
        (4 * MI, 26_000_000): (3, [9, 8, 8], 4, 4, 1),
        (4 * MI, (1 << 27) - 1): (3, [9, 9, 9], 4, 4, 1),
        (4 * MI, 1 << 27): (4, [7, 7, 7, 7], 4, 4, 1),
        (8 * MI + 1, 0xFFFFFFFE): (4, [8, 8, 8, 8], 16, 4, 1),     # the sentinel is the largest uint32_t but one
        (8 * MI + 1, 0xFFFFFFFF): (4, [8, 8, 8, 8], 16, 8, 0),     # 64-bit keys are never packed
        (8 * MI + 1, 5_000_000_000): (4, [9, 8, 8, 8], 16, 8, 0),
        (8 * MI + 1, (1 << 36) - 1): (4, [9, 9, 9, 9], 16, 8, 0),
        (8 * MI + 1, 1 << 36): (5, [8, 8, 7, 7, 7], 16, 8, 0),
    }
    cases = list(want)
    for c, p in zip(cases, _child_plans({}, cases)):
        assert (p["passes"], p["bits"], p["waves"], p["key_bytes"], p["packed"]) == want[c], c
        assert p["drop"] == 1
    assert [key_bits(N) for N in (1, 2, 3, 4, 2047, 2048)] == [1, 2, 2, 3, 11, 12]


@pytest.mark.parametrize("switches", [dict(REC_RSORT_PACK="1"), dict(REC_RSORT_PACK="0", REC_GROUP_DROP="0"),
                                      dict(REC_RSORT_DIGIT="11"), dict(REC_RSORT_DIGIT="12")])
def test_plan_query_follows_the_process_wide_switches(engine_lib, switches):
    """The switches are read once per process: one child per environment (host only, no device is touched)."""
    cases = [(n, N) for n in (1, 2049, 4 * MI, 8 * MI + 1) for N in (500, 2047, 2048, 100_000, 1_250_000_000, 5_000_000_000)]
    got = _child_plans(switches, cases)
    for (n, N), g in zip(cases, got):
        assert g == restated_plan(n, N, switches), (n, N, switches)
    at = {c: g for c, g in zip(cases, got)}
    if switches.get("REC_RSORT_PACK") == "1":
        assert at[(1, 1_250_000_000)]["packed"] == 1 and at[(1, 500)]["packed"] == 0 and at[(1, 5_000_000_000)]["packed"] == 0
    if switches.get("REC_RSORT_PACK") == "0":
        assert at[(8 * MI + 1, 1_250_000_000)]["packed"] == 0 and at[(1, 500)]["drop"] == 0
    if switches.get("REC_RSORT_DIGIT") == "11":
        assert at[(8 * MI + 1, 1_250_000_000)]["bits"] == [11, 10, 10] and at[(8 * MI + 1, 1_250_000_000)]["waves"] == 4
    if switches.get("REC_RSORT_DIGIT") == "12":                      # outside 9..11: ignored
        assert at[(8 * MI + 1, 1_250_000_000)]["bits"] == [8, 8, 8, 7]
