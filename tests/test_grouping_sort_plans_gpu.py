"""The grouping sort (csrc/radix_sort.h behind rec_ids_group / rec_ids_group_payload, the fallback of rec_ids_group_slots,
rec_shard_route) against a stable NumPy argsort (oracle.deepfm_ref.group_ids, oracle.shard_ref.shard_route) on EVERY plan
the sort can take — bit for bit: sorted positions, unique rows, segment offsets, n_uniq = {U, n_valid, has_long}.  The
order of the sort is part of the engine's contract (duplicates of a row are summed in ascending position order), and the
sort picks its code path from sizes the other bit-exact grouping tests never reach.

Every case first asserts, through rec_ids_group_plan, the plan it claims to cover (tests/test_grouping_plans.py holds the
plan rules themselves, without a GPU):

      n         N            passes (digit bits)  waves  keys    packed   what
  a.  4 Mi - 1  1.25e9       4 (8 8 8 7)          4      u32     no       control just under the packed threshold
      4 Mi      1.25e9       4 (8 8 8 7)          4      u32     yes      4-pass parity of the pair buffers (+ payload,
                                                                          + guarded workspace 0xFF / 0x00)
      4 Mi      100 000      2 (9 8)              4      u32     yes      2-pass parity (+ ids >= N and < 0: status flag)
      4 Mi      26 000 000   3 (9 8 8)            4      u32     yes      3-pass parity
      4 Mi      1.25e9       4 (8 8 8 7)          4      u32     yes      padding everywhere but one id
      8 Mi      1.25e9       4 (8 8 8 7)          4      u32     yes      the largest 4-wave grid
      8 Mi + 1  1.25e9       4 (8 8 8 7)          16     u32     yes      the plan of a configs[4] per-GPU shard
                                                                          (+ payload, + guarded workspace 0xFF / 0x00)
      8 Mi + 1  26 000 000   3 (9 8 8)            16     u32     yes
      8 Mi + 1  100 000      2 (9 8)              16     u32     yes
      8 Mi + 1  500          1 (9)                16     u32     no       one pass on 16 waves
      8 Mi + 1  2047         1 (11)               4      u32     no       an 11-bit digit must stay on 4 waves
      8 Mi + 1  5e9          4 (9 8 8 8)          16     u64     no       64-bit keys
  b.  n in {1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193, 20 011}, always 4 waves, unpacked:
                7 | 500 | 1000 | 2047     1 (3 | 9 | 10 | 11)    u32
                2048 | 100 000            2 (6 6 | 9 8)          u32
                26 000 000                3 (9 8 8)              u32
                1.25e9 | 0xFFFFFFFE       4 (8 8 8 7 | 8 8 8 8)  u32      the sentinel N is the largest uint32_t but one
                0xFFFFFFFF | 5e9          4 (8 8 8 8 | 9 8 8 8)  u64
  c.  the sweep of b in one fresh process per setting of the process-wide switches:
                REC_RSORT_PACK=1                      packed wherever passes >= 2 and the keys are 32-bit — the dense
                                                      small-shape coverage of the path large batches take by default
                REC_RSORT_PACK=0 REC_GROUP_DROP=0     the sentinel keys are carried through every pass
                REC_RSORT_DIGIT=11                    1.25e9: 3 (11 10 10), 26 000 000: 3 (9 8 8), 100 000: 2 (9 8)
  d.  rec_shard_route, one pass over the owner key (keys 0..G: the digit of a G-row table):
                G 511 | 512 | 1023 | 1024 at 20 020 lookups   1 (9 | 10 | 10 | 11), 4 waves
                G 8 at 8 Mi + 1 lookups                       1 (4), 16 waves
  e.  rec_ids_group_slots at its eligibility edges (B, S, R): (262 144, 2, 1000) slot-local with 32 chunks per slot |
      (262 145, 2, 1000) general; (8192, 4, 2^20) | (8192, 4, 2^20 + 1); (8192, 60, 64) | (8192, 61, 64); (8191, 26, 1000).

No tolerances anywhere: integer outputs, compared with np.array_equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import shard_ref
from _grouping_cases import (MI, SEG_LONG, SWEEP_N, SWEEP_PLANS, SWEEP_ROWS, IdsMaterial, oracle_grouping, plan_of,
                             restated_plan, sweep_ids, sweep_key)
from helpers import GuardedWorkspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_rsort_env_worker.py")
SWITCHES = ("REC_RSORT_DIGIT", "REC_RSORT_PACK", "REC_GROUP_DROP")
BIG = 1_250_000_000


@pytest.fixture(scope="module")
def ops(engine_lib):
    from paddlerec_amd import ops as o
    assert torch.cuda.is_available()
    return o


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def P(passes, bits, waves, key_bytes, packed):
    return dict(passes=passes, bits=bits, waves=waves, key_bytes=key_bytes, packed=packed, drop=1)


# (n, N) -> the plan the case claims
LARGE = {
    (4 * MI - 1, BIG): P(4, [8, 8, 8, 7], 4, 4, 0),
    (4 * MI, BIG): P(4, [8, 8, 8, 7], 4, 4, 1),
    (4 * MI, 100_000): P(2, [9, 8], 4, 4, 1),
    (4 * MI, 26_000_000): P(3, [9, 8, 8], 4, 4, 1),
    (8 * MI, BIG): P(4, [8, 8, 8, 7], 4, 4, 1),
    (8 * MI + 1, BIG): P(4, [8, 8, 8, 7], 16, 4, 1),
    (8 * MI + 1, 26_000_000): P(3, [9, 8, 8], 16, 4, 1),
    (8 * MI + 1, 100_000): P(2, [9, 8], 16, 4, 1),
    (8 * MI + 1, 500): P(1, [9], 16, 4, 0),
    (8 * MI + 1, 2047): P(1, [11], 4, 4, 0),
    (8 * MI + 1, 5_000_000_000): P(4, [9, 8, 8, 8], 16, 8, 0),
}

_material, _case = {}, {}


def large_case(n, N):
    """(host ids, device ids, oracle grouping) of a case: the random material once per n, the ids and the oracle's
    grouping once per (n, N) — shared by the tests below and never written to."""
    if (n, N) not in _case:
        if n not in _material:
            _material[n] = IdsMaterial(n)
        ids = _material[n].ids(N)
        _case[(n, N)] = (ids, T(ids), oracle_grouping(ids, N))
    return _case[(n, N)]


def assert_plan(engine_lib, n, N, want):
    got = plan_of(engine_lib, n, N)
    assert got == want, "(n %d, N %d) runs %r, the case means %r" % (n, N, got, want)


def assert_grouping(groups, want, payload=None, what=""):
    spos, uniq, offs, nu = want
    assert groups.n_uniq.tolist()[:3] == nu, what
    g_spos, g_uniq, g_offs = groups.host()
    assert np.array_equal(g_uniq, uniq), what + ": unique rows"
    assert np.array_equal(g_offs, offs), what + ": segment offsets"
    assert np.array_equal(g_spos, spos if payload is None else payload[spos]), what + ": sorted positions"


# ------------------------------------------------------------------------------------------ a. the size-gated plans
@pytest.mark.parametrize("n,N", list(LARGE))
def test_size_gated_plans(ops, engine_lib, n, N):
    assert_plan(engine_lib, n, N, LARGE[(n, N)])
    ids, tids, want = large_case(n, N)
    assert want[3][2] == 1 and want[1][0] == 1 and want[1][-1] == N - 1      # long segments; rows 1 and N - 1 are there
    groups, status = ops.ids_group(tids, N, 0, ops.Workspace(DEV))
    assert int(status.item()) == 0
    assert_grouping(groups, want, what="n %d N %d" % (n, N))


@pytest.mark.parametrize("n,N", [(4 * MI, BIG), (8 * MI + 1, BIG)])
def test_packed_plans_with_payload(ops, engine_lib, n, N):
    assert_plan(engine_lib, n, N, LARGE[(n, N)])
    ids, tids, want = large_case(n, N)
    payload = np.random.default_rng(n).integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    groups, status = ops.ids_group(tids, N, 0, ops.Workspace(DEV), payload=T(payload))
    assert int(status.item()) == 0
    assert_grouping(groups, want, payload=payload)


@pytest.mark.parametrize("n,N", [(4 * MI, BIG), (8 * MI + 1, BIG)])
def test_packed_plans_in_a_guarded_workspace(ops, engine_lib, n, N):
    """The packed pair buffers alias the key regions inside the workspace: at EXACTLY the queried bytes, on scratch that
    reads as 0xFF and again as 0x00, nothing is written outside and the bits do not depend on what the scratch held."""
    assert_plan(engine_lib, n, N, LARGE[(n, N)])
    ids, tids, want = large_case(n, N)
    need = C.c_size_t(0)
    assert engine_lib.rec_ids_group_workspace_bytes(n, N, C.byref(need)) == 0
    got = []
    for fill in (0xFF, 0x00):
        ws = GuardedWorkspace(DEV, fill=fill)
        groups, status = ops.ids_group(tids, N, 0, ws)
        torch.cuda.synchronize()
        assert ws.gets[-1][0] == need.value and ws.gets[-1][1].numel() == need.value
        assert ws.intact(), "fill 0x%02X: a guard was written" % fill
        assert int(status.item()) == 0
        assert_grouping(groups, want, what="fill 0x%02X" % fill)
        got.append(groups)
        del ws
    nv, U = want[3][1], want[3][0]
    assert torch.equal(got[0].sorted_pos[:nv], got[1].sorted_pos[:nv]) and torch.equal(got[0].n_uniq, got[1].n_uniq)
    assert torch.equal(got[0].uniq_rows[:U], got[1].uniq_rows[:U])
    assert torch.equal(got[0].seg_offset[:U + 1], got[1].seg_offset[:U + 1])


def test_packed_plan_drops_out_of_range_ids(ops, engine_lib):
    """ids >= N and negative ids: flagged, and grouped as if they were padding."""
    n, N = 4 * MI, 100_000
    assert_plan(engine_lib, n, N, LARGE[(n, N)])
    ids = large_case(n, N)[0].copy()
    at = np.random.default_rng(5).permutation(n)[:8]
    ids[at] = [N, N + 5, 1 << 40, -1, -(1 << 40), (1 << 32) + 7, -(1 << 32) + 7, (1 << 63) - 1]
    groups, status = ops.ids_group(T(ids), N, 0, ops.Workspace(DEV))
    assert int(status.item()) & 1
    ok = ids.copy()
    ok[at] = 0
    assert_grouping(groups, oracle_grouping(ok, N))


def test_packed_plan_with_one_real_id(ops, engine_lib):
    n, N = 4 * MI, BIG
    assert_plan(engine_lib, n, N, LARGE[(n, N)])
    ids = np.zeros(n, np.int64)
    ids[n - 12345] = N - 1
    groups, status = ops.ids_group(T(ids), N, 0, ops.Workspace(DEV))
    assert int(status.item()) == 0
    assert_grouping(groups, (np.array([n - 12345]), np.array([N - 1]), np.array([0, 1]), [1, 1, 0]))


# ------------------------------------------------------------------------------------------ b. small n, in process
_sweep = {}


def sweep_oracle(n, N):
    if (n, N) not in _sweep:
        _sweep[(n, N)] = oracle_grouping(sweep_ids(n, N), N)
    return _sweep[(n, N)]


@pytest.mark.parametrize("N", SWEEP_ROWS)
def test_small_n_sweep(ops, engine_lib, N):
    key_bytes, bits = SWEEP_PLANS[N]
    ws = ops.Workspace(DEV)
    for n in SWEEP_N:
        assert_plan(engine_lib, n, N, P(len(bits), bits, 4, key_bytes, 0))
        ids = sweep_ids(n, N)
        assert int(ids.max()) == N - 1                                     # around 2^32: the largest key is in the batch
        want = sweep_oracle(n, N)
        groups, status = ops.ids_group(T(ids), N, 0, ws)
        assert int(status.item()) == 0
        assert_grouping(groups, want, what="n %d N %d" % (n, N))
        if n in (1, 513, 8193, 20011):                                     # ids_rank: the inverse permutation
            rank = ops.ids_rank(groups).cpu().numpy()
            inv = np.full(n, -1, np.int32)
            inv[want[0]] = np.arange(len(want[0]), dtype=np.int32)
            assert np.array_equal(rank[:n], inv), "rank at n %d N %d" % (n, N)


# ------------------------------------------------------------------------------------------ c. process-wide switches
@pytest.mark.parametrize("switches", [dict(REC_RSORT_PACK="1"), dict(REC_RSORT_PACK="0", REC_GROUP_DROP="0"),
                                      dict(REC_RSORT_DIGIT="11")], ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_small_n_sweep_under_process_switches(engine_lib, tmp_path, switches):
    """The switches are `static const` in the library: one fresh child per setting runs the sweep of b, reports the plan
    of every case and its grouping; both are checked here."""
    out = str(tmp_path / "sweep.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, WORKER, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "%r: %s" % (switches, r.stderr[-2000:])
    got = np.load(out)
    n_packed = 0
    for N in SWEEP_ROWS:
        for n in SWEEP_N:
            k = sweep_key(n, N)
            p = restated_plan(n, N, switches)
            plan = got["plan_" + k].tolist()
            assert plan == [p["passes"], p["waves"], p["key_bytes"], p["packed"], p["drop"]] + p["bits"], (n, N, plan)
            n_packed += p["packed"]
            spos, uniq, offs, nu = sweep_oracle(n, N)
            what = "%r n %d N %d" % (switches, n, N)
            assert got["nuniq_" + k].tolist() == nu + [0], what
            assert np.array_equal(got["spos_" + k], spos), what + ": sorted positions"
            assert np.array_equal(got["uniq_" + k], uniq), what + ": unique rows"
            assert np.array_equal(got["offs_" + k], offs), what + ": segment offsets"
    # what each setting is here for, as literal values
    plan_at = lambda n, N: got["plan_" + sweep_key(n, N)].tolist()
    if switches.get("REC_RSORT_PACK") == "1":                 # every 32-bit table of >= 2 passes, at every tile edge
        assert n_packed == 5 * len(SWEEP_N)
        assert plan_at(2049, BIG) == [4, 4, 4, 1, 1, 8, 8, 8, 7] and plan_at(2049, 2048) == [2, 4, 4, 1, 1, 6, 6]
    elif switches.get("REC_GROUP_DROP") == "0":
        assert n_packed == 0 and plan_at(2049, BIG) == [4, 4, 4, 0, 0, 8, 8, 8, 7]
    else:
        assert plan_at(2049, BIG) == [3, 4, 4, 0, 1, 11, 10, 10] and plan_at(2049, 0xFFFFFFFF) == [3, 4, 8, 0, 1, 11, 11, 10]


# ------------------------------------------------------------------------------------------ d. rec_shard_route
def check_route(ops, ids, N, G):
    want = shard_ref.shard_route(ids, G, 0, None)
    route, status = ops.shard_route(T(ids), N, 0, G, ops.Workspace(DEV))
    assert int(status.item()) == 0
    k = len(want["send_pos"])
    assert np.array_equal(route.send_counts.cpu().numpy(), want["send_counts"])
    assert np.array_equal(route.send_pos[:k].cpu().numpy(), want["send_pos"])
    assert np.array_equal(route.send_local_row[:k].cpu().numpy(), want["send_local_row"])
    assert np.array_equal(route.send_sample[:k].cpu().numpy(), want["send_sample"])
    assert np.array_equal(route.slot_of_pos[:ids.size].cpu().numpy(), want["slot_of_pos"])


# rec_shard_route sorts the owner keys 0..G with rsort::make_plan(n, bits of G): the plan of a G-row table
@pytest.mark.parametrize("G,bits", [(511, 9), (512, 10), (1023, 10), (1024, 11)])
def test_shard_route_wide_one_pass_digits(ops, engine_lib, G, bits):
    B, S, N = 770, 26, 100_003
    assert_plan(engine_lib, B * S, G, P(1, [bits], 4, 4, 0))
    ids = IdsMaterial(B * S, seed=G).ids(N).reshape(B, S)
    assert len(np.unique(ids[ids != 0] % G)) > G // 2                      # most owners receive something
    check_route(ops, ids, N, G)


def test_shard_route_one_pass_on_16_waves(ops, engine_lib):
    n, N, G = 8 * MI + 1, BIG, 8
    assert_plan(engine_lib, n, G, P(1, [4], 16, 4, 0))
    check_route(ops, large_case(n, N)[0].reshape(n, 1), N, G)


# ------------------------------------------------------------------------------------------ e. rec_ids_group_slots edges
@pytest.mark.parametrize("B,S,R_,slot_local", [
    (262_144, 2, 1000, True),            # 32 chunks of 8192 per slot: the most the slot-local scatter scans
    (262_145, 2, 1000, False),
    (8192, 4, 1 << 20, True),            # the widest slot-local key: two 10-bit digits
    (8192, 4, (1 << 20) + 1, False),
    (8192, 60, 64, True),                # the most slots the transpose tile takes
    (8192, 61, 64, False),
    (8191, 26, 1000, False),             # one sample short of a slot-local tile
])
def test_group_slots_eligibility_edges(ops, engine_lib, B, S, R_, slot_local):
    from oracle import deepfm_ref as R
    # the path: the slot-local workspace differs from the general sort's for the same lookups
    a, b = C.c_size_t(0), C.c_size_t(0)
    assert engine_lib.rec_ids_group_slots_workspace_bytes(B, S, R_, C.byref(a)) == 0
    assert engine_lib.rec_ids_group_workspace_bytes(B * S, S * R_, C.byref(b)) == 0
    assert (a.value != b.value) == slot_local and ops.group_slots_eligible(B, S, R_) == slot_local
    rng = np.random.default_rng(B + S)
    ids = rng.integers(1, R_, size=(B, S), dtype=np.int64)
    ids[rng.random((B, S)) < 0.1] = 0
    ids[0, 0], ids[B - 1, S - 1] = R_ - 1, R_ - 1                          # the last row of the first and the last slot
    so = np.arange(S, dtype=np.int64) * R_
    rows, valid = R.effective_rows(ids, 0, so)
    spos, uniq, offs = R.group_ids(rows.reshape(-1), valid.reshape(-1))
    want = (spos, uniq, offs, [len(uniq), len(spos), int(np.diff(offs).max() >= SEG_LONG)])
    tids = T(ids)
    groups, status = ops.ids_group_slots(tids, R_, 0, ops.Workspace(DEV), want_rank=True)
    assert int(status.item()) == 0
    assert_grouping(groups, want)
    inv = np.full(B * S, -1, np.int32)
    inv[spos] = np.arange(len(spos), dtype=np.int32)
    assert np.array_equal(groups.rank.cpu().numpy(), inv)
    # ... and the general path over slot_offset gives the same grouping and the same rank
    g2, _ = ops.ids_group(tids, S * R_, 0, ops.Workspace(DEV), T(so))
    assert_grouping(g2, want)
    assert np.array_equal(ops.ids_rank(g2).cpu().numpy(), inv)
