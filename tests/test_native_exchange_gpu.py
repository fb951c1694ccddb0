"""The native RCCL exchange (paddlerec_amd/csrc/exchange.hip behind paddlerec_amd.sharded.Comm on an nccl group) and the
link stand-in rec_link_emulate, on one GPU.

RCCL wants a process group of its own, so ONE fresh child (tests/_native_exchange_worker.py) makes an nccl group of
world 1, runs every check in it and writes what it saw; the tests below share that output and each asserts one group of
facts.  The child is started once, without a second try: if it fails or runs out of time, every test of this module fails
with its stderr and nothing more is started on the GPU from here.  (More than one rank is out of reach: RCCL refuses two
ranks on one device.  tests/test_exchange_host.py covers the displacement arithmetic of any world size on the host.)

Time limits: REC_NATIVE_INIT_TIMEOUT = 30 s inside the child, 120 s (four times that) for the child as a whole.
Measured on an MI355X: the child takes 5.6 s, 4.5 s of it until the communicator stands.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "_native_exchange_worker.py")
CHILD_TIMEOUT = 120


_CHILD = {}        # the child's outcome, success or failure: it is started at most once per session


@pytest.fixture(scope="module")
def child(engine_lib, tmp_path_factory):
    """{"facts": ..., "dir": ...} of the one child run; started on first use, never again."""
    if "result" not in _CHILD:
        outdir = str(tmp_path_factory.mktemp("native_exchange"))
        try:
            r = subprocess.run([sys.executable, WORKER, outdir], timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE)
            if r.returncode != 0:
                _CHILD["result"] = "the child exited with status %d:\n%s" % (
                    r.returncode, r.stderr.decode("utf-8", "replace")[-6000:])
            else:
                with open(os.path.join(outdir, "facts.json")) as f:
                    _CHILD["result"] = dict(facts=json.load(f), dir=outdir)
        except subprocess.TimeoutExpired as e:
            _CHILD["result"] = "the child did not finish within %d s:\n%s" % (
                CHILD_TIMEOUT, (e.stderr or b"").decode("utf-8", "replace")[-6000:])
    if isinstance(_CHILD["result"], str):
        pytest.fail(_CHILD["result"], pytrace=False)
    return _CHILD["result"]


@pytest.fixture(scope="module")
def facts(child):
    f = child["facts"]
    c = f["communicator"]
    # coverage of the NATIVE path is the point: a fall-back to torch.distributed's collectives is a failure of every test
    assert c["native"] and not c["warned"], "the native RCCL exchange did not come up: %r" % (c,)
    return f


# ------------------------------------------------------------------------------------------------------ a. communicator
def test_native_communicator_is_active(facts):
    c = facts["communicator"]
    assert c["staged"] is False and c["available"] == 1
    assert c["native"] is True and c["native_ranks"] == 1 and c["timed_out"] is False and c["warned"] is False
    assert c["size_rc"] == 0 and c["size"] == 1, c["last_error"]
    assert facts["seconds"] < CHILD_TIMEOUT
    print("child: %.1f s in all, %.1f s until the communicator stood" % (facts["seconds"], facts["init_seconds"]))


def test_second_communicator_is_created_and_destroyed(facts):
    c = facts["communicator"]
    assert c["id_rc"] == 0 and c["init_rc"] == 0, c["last_error"]
    assert c["second_handle"] is True and c["second_size_rc"] == 0 and c["second_size"] == 1
    assert c["destroy_rc"] == 0, c["last_error"]


# --------------------------------------------------------------------------------------------------------- b. all-to-all
A2A_CASES = ["%s,n=%d" % (t, n) for t in ("int64", "float32x9", "float32x16", "uint8x3") for n in (0, 1, 1000, 70001)]


def test_all_to_all_cases_are_the_stated_ones(facts):
    cases = facts["all_to_all"]["cases"]
    assert sorted(cases) == sorted(A2A_CASES)
    assert [cases["%s,n=1" % t]["row_bytes"] for t in ("int64", "float32x9", "float32x16", "uint8x3")] == [8, 36, 64, 3]
    assert all(cases["%s,n=%d" % (t, n)]["nan_words"] >= 2 for t in ("float32x9", "float32x16") for n in (1, 1000, 70001))


@pytest.mark.parametrize("route", ["comm", "direct"])
def test_all_to_all_world1_returns_the_input_bytes(facts, route):
    """Comm.all_to_all / rec_alltoall_exchange at world 1: every output byte is the input byte (NaN payloads included),
    the rows behind n keep their sentinel, the input is unchanged."""
    for name in A2A_CASES:
        res = facts["all_to_all"]["cases"][name]
        if route == "direct":
            assert res["direct_rc"] == 0, name
        else:
            assert res["comm_returns_out"] is True, name
        assert res[route + "_mismatch"] == 0, name
        assert res[route + "_tail_touched"] == 0, name
        assert res[route + "_input_changed"] == 0, name


def test_all_to_all_edges(facts):
    f = facts["all_to_all"]
    assert f["null_rc"] == 0                                          # n = 0 with null data pointers
    nc = f["noncontiguous"]
    for side in ("inp", "out"):
        assert nc[side].startswith("RecError") and "contiguous" in nc[side], nc
        assert nc[side + "_output_untouched"] is True
    assert f["noncontiguous_made_no_call"] is True
    back, sent, fresh = f["counts_device"]
    assert back == sent == [12345] and fresh is True


# ---------------------------------------------------------------------------------------------------------- c. all-reduce
def test_all_reduce_world1_is_the_identity(facts):
    f = facts["all_reduce"]
    for n in (0, 1, 3, 2 ** 20 + 3):
        res = f["n=%d" % n]
        assert res["nans"] == 0                                       # a sum over one rank is the identity on the rest
        assert res["direct_rc"] == 0, n
        for route in ("comm", "direct"):
            assert res[route + "_mismatch"] == 0, (n, route)
            assert res[route + "_torch_calls"] == 0, (n, route)       # the native entry point carried it


def test_all_reduce_of_other_tensors_goes_through_torch_distributed(facts):
    f = facts["all_reduce"]
    assert f["noncontiguous"] == dict(contiguous=False, torch_calls=1, mismatch=0)
    assert f["int64"] == dict(torch_calls=1, mismatch=0)


# ----------------------------------------------------------------------------- d. the sharded step on the native exchange
def _run(child, which, tag):
    return dict(np.load(os.path.join(child["dir"], "step_%s_%s.npz" % (which, tag))))


def _tag(dedup, tables, zipf):
    return "dedup%d_tables%d_zipf%d" % (dedup, tables, zipf)


def test_sharded_step_runs_are_the_stated_ones(facts):
    f = facts["sharded_step"]
    assert f["torch_comm_native"] is False and f["torch_comm_ranks"] == 0 and "FAILED" not in f["torch_comm_said"]
    assert sorted(r["tag"] for r in f["runs"]) == sorted(_tag(d, t, z) for d in (0, 1) for t in (0, 1) for z in (0, 1))


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("zipf", [False, True])
def test_sharded_step_native_equals_torch_distributed_bitwise(child, facts, dedup, tables, zipf):
    """The exchange only moves bytes; kernels and their order are the same: loss, predictions, every dense parameter, the
    tables, the optimizer state and the sequence of collectives are identical."""
    nat, ref = _run(child, "native", _tag(dedup, tables, zipf)), _run(child, "torch", _tag(dedup, tables, zipf))
    assert sorted(nat) == sorted(ref) and {"loss0", "loss1", "pred1", "dense_flat", "dense_m_flat", "dense_v_flat",
                                           "table_rec", "table_mv", "W", "W1", "trace"} <= set(nat)
    assert int(nat["status"][0]) == 0 and np.isfinite(nat["loss1"]).all()
    assert nat["trace"].tolist() == ref["trace"].tolist() and len(nat["trace"]) > 10
    assert any(t.startswith("all_to_all:float32") for t in nat["trace"].tolist()) and "all_reduce" in nat["trace"].tolist()
    for k in sorted(nat):
        if k != "trace":
            assert nat[k].dtype == ref[k].dtype and nat[k].shape == ref[k].shape, k
            assert nat[k].tobytes() == ref[k].tobytes(), k
    # the steps did something: weights and moments moved
    assert np.abs(nat["table_mv"]).max() > 0 and np.abs(nat["dense_m_flat"]).max() > 0


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("zipf", [False, True])
def test_sharded_step_native_equals_the_oracle(child, facts, tables, zipf):
    """The comparison (and tolerances) tests/test_sharded.py applies to its gloo run, on the native run."""
    from test_sharded import _check
    _check(1, [_run(child, "native", _tag(False, tables, zipf))], tables, zipf=zipf)


# ------------------------------------------------------------------------------------------------- e. rec_link_emulate
def test_link_emulate_cases_are_the_stated_ones(facts):
    cases = facts["link_emulate"]["cases"]
    assert {(c["ring"], c["blocks"]) for c in cases} == {(r, b) for r in (64 << 10, 1 << 20, 32 << 20) for b in (1, 8, 64)}
    for ring in (64 << 10, 1 << 20, 32 << 20):
        for blocks in (1, 8, 64):
            mine = {c["name"]: c for c in cases if (c["ring"], c["blocks"]) == (ring, blocks)}
            want = {"zero", "one_iteration_each", "ragged_share", "wraps"} | ({"share_of_zero"} if blocks > 1 else set())
            assert set(mine) == want
            assert mine["zero"]["bytes"] == 0 and mine["wraps"]["bytes"] == 4 * ring
            assert mine["one_iteration_each"]["bytes"] == blocks * 16384
            assert (mine["ragged_share"]["bytes"] // blocks) % 16384 != 0
            if blocks > 1:
                assert 0 < mine["share_of_zero"]["bytes"] < blocks
    assert all(c["rc"] == 0 for c in cases)


def test_link_emulate_copy_stays_in_its_windows(facts):
    """dst starts as ~src, and the copy is position-preserving: afterwards every dst byte is src or ~src at its offset,
    everything outside the workgroups' windows is still ~src, and src is unchanged.  (How much of a window was copied
    depends on timing: the kernel copies only while it is ahead of the link's schedule.  Not asserted.)"""
    for c in facts["link_emulate"]["cases"]:
        assert c["neither"] == 0, c
        assert c["outside_touched"] == 0, c
        assert c["src_changed"] == 0, c
        if c["name"] in ("zero", "share_of_zero"):
            assert c["window_bytes"] == 0
        elif c["name"] == "wraps":                   # four times the ring: the windows cover all of it
            assert c["window_bytes"] == c["ring"]
        else:
            assert 0 < c["window_bytes"] <= c["ring"]
        # a byte of src equals the byte of ~src nowhere, so "copied" counts exactly the bytes the kernel wrote
        assert c["copied_bytes"] <= c["window_bytes"], c


def test_link_emulate_lasts_the_modelled_time(facts):
    """By construction the kernel cannot return before fixed_us + bytes / (gbytes_per_s * 1e3) microseconds have passed
    on the device's wall clock.  The launch is bracketed by two events; the slack granted is the largest reading of 20
    event pairs with nothing between them, measured in the same run.  No upper bound: the card is shared.
    Measured on an MI355X: slack 6.96 us (7.12 us in a second run); in the first run the 42 launches (modelled 200 us .. 2 ms) lasted 7.7 .. 48 us longer than
    modelled (one cold first launch 453 us longer), none shorter, so the slack was not drawn on."""
    f = facts["link_emulate"]
    slack = f["slack_us"]
    print("event-timer slack %.2f us" % slack)
    assert 0.0 <= slack < 100.0                      # far below the modelled durations of 200 us and more
    for c in f["cases"]:
        assert 200.0 <= c["modelled_us"] <= 2200.0, c
        assert c["elapsed_us"] >= c["modelled_us"] - slack, c


def test_emulated_link_behind_a_collective(facts):
    """REC_EMULATE_LINKS=8: Comm.all_to_all launches the stand-in after the collective; the collective's result is the
    same, and the pair lasts at least the link's modelled time."""
    v = facts["link_emulate"]["via_comm"]
    assert v["emulate"] == 8 and v["native"] is True and v["warned"] is False
    assert v["ring_allocated"] is True and v["mismatch"] == 0
    assert v["elapsed_us"] >= v["modelled_us"] - facts["link_emulate"]["slack_us"], v
