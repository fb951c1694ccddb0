"""Host side of paddlerec_amd/csrc/exchange.hip: everything here returns before an RCCL or HIP function runs, so it
needs no GPU (tests/test_native_exchange_gpu.py runs the collectives and the link stand-in on one).

  * rec_alltoall_layout  : the counts -> bytes / displacements arithmetic of rec_alltoall_exchange, at any world size,
                           against np.cumsum in int64; what it refuses, and that a refusal writes nothing.
  * rec_link_emulate     : every argument refusal, the 1 s cap on the modelled duration among them.
  * rec_comm_* / rec_alltoall_exchange / rec_allreduce_sum_f32 : argument refusals that come before RCCL is consulted.
"""
import ctypes as C

import numpy as np
import pytest

EINVAL, ESHAPE = -1, -2
SENTINEL = -0x0123456789ABCDEF
I64_MAX = 2 ** 63 - 1


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _layout(L, world, send, recv, row_bytes, null=None):
    """Calls rec_alltoall_layout on sentinel-filled outputs (world entries and one more each; `null` names one argument
    passed as NULL); returns (rc, outputs by name)."""
    n = max(world, 1)
    out = {k: np.full(n + 1, SENTINEL, np.int64) for k in ("send_bytes", "send_displs", "recv_bytes", "recv_displs")}
    out["total_send"], out["total_recv"] = np.full(1, SENTINEL, np.int64), np.full(1, SENTINEL, np.int64)
    args = dict(out, send_counts=np.ascontiguousarray(send, np.int64), recv_counts=np.ascontiguousarray(recv, np.int64))
    if null is not None:
        args[null] = None
    rc = L.rec_alltoall_layout(world, _p(args["send_counts"]), _p(args["recv_counts"]), row_bytes,
                               _p(args["send_bytes"]), _p(args["send_displs"]), _p(args["recv_bytes"]),
                               _p(args["recv_displs"]), _p(args["total_send"]), _p(args["total_recv"]))
    return rc, out


def _untouched(out):
    return all(bool((a == SENTINEL).all()) for a in out.values())


def _count_cases(world, rng):
    """(name, send counts, recv counts) of one world size."""
    z = np.zeros(world, np.int64)
    rand = rng.integers(0, 100000, world, dtype=np.int64)
    gaps = rand.copy()
    gaps[::2] = 0                                        # zeros between non-zeros (world 1: all zero)
    one = z.copy()
    one[world // 2] = 123457                             # one peer owns everything
    big = np.full(world, 2 ** 40, np.int64)              # 2^40 rows x 64 bytes x 64 peers = 2^52 bytes: still fits
    big[-1] += 5
    return [("zero", z, z), ("random", rand, rand[::-1]), ("gaps", gaps, np.roll(gaps, 1)), ("one_owner", one, z),
            ("owner_recv", z, one), ("huge", big, big[::-1])]


@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("row_bytes", [1, 3, 8, 36, 64])
def test_alltoall_layout_equals_numpy_cumsum(engine_lib, world, row_bytes):
    rng = np.random.default_rng(1000 * world + row_bytes)
    for name, send, recv in _count_cases(world, rng):
        rc, out = _layout(engine_lib, world, send, recv, row_bytes)
        assert rc == 0, (name, engine_lib.rec_last_error())
        for side, counts in (("send", send), ("recv", recv)):
            nbytes = counts.astype(np.int64) * np.int64(row_bytes)
            ends = np.cumsum(nbytes, dtype=np.int64)
            assert int(ends[-1]) == sum(int(c) * row_bytes for c in counts)          # the int64 reference did not wrap
            assert np.array_equal(out[side + "_bytes"][:world], nbytes), (name, side)
            assert np.array_equal(out[side + "_displs"][:world], ends - nbytes), (name, side)
            assert int(out["total_" + side][0]) == int(ends[-1]), (name, side)
            assert out[side + "_bytes"][world] == SENTINEL and out[side + "_displs"][world] == SENTINEL   # world entries only


def test_alltoall_layout_refuses_bad_arguments(engine_lib):
    L = engine_lib
    ok = np.array([3, 0, 7, 1], np.int64)
    for idx in (0, 3):                                   # a negative count at the first and at the last index
        for side in (0, 1):
            bad = ok.copy()
            bad[idx] = -1
            pair = (bad, ok) if side == 0 else (ok, bad)
            rc, out = _layout(L, 4, pair[0], pair[1], 8)
            assert rc == EINVAL and b"negative" in L.rec_last_error() and _untouched(out), (idx, side)
    for rb in (0, -1):
        rc, out = _layout(L, 4, ok, ok, rb)
        assert rc == EINVAL and L.rec_last_error() and _untouched(out), rb
    for world in (0, -1):
        rc, out = _layout(L, world, ok, ok, 8)
        assert rc == EINVAL and L.rec_last_error() and _untouched(out), world
    for null in ("send_counts", "recv_counts", "send_bytes", "send_displs", "recv_bytes", "recv_displs", "total_send",
                 "total_recv"):
        rc, out = _layout(L, 4, ok, ok, 8, null=null)
        assert rc == EINVAL and b"null" in L.rec_last_error() and _untouched(out), null
    rc, out = _layout(L, 4, ok, ok, 8)                   # the same call with nothing wrong
    assert rc == 0 and out["total_send"][0] == 88


def test_alltoall_layout_refuses_what_does_not_fit_int64(engine_lib):
    """The parent of this check computed (size_t)count * row_bytes and the running sums without looking: they wrapped."""
    L = engine_lib
    z = np.zeros(3, np.int64)
    # a product that overflows: 2^61 rows x 8 bytes = 2^64 (wraps to 0 in 64 bits), in any position and on either side
    for idx in range(3):
        c = np.array([5, 5, 5], np.int64)
        c[idx] = 2 ** 61
        for send, recv in ((c, z), (z, c)):
            rc, out = _layout(L, 3, send, recv, 8)
            assert rc == ESHAPE and b"int64" in L.rec_last_error() and _untouched(out), idx
    rc, out = _layout(L, 1, [I64_MAX // 3 + 1], [0], 3)                               # 2^63 + 2: positive as size_t only
    assert rc == ESHAPE and _untouched(out)
    # a sum that overflows while every product fits: 3 x (2^59 rows x 8 bytes = 2^62)
    c = np.full(3, 2 ** 59, np.int64)
    for send, recv in ((c, z), (z, c)):
        rc, out = _layout(L, 3, send, recv, 8)
        assert rc == ESHAPE and b"int64" in L.rec_last_error() and _untouched(out)
    # the edge itself fits: a total of exactly INT64_MAX bytes
    rc, out = _layout(L, 2, [I64_MAX - 7, 7], [0, I64_MAX], 1)
    assert rc == 0 and int(out["total_send"][0]) == I64_MAX == int(out["total_recv"][0])
    assert out["send_displs"][:2].tolist() == [0, I64_MAX - 7] and out["recv_displs"][:2].tolist() == [0, 0]
    rc, out = _layout(L, 2, [I64_MAX - 7, 8], [0, 0], 1)                              # ... and one byte more does not
    assert rc == ESHAPE and _untouched(out)


# --------------------------------------------------------------------------------------------------- rec_link_emulate
RING = 1 << 20
A, B = 1 << 20, 1 << 24          # stand-ins for two device addresses, 16-byte aligned; never dereferenced: every call
                                 # in this file is refused before the first HIP call


def _link(L, nbytes=4096, rate=100.0, fixed=8.0, blocks=8, src=A, dst=B, ring=RING):
    return L.rec_link_emulate(nbytes, rate, fixed, blocks, src, dst, ring, None)


def _refused(L, **kw):
    """EINVAL, and a message of this call's own (another entry point's refusal fills the slot with its text first)."""
    assert L.rec_stream_spin(-1, None) == EINVAL
    before = L.rec_last_error()
    assert b"micros" in before
    rc = _link(L, **kw)
    msg = L.rec_last_error()
    assert rc == EINVAL and msg and msg != before, (kw, rc, msg)
    return msg


def test_link_emulate_refuses_bad_arguments(engine_lib):
    L = engine_lib
    for rate in (0.0, -1.0, float("nan")):
        _refused(L, rate=rate)
    for fixed in (-1.0, -1e-3, float("nan")):
        _refused(L, fixed=fixed)
    for blocks in (0, 65, -1):
        _refused(L, blocks=blocks)
    # the ring: a power of two in [64 KB, 2^31]
    for ring in (0, 1 << 15, 65536 - 16, 65536 + 16, 3 << 20, (1 << 31) + 16, 1 << 32):
        assert b"power of two" in _refused(L, ring=ring), ring
    for kw in (dict(src=None), dict(dst=None), dict(src=A + 8), dict(dst=B + 8), dict(src=A + 4), dict(dst=B + 1)):
        assert b"aligned" in _refused(L, **kw), kw


def test_link_emulate_caps_the_modelled_duration_at_one_second(engine_lib):
    """duration = fixed_us + bytes / (gbytes_per_s * 1e3) microseconds; above 1 s the call is refused.  Both sides of the
    limit are called with src = NULL, so that neither can reach a launch whatever the library does: a duration within
    the limit gets as far as the pointer check (its message), one above it is stopped by the cap (its message)."""
    L = engine_lib
    within = [dict(nbytes=999_999_000, rate=1.0, fixed=0.0),           # 999 999 us
              dict(nbytes=1_000_000_000, rate=1.0, fixed=0.0),         # exactly 1 s: the limit is inclusive, as rec_stream_spin's
              dict(nbytes=0, rate=1.0, fixed=999_999.0),
              dict(nbytes=499_999_000, rate=1.0, fixed=500_000.0),     # the two terms add up to 999 999 us
              dict(nbytes=2 ** 40, rate=1100.0, fixed=8.0)]            # 1 TiB at 1.1 TB/s
    above = [dict(nbytes=1_000_001_000, rate=1.0, fixed=0.0),          # 1 000 001 us
             dict(nbytes=0, rate=1.0, fixed=1_000_001.0),
             dict(nbytes=500_001_000, rate=1.0, fixed=500_000.0),
             dict(nbytes=2 ** 40, rate=1000.0, fixed=8.0),             # 1 TiB at 1 TB/s: 1.0995 s
             dict(nbytes=1 << 20, rate=1e-6, fixed=0.0),               # a tiny rate
             dict(nbytes=2 ** 64 - 1, rate=153.0, fixed=8.0)]
    for kw in within:
        assert b"aligned" in _refused(L, src=None, **kw), kw
    for kw in above:
        msg = _refused(L, src=None, **kw)
        assert b"duration" in msg and b"aligned" not in msg, (kw, msg)
        assert b"duration" in _refused(L, **kw), kw                    # and with nothing else wrong with the call
    assert L.rec_stream_spin(1_000_001, None) == EINVAL                # the sibling's limit, for the record


# ------------------------------------------------------------------------------- communicator entry points, arguments
def _rccl_maps():
    with open("/proc/self/maps") as f:
        return sorted({ln.split()[-1] for ln in f if "rccl" in ln})


def test_comm_entry_points_refuse_bad_arguments_before_rccl(engine_lib):
    """Every refusal below is made from the arguments alone: the message is the argument check's (never RCCL's), no
    communicator is written, and no RCCL library is mapped by the calls."""
    L = engine_lib
    maps = _rccl_maps()
    ident = (C.c_char * 128)()
    idp = C.cast(ident, C.c_void_p)
    comm = C.c_void_p()
    fake = C.c_void_p(4096)                                            # a non-null communicator value; never used

    def refused(rc):
        msg = L.rec_last_error()
        assert rc == EINVAL and msg and b"RCCL" not in msg and b"nccl" not in msg, (rc, msg)

    refused(L.rec_comm_unique_id(None))
    refused(L.rec_comm_init(None, 1, 0, C.byref(comm)))
    refused(L.rec_comm_init(idp, 1, 0, None))
    refused(L.rec_comm_init(idp, 0, 0, C.byref(comm)))
    refused(L.rec_comm_init(idp, 1, -1, C.byref(comm)))
    refused(L.rec_comm_init(idp, 1, 1, C.byref(comm)))
    refused(L.rec_comm_init(idp, 8, 8, C.byref(comm)))
    assert comm.value is None
    n = C.c_int32(-7)
    refused(L.rec_comm_size(None, C.byref(n)))
    refused(L.rec_comm_size(fake, None))
    assert n.value == -7
    one = (C.c_int64 * 1)(1)
    refused(L.rec_alltoall_exchange(None, fake, one, fake, one, 8, None))
    refused(L.rec_alltoall_exchange(fake, fake, one, fake, one, 0, None))
    refused(L.rec_alltoall_exchange(fake, fake, one, fake, one, -4, None))
    refused(L.rec_alltoall_exchange(fake, fake, None, fake, one, 8, None))
    refused(L.rec_alltoall_exchange(fake, fake, one, fake, None, 8, None))
    refused(L.rec_allreduce_sum_f32(None, fake, 4, None))
    refused(L.rec_allreduce_sum_f32(fake, fake, -1, None))
    refused(L.rec_allreduce_sum_f32(fake, None, 4, None))
    assert L.rec_allreduce_sum_f32(fake, None, 0, None) == 0           # nothing to reduce: returns before RCCL as well
    assert L.rec_comm_destroy(None) == 0
    assert _rccl_maps() == maps


def test_comm_available_answers_and_never_fails(engine_lib):
    L = engine_lib
    first = L.rec_comm_available()
    assert first in (0, 1)
    assert L.rec_comm_available() == first                             # resolved once per process
    assert L.rec_comm_destroy(None) == 0                               # REC_OK with or without RCCL
