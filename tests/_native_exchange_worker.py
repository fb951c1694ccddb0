"""The one child process of tests/test_native_exchange_gpu.py: an nccl process group of world 1 on cuda:0, and in it every
check of the native RCCL exchange (paddlerec_amd/csrc/exchange.hip behind paddlerec_amd.sharded.Comm) and of the link
stand-in rec_link_emulate.  ONE RCCL initialisation serves the whole test module.

    python tests/_native_exchange_worker.py <outdir>

Writes <outdir>/facts.json (what was observed, per group a..e of the test module) and one <outdir>/step_*.npz per
sharded run.  Comparisons of large buffers are made here and reported as mismatch counts; the pytest functions assert.
Nothing in here retries, and an exception ends the process with a non-zero status.
"""
import contextlib
import ctypes as C
import io
import json
import os
import socket
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from _sharded_worker import CFG, later_ids  # noqa: E402
from helpers import deepfm_state_dict, layer_moments, make_deepfm_problem  # noqa: E402

DEV = torch.device("cuda", 0)
SENT = 0xA5                                   # sentinel byte of every output buffer
PAD_ROWS = 37                                 # rows behind the window an exchange writes
ROW_TYPES = (("int64", torch.int64, ()), ("float32x9", torch.float32, (9,)), ("float32x16", torch.float32, (16,)),
             ("uint8x3", torch.uint8, (3,)))
A2A_SIZES = (0, 1, 1000, 70001)
ALLREDUCE_SIZES = (0, 1, 3, 2 ** 20 + 3)
RINGS = (64 << 10, 1 << 20, 32 << 20)
BLOCKS = (1, 8, 64)
ITER = 16384                                  # bytes one workgroup of rec_link_emulate moves per iteration


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr() if t.numel() else 0)


def as_bytes(t):
    """Host uint8 copy of a contiguous tensor's memory."""
    if t.numel() == 0:
        return np.empty(0, np.uint8)
    return t.detach().contiguous().view(torch.uint8).reshape(-1).cpu().numpy().copy()


def make_comm(**env):
    """Comm() under the given environment (read in its constructor); returns (comm, what it printed on stderr)."""
    from paddlerec_amd.sharded import Comm
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stderr(buf):
            comm = Comm()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    sys.stderr.write(buf.getvalue())
    return comm, buf.getvalue()


# ------------------------------------------------------------------------------------------------- a. communicator
def check_communicator(L, facts):
    comm, said = make_comm(REC_NATIVE_EXCHANGE="1")
    f = dict(native=comm.native is not None, native_ranks=comm.native_ranks, timed_out=comm.native_init_timed_out,
             warned="FAILED" in said, staged=comm.staged, available=int(L.rec_comm_available()))
    if comm.native is not None:
        n = C.c_int32(-1)
        f["size_rc"] = L.rec_comm_size(comm.native, C.byref(n))
        f["size"] = n.value
        # a second communicator of its own unique id, made only to be destroyed
        raw = (C.c_char * 128)()
        f["id_rc"] = L.rec_comm_unique_id(C.cast(raw, C.c_void_p))
        h = C.c_void_p()
        f["init_rc"] = L.rec_comm_init(raw.raw, 1, 0, C.byref(h)) if f["id_rc"] == 0 else None
        if f["init_rc"] == 0:
            f["second_handle"] = bool(h.value) and h.value != comm.native.value
            m = C.c_int32(-1)
            f["second_size_rc"] = L.rec_comm_size(h, C.byref(m))
            f["second_size"] = m.value
            f["destroy_rc"] = L.rec_comm_destroy(h)
        f["last_error"] = L.rec_last_error().decode("utf-8", "replace") if any(
            f.get(k) not in (0, None) for k in ("size_rc", "id_rc", "init_rc", "second_size_rc", "destroy_rc")) else ""
    facts["communicator"] = f
    return comm


# -------------------------------------------------------------------------------------------------- b. all-to-all
def random_rows(rng, n, dtype, tail):
    """[n, *tail] of random bit patterns; float rows carry NaNs with payloads, infinities and denormals."""
    shape = (n,) + tail
    if n == 0:
        return torch.empty(shape, dtype=dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
    if dtype == torch.float32 and n:
        w = raw.view(np.uint32)
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000],
                           np.uint32)
        w[:: max(1, w.size // 64)][: special.size] = special[: w[:: max(1, w.size // 64)].size]
    return torch.from_numpy(raw).view(dtype).reshape(shape)


def check_all_to_all(L, comm, facts):
    from paddlerec_amd.ops import RecError
    rng = np.random.default_rng(2024)
    cases = {}
    for name, dtype, tail in ROW_TYPES:
        for n in A2A_SIZES:
            host = random_rows(rng, n, dtype, tail)
            want = as_bytes(host)
            inp = host.to(DEV)
            row_bytes = inp.element_size() * (tail[0] if tail else 1)
            res = dict(row_bytes=row_bytes, nan_words=int(np.isnan(host.numpy()).sum()) if dtype == torch.float32 else 0)
            for route in ("comm", "direct"):
                big = torch.full(((n + PAD_ROWS) * row_bytes,), SENT, dtype=torch.uint8, device=DEV)
                out = big[: n * row_bytes].view(dtype).reshape((n,) + tail)
                if route == "comm":
                    got = comm.all_to_all(out, inp, [n], [n])
                    res["comm_returns_out"] = got.data_ptr() == out.data_ptr() and got.shape == out.shape
                else:
                    counts = (C.c_int64 * 1)(n)
                    res["direct_rc"] = L.rec_alltoall_exchange(comm.native, ptr(inp), counts, ptr(out), counts, row_bytes,
                                                               stream_ptr())
                torch.cuda.synchronize()
                b = big.cpu().numpy()
                res[route + "_mismatch"] = int((b[: n * row_bytes] != want).sum())
                res[route + "_tail_touched"] = int((b[n * row_bytes:] != SENT).sum())
                res[route + "_input_changed"] = int((as_bytes(inp) != want).sum())
            cases["%s,n=%d" % (name, n)] = res
    f = dict(cases=cases)
    # nothing to move and no buffers at all
    zero = (C.c_int64 * 1)(0)
    f["null_rc"] = L.rec_alltoall_exchange(comm.native, None, zero, None, zero, 8, stream_ptr())
    # a non-contiguous side is refused before anything is called
    wide = torch.arange(40 * 16, dtype=torch.float32, device=DEV).reshape(40, 16)
    strided, dense = wide[:, :9], wide[:, :9].contiguous()
    target = torch.full((40, 16), -3.0, dtype=torch.float32, device=DEV)
    before = L.rec_last_error()
    raised = {}
    for key, (o, i) in dict(inp=(torch.full((40, 9), -3.0, device=DEV), strided), out=(target[:, :9], dense)).items():
        try:
            comm.all_to_all(o, i, [40], [40])
            raised[key] = "nothing"
        except RecError as e:
            raised[key] = "RecError: %s" % e
        torch.cuda.synchronize()
        raised[key + "_output_untouched"] = bool((o == -3.0).all().item())
    f["noncontiguous"] = raised
    f["noncontiguous_made_no_call"] = L.rec_last_error() == before
    cnt = torch.tensor([12345], dtype=torch.int64, device=DEV)
    back = comm.exchange_counts_device(cnt)
    torch.cuda.synchronize()
    f["counts_device"] = [back.tolist(), cnt.tolist(), back.data_ptr() != cnt.data_ptr()]
    facts["all_to_all"] = f


# --------------------------------------------------------------------------------------------------- c. all-reduce
class CountingDist:
    """torch.distributed with its all_reduce calls counted (Comm reaches it as self.dist)."""

    def __init__(self, real):
        self._real, self.all_reduces = real, 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def all_reduce(self, *a, **k):
        self.all_reduces += 1
        return self._real.all_reduce(*a, **k)


def finite_bits(rng, n):
    """n float32 of random bit patterns, NaNs replaced; +-inf, +-0 and denormals among them."""
    w = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    nan = ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)
    w[nan] &= np.uint32(0xFF800000)                                       # a NaN becomes the infinity of its sign
    special = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF], np.uint32)
    if n >= special.size:
        w[-special.size:] = special
    return w


def check_all_reduce(L, comm, facts):
    rng = np.random.default_rng(7)
    real = comm.dist
    comm.dist = counting = CountingDist(real)
    f = {}
    try:
        for n in ALLREDUCE_SIZES:
            bits = finite_bits(rng, n)
            res = dict(nans=int(np.isnan(bits.view(np.float32)).sum()))
            for route in ("comm", "direct"):
                t = torch.from_numpy(bits.copy()).view(torch.float32).to(DEV)
                calls = counting.all_reduces
                if route == "comm":
                    comm.all_reduce_sum(t)
                else:
                    res["direct_rc"] = L.rec_allreduce_sum_f32(comm.native, ptr(t), n, stream_ptr())
                torch.cuda.synchronize()
                res[route + "_mismatch"] = int((as_bytes(t).view(np.uint32) != bits).sum())
                res[route + "_torch_calls"] = counting.all_reduces - calls
            f["n=%d" % n] = res
        # what the native entry point does not take goes through torch.distributed, and a sum over one rank changes nothing
        base = torch.from_numpy(finite_bits(rng, 15).copy()).view(torch.float32).to(DEV).reshape(3, 5)
        keep = as_bytes(base)
        view = base.t()                                                   # dense, not contiguous
        calls = counting.all_reduces
        comm.all_reduce_sum(view)
        torch.cuda.synchronize()
        f["noncontiguous"] = dict(contiguous=view.is_contiguous(), torch_calls=counting.all_reduces - calls,
                                  mismatch=int((as_bytes(base) != keep).sum()))
        ints = torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, 1001, dtype=np.int64)).to(DEV)
        keep = as_bytes(ints)
        calls = counting.all_reduces
        comm.all_reduce_sum(ints)
        torch.cuda.synchronize()
        f["int64"] = dict(torch_calls=counting.all_reduces - calls, mismatch=int((as_bytes(ints) != keep).sum()))
    finally:
        comm.dist = real
    facts["all_reduce"] = f


# ------------------------------------------------------------------------------ d. the sharded step on either exchange
def sharded_run(comm, tables, zipf, dedup):
    """tests/_sharded_worker.py's run at world 1 on `comm`: CFG's problem, two train_steps; the same outputs."""
    from paddlerec_amd.sharded import ShardedDeepFMLayer
    c = CFG
    pr = make_deepfm_problem(B=c["B"], N=c["N"], D=c["D"], fc=c["fc"], seed=c["seed"], pad_frac=c["pad_frac"],
                             tables=tables, zipf=zipf)
    so = pr["slot_offsets"]
    comm.trace = []
    torch.manual_seed(1000)
    m = ShardedDeepFMLayer(pr["N"], c["D"], 13, 26, list(c["fc"]), device=str(DEV),
                           slot_offset=None if so is None else torch.as_tensor(so), comm=comm, dedup=dedup)
    m.set_dict(deepfm_state_dict(pr["params"], len(c["fc"]) + 1))
    rng = np.random.default_rng(c["seed"] + 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    batches = []
    for step in range(c["steps"]):
        if step == 0:
            ids, dense, label = pr["ids"], pr["dense"], pr["label"]
        else:
            ids = later_ids(rng, c, 1, zipf)
            dense = rng.random((c["B"], 13), dtype=np.float32)
            label = (rng.random((c["B"], 1)) < 0.3).astype(np.int64)
        batches.append((t(ids), t(dense), t(label)))
    out = {}
    for step, (ids_t, dense_t, label_t) in enumerate(batches):
        nxt = batches[step + 1][0] if step + 1 < len(batches) else None
        loss, pred = m.train_step(ids_t, dense_t, label_t, lr=c["lr"], next_sparse_inputs=nxt)
        out["loss%d" % step] = loss.cpu().numpy().copy()
        out["pred%d" % step] = pred.cpu().numpy().copy()
    out["pred_eval"] = m.forward(t(pr["ids"]), t(pr["dense"])).cpu().numpy()
    W, W1 = m.gather_global_tables()
    out["W"], out["W1"] = W.cpu().numpy(), W1.cpu().numpy()
    out["dense_flat"] = m.dense.data.detach().cpu().numpy().copy()           # EVERY dense parameter, one flat buffer
    out["mlp_w0"] = m.dense.p["dnn.linear_0.weight"].cpu().numpy()
    out["dense_w"] = m.dense.p["fm.dense_w"].cpu().numpy()
    out["dense_m_flat"] = m.dense.m.detach().cpu().numpy().copy()            # ... and both of their Adam moments
    out["dense_v_flat"] = m.dense.v.detach().cpu().numpy().copy()
    mom = layer_moments(m)
    out["m_mlp_w0"], out["v_mlp_w0"] = mom["dnn.linear_0.weight"]
    out["m_dense_w"], out["v_dense_w"] = mom["fm.dense_w"]
    out["mW_local"] = m.sparse_state["m"].cpu().numpy()
    out["vW_local"] = m.sparse_state["v"].cpu().numpy()
    out["table_rec"] = m.fm.rec.cpu().numpy()                # every row's record line: W, W1 and W1's two moments
    out["table_mv"] = m.sparse_state["mv"].cpu().numpy()     # ... and W's two moments
    out["status"] = m.status.cpu().numpy()
    out["trace"] = np.asarray(comm.trace)
    comm.trace = None
    return out


def check_sharded_step(native, facts, outdir):
    plain, said = make_comm(REC_NATIVE_EXCHANGE="0")
    f = dict(torch_comm_native=plain.native is not None, torch_comm_ranks=plain.native_ranks, torch_comm_said=said,
             runs=[])
    for dedup in (False, True):
        for tables in (False, True):
            for zipf in (False, True):
                tag = "dedup%d_tables%d_zipf%d" % (dedup, tables, zipf)
                for which, comm in (("native", native), ("torch", plain)):
                    np.savez(os.path.join(outdir, "step_%s_%s.npz" % (which, tag)), **sharded_run(comm, tables, zipf, dedup))
                f["runs"].append(dict(tag=tag, dedup=dedup, tables=tables, zipf=zipf))
    facts["sharded_step"] = f


# ------------------------------------------------------------------------------------------------ e. rec_link_emulate
def link_cases(ring, blocks):
    """(name, bytes) of one ring size and workgroup count."""
    cases = [("zero", 0), ("one_iteration_each", blocks * ITER), ("ragged_share", blocks * (2 * ITER + 4001) + min(blocks - 1, 3)),      # odd share: bases off 16 bytes
             ("wraps", 4 * ring)]
    if blocks > 1:
        cases.insert(1, ("share_of_zero", blocks - 1))
    return cases


def windows(nbytes, blocks, ring):
    """Byte ranges [lo, hi) of the ring (no wrap inside a range) that the workgroups may write."""
    mask = (ring - 1) & ~15
    share = nbytes // blocks
    length = -(-share // ITER) * ITER
    out = []
    if length == 0:
        return out
    if length >= ring:
        return [(0, ring)]
    for b in range(blocks):
        lo = (b * share) & mask
        hi = lo + length
        out += [(lo, hi)] if hi <= ring else [(lo, ring), (0, hi - ring)]
    return out


def timer_slack_us():
    """The largest reading of 20 event pairs with nothing between them."""
    worst = 0.0
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        b.record()
        b.synchronize()
        worst = max(worst, a.elapsed_time(b) * 1e3)
    return worst


def check_link_emulate(L, facts):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(99)
    f = dict(slack_us=timer_slack_us(), cases=[])
    for ring in RINGS:
        src = torch.randint(0, 256, (ring,), dtype=torch.uint8, device=DEV, generator=gen)
        keep = src.clone()
        inv = src.bitwise_not()
        dst = torch.empty_like(src)
        allowed = torch.empty(ring, dtype=torch.bool, device=DEV)
        for blocks in BLOCKS:
            for k, (name, nbytes) in enumerate(link_cases(ring, blocks)):
                dst.copy_(inv)
                # modelled duration 200 us .. 2 ms: a fixed part of 200 us and 100 .. 1800 us of transfer
                fixed_us = 200.0
                transfer_us = 0.0 if nbytes == 0 else (100.0, 300.0, 700.0, 1800.0)[(k + blocks) % 4]
                rate = 100.0 if nbytes == 0 else max(nbytes / (transfer_us * 1e3), 1e-3)
                rate = float(np.float32(rate))                           # what the C ABI receives
                modelled_us = fixed_us + nbytes / (rate * 1e3)
                assert 200.0 <= modelled_us <= 2200.0, (name, modelled_us)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = L.rec_link_emulate(nbytes, rate, fixed_us, blocks, ptr(src), ptr(dst), ring, stream_ptr())
                e1.record()
                torch.cuda.synchronize()
                allowed.zero_()
                for lo, hi in windows(nbytes, blocks, ring):
                    allowed[lo:hi] = True
                copied = dst == src
                kept = dst == inv
                f["cases"].append(dict(
                    ring=ring, blocks=blocks, name=name, bytes=nbytes, rate=rate, rc=rc, modelled_us=modelled_us,
                    elapsed_us=e0.elapsed_time(e1) * 1e3,
                    neither=int((~(copied | kept)).sum().item()),                    # bytes that are neither src nor ~src
                    outside_touched=int((~kept & ~allowed).sum().item()),           # bytes changed outside every window
                    src_changed=int((src != keep).sum().item()),
                    window_bytes=int(allowed.sum().item()), copied_bytes=int(copied.sum().item())))
    # Comm._emulate_link behind a collective (REC_EMULATE_LINKS=8)
    comm, said = make_comm(REC_EMULATE_LINKS="8", REC_NATIVE_EXCHANGE="1")
    n = 70001
    inp = torch.from_numpy(np.random.default_rng(5).integers(0, 256, n * 64, dtype=np.uint8)).view(torch.float32)
    inp = inp.reshape(n, 16).to(DEV)
    out = torch.full((n, 16), -3.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    comm.all_to_all(out, inp, [n], [n])
    e1.record()
    torch.cuda.synchronize()
    f["via_comm"] = dict(emulate=comm.emulate, native=comm.native is not None, warned="FAILED" in said,
                         ring_allocated=comm._emu_ring is not None,
                         mismatch=int((as_bytes(out) != as_bytes(inp)).sum()),
                         modelled_us=8.0 + (n * 64 * 7 // 8) / (7 * 153.0 * 1e3), elapsed_us=e0.elapsed_time(e1) * 1e3)
    facts["link_emulate"] = f


def main():
    outdir = sys.argv[1]
    t0 = time.time()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), REC_NATIVE_INIT_TIMEOUT="30")
    torch.cuda.set_device(DEV)
    dist.init_process_group("nccl", device_id=DEV, rank=0, world_size=1)
    from paddlerec_amd._lib import lib
    L = lib()
    facts = dict(queues_env=os.environ.get("GPU_MAX_HW_QUEUES"))
    native = check_communicator(L, facts)
    facts["init_seconds"] = time.time() - t0
    if native.native is not None:                 # without it there is nothing to cover: the parent fails on the facts
        check_all_to_all(L, native, facts)
        check_all_reduce(L, native, facts)
        check_sharded_step(native, facts, outdir)
        check_link_emulate(L, facts)
    torch.cuda.synchronize()
    facts["seconds"] = time.time() - t0
    with open(os.path.join(outdir, "facts.json"), "w") as fh:
        json.dump(facts, fh, indent=1)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
