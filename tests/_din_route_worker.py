"""One process of tests/test_din_gpu.py: the DIN attention pair under the process-wide switches of the environment.
REC_DIN_TILE_SPLIT, REC_DIN_TICKETS, REC_DIN_FWD_VARIANT, REC_DIN_FWD_GENERIC and REC_DIN_BWD_GENERIC are read once per
process (function-local statics of din_fwd_run / din_bwd_run in csrc/din_attention.hip), hence a process per setting.

    REC_DIN_TILE_SPLIT=0 python tests/_din_route_worker.py <in.npz> <out.npz>

in.npz holds any number of problems, "<name>__<array>" with the arrays of problem() below, and "<name>__mode" =
[fwd_ws, use_saved, bwd_ws].  Writes per problem: out, attw, dh, dq, status and the route log of the forward and of the
backward call ("<name>__fwd_route", "<name>__bwd_route": arrays of notes).  The parent test imports problem() and run() to
build the inputs and to run the same calls in its own process."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ARRAYS = ("hi", "hc", "tis", "tcs", "mask", "tab0", "tab1", "tab2", "tab3", "aw0", "aw1", "aw2", "ab0", "ab1", "ab2", "dout")


def problem(B, Tn, Ei, Ec, seed, ni=200, nc=41, H1=80, H2=40):
    """A DIN attention problem as NumPy arrays: histories of random length (sample 0 full), ids >= 1, the mask the
    reference builds (0 valid / -1e9 padding), target ids repeated along the history."""
    rng = np.random.default_rng(seed)
    E = Ei + Ec
    p = {}
    for k, (n, d) in enumerate(((ni, Ei), (nc, Ec), (ni, Ei), (nc, Ec))):
        p["tab%d" % k] = rng.uniform(-0.3, 0.3, (n, d)).astype(np.float32)
    lens = rng.integers(1, Tn + 1, B)
    lens[0] = Tn
    valid = np.arange(Tn)[None] < lens[:, None]
    p["hi"] = np.where(valid, rng.integers(1, ni, (B, Tn)), 0).astype(np.int64)
    p["hc"] = np.where(valid, rng.integers(1, nc, (B, Tn)), 0).astype(np.int64)
    p["mask"] = np.where(valid, 0, -1000000000).astype(np.int64)
    p["tis"] = np.repeat(rng.integers(1, ni, B)[:, None], Tn, 1).astype(np.int64)
    p["tcs"] = np.repeat(rng.integers(1, nc, B)[:, None], Tn, 1).astype(np.int64)
    for k, sh in enumerate(((4 * E, H1), (H1, H2), (H2, 1))):
        p["aw%d" % k] = rng.uniform(-0.3, 0.3, sh).astype(np.float32)
        p["ab%d" % k] = rng.uniform(-0.1, 0.1, sh[1:]).astype(np.float32)
    p["dout"] = rng.standard_normal((B, E)).astype(np.float32)
    return p


def run(p, fwd_ws, use_saved, bwd_ws, dev="cuda"):
    """Forward then backward of one problem -> dict of NumPy results and the two route logs.  fwd_ws / bwd_ws: the call
    goes through the _ws entry point with the workspace its query names; use_saved: the backward gets what the forward
    saved."""
    from paddlerec_amd import ops
    t = {k: torch.as_tensor(np.ascontiguousarray(p[k])).to(dev) for k in ARRAYS}
    tabs = [t["tab%d" % k] for k in range(4)]
    aw, ab = [t["aw%d" % k] for k in range(3)], [t["ab%d" % k] for k in range(3)]
    ids = [t[k] for k in ("hi", "hc", "tis", "tcs")]
    saved = {} if use_saved else None
    with ops.route_log() as fwd_route:
        out, attw, status = ops.din_attention_pool(*ids, t["mask"], *tabs, aw, ab, saved=saved,
                                                   ws=ops.Workspace(dev) if fwd_ws else None)
    with ops.route_log() as bwd_route:
        dh, dq = ops.din_attention_pool_bwd(*ids, *tabs, aw, ab, attw, t["dout"], saved=saved,
                                            ws=ops.Workspace(dev) if bwd_ws else None)
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), attw=attw.cpu().numpy(), dh=dh.cpu().numpy(), dq=dq.cpu().numpy(),
                status=status.cpu().numpy(), fwd_route=np.array(fwd_route), bwd_route=np.array(bwd_route),
                saved_act1=np.array(int(bool(use_saved) and saved.get("act1") is not None)))


def main():
    src, dst = sys.argv[1], sys.argv[2]
    inp = np.load(src)
    names = sorted({k.split("__")[0] for k in inp.files})
    res = {}
    for name in names:
        p = {k: inp[name + "__" + k] for k in ARRAYS}
        fwd_ws, use_saved, bwd_ws = (bool(x) for x in inp[name + "__mode"])
        for k, v in run(p, fwd_ws, use_saved, bwd_ws).items():
            res[name + "__" + k] = v
    np.savez(dst, **res)


if __name__ == "__main__":
    main()
