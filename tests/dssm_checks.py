"""What tests/test_dssm.py and test_dssm_gpu.py share: the goldens evaluated once by tests/dssm_ref.py, the tolerance and the
comparison of a layer (paddlerec_amd/dssm.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/ncf_checks.py, tests/tisas_checks.py): for every tensor err = max|got - ref64| /
max|ref64|; the bound is 8 x the same error of dssm_ref.py evaluated in float32 on the same inputs, floor 1e-6.  That float32
error IS the float32 unit roundoff (2^-24) times the number of summands times the magnitude of the terms, for the sums this
very tensor is made of — measured on the inputs at hand instead of bounded from above; the factor 8 covers another summation
order (the kernels fold lanes and waves as trees, numpy sums pairwise), the floor (17 roundoffs) a tensor numpy happens to get
exactly.  The gradient through a clamped cosine is of order 1 / eps = 1e8 times its neighbours: tensors that can hold such
rows beside ordinary ones (dq, dd) are compared ROW BY ROW (check_rows), each row relative to its own largest entry.
Parameters and moments after Adam: helpers.assert_adam_weights_close and the 1e-5-of-scale bar of helpers.assert_close_scaled."""
import functools
import os

import numpy as np
import torch

import dssm_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close, assert_close_scaled

GOLDENS = ("dssm_relu.npz", "dssm_lin.npz")
CSR = ("cols", "vals", "lod")


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def check_tensor(what, name, got, r64, r32):
    e, b = R.relerr(np.asarray(got).reshape(np.shape(r64)), r64), bound_of(r32, r64)
    print("%-12s %-46s err %.3g  float32-ref err %.3g" % (what, name, e, b / 8))
    assert e <= b, (what, name, e, b)


def check_rows(what, name, got, r64, r32):
    """Every row of a [rows, n] tensor against its own scale; a row that is exactly zero in float64 must be exactly zero."""
    got, r64, r32 = (np.asarray(a, np.float64).reshape(np.shape(r64)) for a in (got, r64, r32))
    worst = 0.0
    for r in range(r64.shape[0]):
        if not r64[r].any():
            assert not got[r].any(), (what, name, r, got[r])
            continue
        e, b = R.relerr(got[r], r64[r]), bound_of(r32[r], r64[r])
        worst = max(worst, e / b)
        assert e <= b, (what, name, r, e, b)
    print("%-12s %-46s worst row at %.3g of its bound" % (what, name, worst))


def csr_of(g, prefix):
    return tuple(g["%s_%s" % (prefix, k)] for k in CSR)


def dense_of(g, prefix, width, dt=np.float64):
    return R.csr_dense(*csr_of(g, prefix), width, dt)


def ref_step(G, p, m, v, s, step):
    """dssm_ref's train step of recorded batch s from (p, m, v) in float64 and float32."""
    g, T = G["g"], G["trigram_d"]
    return [R.train_step(p, m, v, G["relu"], dense_of(g, "q_%d" % s, T, dt), dense_of(g, "d_%d" % s, T, dt), G["slice_end"],
                         step, G["lr"], dt) for dt in (np.float64, np.float32)]


@functools.lru_cache(maxsize=None)
def gold(name):
    """A golden and dssm_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE.  Computed once per
    session, never written afterwards."""
    g, p, lr, steps = R.load_golden(os.path.join(GOLDEN, name))
    G = dict(g=g, p=p, lr=lr, steps=steps, trigram_d=int(g["trigram_d"][0]), fc_sizes=g["fc_sizes"].tolist(),
             relu=[bool(x) for x in g["relu"]], slice_end=int(g["slice_end"][0]), B=int(g["B"][0]), neg=int(g["neg"][0]))
    G["fc_acts"] = ["relu" if r else "" for r in G["relu"]]
    r64, r32, cur, m, v = [], [], p, None, None
    for s in range(steps):
        a, b = ref_step(G, cur, m, v, s, s + 1)
        r64.append(a)
        r32.append(b)
        cur, m, v = ({k: g["%s_%d_%s" % (pre, s, k)] for k in p} for pre in ("n", "m", "v"))
    G.update(r64=r64, r32=r32, final=cur)
    for dt, key in ((np.float64, "inf64"), (np.float32, "inf32")):
        G[key] = R.forward_infer(cur, G["relu"], dense_of(g, "inf_q", G["trigram_d"], dt), dense_of(g, "inf_d", G["trigram_d"], dt), dt)
    return G


def check_step(r64, r32, lr, s, got, what):
    """One step's loss, cos, hit_prob, gradients, moments and post-step parameters (got: dict(loss, cos, hit_prob, g, n, m,
    v)) against the float64 reference."""
    for k in ("loss", "cos", "hit_prob"):
        check_tensor(what, "step %d %s" % (s, k), got[k], r64[k], r32[k])
    assert sorted(got["g"]) == sorted(r64["g"]), (what, sorted(got["g"]))
    for k in r64["g"]:
        check_tensor(what, "step %d g_%s" % (s, k), got["g"][k], r64["g"][k], r32["g"][k])
        assert_close_scaled(np.asarray(got["m"][k]).reshape(r64["m"][k].shape), r64["m"][k], 1e-5, err_msg="%s m of %s" % (what, k))
        assert_close_scaled(np.asarray(got["v"][k]).reshape(r64["v"][k].shape), r64["v"][k], 1e-5, err_msg="%s v of %s" % (what, k))
        assert_adam_weights_close(np.asarray(got["n"][k]).reshape(r64["n"][k].shape), r64["n"][k], lr, 1,
                                  err_msg="%s step %d %s" % (what, s, k))


def recorded_step(G, s):
    g = G["g"]
    pick = lambda pre: {k: g["%s_%d_%s" % (pre, s, k)] for k in G["p"]}
    return dict(loss=g["loss_%d" % s], cos=g["cos_%d" % s], hit_prob=g["hit_%d" % s], g=pick("g"), n=pick("n"), m=pick("m"),
                v=pick("v"))


def check_golden(G):
    """Every array the golden records, both steps and the infer call, against the float64 reference."""
    for s in range(G["steps"]):
        check_step(G["r64"][s], G["r32"][s], G["lr"], s, recorded_step(G, s), "golden")
    check_tensor("golden", "infer cos", G["g"]["inf_cos"], G["inf64"], G["inf32"])


def layer_of(G, device="cuda"):
    from paddlerec_amd.dssm import DSSMLayer
    m = DSSMLayer(G["trigram_d"], 1, G["slice_end"], G["fc_sizes"], G["fc_acts"], device=device)
    assert sorted(m.state_dict()) == sorted(G["p"])
    return m


def layer_state(m):
    npy = lambda d: {k: v.detach().cpu().numpy().copy() for k, v in d.items()}
    mm, vv = m.moments()
    return npy(m.state_dict()), npy(mm), npy(vv)


def feeds_of(G, prefix, route, device, rows=None):
    """The layer's inputs of a recorded batch: "sparse" -> [query, docs] in CSR; "general" -> the reference's list of dense
    [B, trigram_d] tensors.  rows: keep the first `rows` samples of every field."""
    g, T = G["g"], G["trigram_d"]
    q, d = dense_of(g, prefix.replace("*", "q"), T, np.float32), dense_of(g, prefix.replace("*", "d"), T, np.float32)
    B = q.shape[0]
    fields = [q] + [d[k * B:(k + 1) * B] for k in range(d.shape[0] // B)]
    if rows is not None:
        fields = [f[:rows] for f in fields]
    if route == "general":
        return [torch.as_tensor(f).to(device) for f in fields]
    from paddlerec_amd.reader import dssm_csr
    return [tuple(torch.as_tensor(a).to(device) for a in dssm_csr(list(x))[:3]) for x in (fields[0], np.concatenate(fields[1:]))]


def check_layer(G, m, route, what):
    """The recorded batches through the layer as consecutive steps, each against dssm_ref evaluated from the state the layer
    had before it; the first step is also held to the recording itself."""
    m.set_dict(G["p"])
    for s in range(G["steps"]):
        p, mm, vv = layer_state(m)
        r64, r32 = ref_step(G, p, mm, vv, s, s + 1)
        loss = m.train_step(feeds_of(G, "*_%d" % s, route, m.device), lr=G["lr"])
        n, nm, nv = layer_state(m)
        cos, hit = m.last_outputs()
        got = dict(loss=loss.cpu().numpy(), cos=cos.cpu().numpy(), hit_prob=hit.cpu().numpy(),
                   g={k: v.cpu().numpy() for k, v in m.last_gradients().items()}, n=n, m=nm, v=nv)
        check_step(r64, r32, G["lr"], s, got, what)
        assert int(m.status.item()) == 0 and int(m._group_status.item()) == 0
        if s == 0:
            rec = recorded_step(G, 0)
            for k in ("loss", "cos", "hit_prob"):
                assert R.relerr(got[k].reshape(rec[k].shape), rec[k]) <= bound_of(G["r32"][0][k], G["r64"][0][k]), (what, k)


def check_infer(G, m, route, what):
    m.set_dict(G["final"])
    cos, ones = m.forward(feeds_of(G, "inf_*", route, m.device), True)
    assert tuple(cos.shape) == (G["B"], 1) and tuple(ones.shape) == (G["slice_end"], 1) and bool((ones == 1).all())
    check_tensor(what, "infer cos", cos.cpu().numpy(), G["inf64"], G["inf32"])
