"""What tests/test_ncf.py and test_ncf_gpu.py share: the goldens evaluated once by tests/ncf_ref.py, the project's tolerance
and the comparison of a layer (paddlerec_amd/ncf.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/tisas_checks.py, tests/ensfm_checks.py): for every tensor err = max|got - ref64| /
max|ref64|; the bound is 8 x the same error of ncf_ref.py evaluated in float32 on the same inputs, floor 1e-6.  Parameters
and moments after Adam: helpers.assert_adam_weights_close and the 1e-5-of-scale bar of helpers.assert_moments_close."""
import functools
import os

import numpy as np
import torch

import ncf_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close, assert_close_scaled

GOLDENS = ("ncf_neumf.npz", "ncf_gmf.npz", "ncf_mlp.npz")


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def check_tensor(what, name, got, r64, r32):
    e, b = R.relerr(np.asarray(got).reshape(np.shape(r64)), r64), bound_of(r32, r64)
    print("%-12s %-46s err %.3g  float32-ref err %.3g" % (what, name, e, b / 8))
    assert e <= b, (what, name, e, b)


def ref_step(G, p, m, v, s, step):
    """ncf_ref's train step of recorded batch s from (p, m, v) in float64 and float32."""
    g = G["g"]
    return [R.train_step(p, m, v, g["users_%d" % s], g["items_%d" % s], g["labels_%d" % s], step, G["lr"], dt)
            for dt in (np.float64, np.float32)]


@functools.lru_cache(maxsize=None)
def gold(name):
    """A golden and ncf_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE.  Computed once per
    session, never written afterwards."""
    g, p, lr, steps = R.load_golden(os.path.join(GOLDEN, name))
    G = dict(g=g, p=p, lr=lr, steps=steps, mode=str(g["mode"][0]), mf_dim=int(g["mf_dim"][0]), layers=g["layers"].tolist())
    r64, r32, cur, m, v = [], [], p, None, None
    for s in range(steps):
        a, b = ref_step(G, cur, m, v, s, s + 1)
        r64.append(a)
        r32.append(b)
        cur, m, v = ({k: g["%s_%d_%s" % (pre, s, k)] for k in p} for pre in ("n", "m", "v"))
    G.update(r64=r64, r32=r32, final=cur)
    for dt, key in ((np.float64, "inf64"), (np.float32, "inf32")):
        G[key] = R.forward(cur, g["inf_users"], g["inf_items"], dt)["pred"]
    return G


def check_step(r64, r32, lr, s, got, what):
    """One step's loss, pred, gradients, moments and post-step parameters (got: dict(loss, pred, g, n, m, v)) against the
    float64 reference."""
    for k in ("loss", "pred"):
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
    return dict(loss=g["loss_%d" % s], pred=g["pred_%d" % s], g=pick("g"), n=pick("n"), m=pick("m"), v=pick("v"))


def check_golden(G):
    """Every array the golden records, both steps and the infer call, against the float64 reference."""
    for s in range(G["steps"]):
        check_step(G["r64"][s], G["r32"][s], G["lr"], s, recorded_step(G, s), "golden")
    check_tensor("golden", "infer pred", G["g"]["inf_pred"], G["inf64"], G["inf32"])


def layer_of(G, device="cuda"):
    from paddlerec_amd.ncf import NCFLayer
    g = G["g"]
    m = NCFLayer(int(g["num_users"][0]), int(g["num_items"][0]), G["mf_dim"], G["layers"], G["mode"], device=device)
    assert sorted(m.state_dict()) == sorted(G["p"])
    return m


def layer_state(m):
    npy = lambda d: {k: v.detach().cpu().numpy().copy() for k, v in d.items()}
    mm, vv = m.moments()
    return npy(m.state_dict()), npy(mm), npy(vv)


def check_layer(G, m, what):
    """The recorded batches through the layer as consecutive steps, each against ncf_ref evaluated from the state the layer
    had before it; the first step is also held to the recording itself."""
    g, dev = G["g"], m.device
    m.set_dict(G["p"])
    t = lambda k: torch.as_tensor(g[k]).to(dev)
    for s in range(G["steps"]):
        p, mm, vv = layer_state(m)
        r64, r32 = ref_step(G, p, mm, vv, s, s + 1)
        loss = m.train_step(t("users_%d" % s), t("items_%d" % s), t("labels_%d" % s), lr=G["lr"])
        n, nm, nv = layer_state(m)
        got = dict(loss=loss.cpu().numpy(), pred=m._last["pred"].cpu().numpy(),
                   g={k: v.cpu().numpy() for k, v in m.last_gradients().items()}, n=n, m=nm, v=nv)
        check_step(r64, r32, G["lr"], s, got, what)
        assert int(m.status.item()) == 0 and int(m._group_status.item()) == 0
        if s == 0:
            rec = recorded_step(G, 0)
            for k in ("loss", "pred"):
                assert R.relerr(got[k].reshape(rec[k].shape), rec[k]) <= bound_of(G["r32"][0][k], G["r64"][0][k]), (what, k)


def check_infer(G, m, what):
    g = G["g"]
    m.set_dict(G["final"])
    pred = m.forward(torch.as_tensor(g["inf_users"]).to(m.device), torch.as_tensor(g["inf_items"]).to(m.device))
    assert tuple(pred.shape) == (len(g["inf_users"]), 1)
    check_tensor(what, "infer pred", pred.cpu().numpy(), G["inf64"], G["inf32"])
