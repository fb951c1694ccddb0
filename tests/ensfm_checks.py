"""What tests/test_ensfm.py and test_ensfm_gpu.py share: the golden evaluated once by tests/ensfm_ref.py, the project's
tolerance and the comparison of a layer (paddlerec_amd/ensfm.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/tisas_checks.py), for EVERY tensor, the Adagrad accumulators included (they are
quadratic in the gradients): err = max|got - ref64| / max|ref64|; the bound is 8 x the same error of ensfm_ref.py evaluated
in float32 on the same inputs, floor 1e-6.  Parameters after Adagrad get the two-part statement of
helpers.assert_adam_weights_close, adapted: at least 0.98 of the elements within 1e-5 of the tensor's scale, and none
further away than Adagrad can move it — |lr g / (sqrt(acc) + eps)| < lr per step, so steps * lr."""
import functools
import os

import numpy as np
import torch

import ensfm_ref as R
from conftest import GOLDEN


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def assert_adagrad_weights_close(got, want, lr, steps, rel=1e-5, frac=0.98, err_msg=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64).reshape(np.shape(got))
    err = np.abs(got - want)
    scale = max(float(np.abs(want).max()), 1e-30)
    tight = float(np.mean(err <= rel * scale))
    assert tight >= frac, "%s only %.4f of the elements within %.0e of the scale %.3e (max err %.3e)" % (
        err_msg, tight, rel, scale, float(err.max()))
    assert float(err.max()) <= steps * lr, "%s max err %.3e exceeds what %d Adagrad steps of lr %.3g can move" % (
        err_msg, float(err.max()), steps, lr)


def ref_step(G, p, acc, s):
    """ensfm_ref's train step of recorded batch s from (p, acc) in float64 and float32 -> (r64, r32), each a dict of the
    forward tensors, g, n (new parameters) and a (new accumulators)."""
    g, out = G["g"], []
    for dt in (np.float64, np.float32):
        c, gr, new, nacc = R.train_step(p, g["u_%d" % s], g["attr"], g["ur_%d" % s], G["w"], G["lr"], acc, dt)
        out.append(dict({k: c[k] for k in R.FWD}, g=gr, n=new, a=nacc))
    return out


@functools.lru_cache(maxsize=None)
def gold(name="ensfm_rand.npz"):
    """The golden and ensfm_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE.  Computed once per
    session, never written afterwards."""
    g, p, lr, w, steps = R.load_golden(os.path.join(GOLDEN, name))
    G = dict(g=g, p=p, lr=lr, w=w, steps=steps)
    r64, r32, cur, acc = [], [], p, None
    for s in range(steps):
        a, b = ref_step(G, cur, acc, s)
        r64.append(a)
        r32.append(b)
        cur = {k: g["n_%d_%s" % (s, k)] for k in p}
        acc = {k: g["a_%d_%s" % (s, k)] for k in p}
    G.update(r64=r64, r32=r32, final=cur)
    for dt, key in ((np.float64, "inf64"), (np.float32, "inf32")):
        G[key] = R.forward(cur, g["inf_u"], g["attr"], None, dt)["pre"]
    return G


def check_tensor(what, name, got, r64, r32):
    e, b = R.relerr(np.asarray(got).reshape(np.shape(r64)), r64), bound_of(r32, r64)
    print("%-10s %-44s err %.3g  float32-ref err %.3g" % (what, name, e, b / 8))
    assert e <= b, (what, name, e, b)


def check_step(r64, r32, lr, s, fwd, grads, params, accs, what):
    """One step's forward tensors, gradients, accumulators and post-step parameters against the float64 reference."""
    for k in R.FWD:
        check_tensor(what, "step %d %s" % (s, k), fwd[k], r64[k], r32[k])
    assert sorted(grads) == sorted(R.PARAMS), (what, sorted(grads))
    for k in R.PARAMS:
        check_tensor(what, "step %d g_%s" % (s, k), grads[k], r64["g"][k], r32["g"][k])
        check_tensor(what, "step %d acc_%s" % (s, k), accs[k], r64["a"][k], r32["a"][k])
        assert_adagrad_weights_close(np.asarray(params[k]), r64["n"][k], lr, 1, err_msg="%s step %d %s" % (what, s, k))


def check_golden(G):
    """Every array the golden records, both steps and the infer call, against the float64 reference."""
    g = G["g"]
    for s in range(G["steps"]):
        pick = lambda pre: {k: g["%s_%d_%s" % (pre, s, k)] for k in R.PARAMS}
        check_step(G["r64"][s], G["r32"][s], G["lr"], s, {k: g["%s_%d" % (k, s)] for k in R.FWD}, pick("g"), pick("n"), pick("a"),
                   "golden")
    check_tensor("golden", "infer pre", g["inf_pre"], G["inf64"], G["inf32"])


def layer_of(G, device="cuda"):
    from paddlerec_amd.ensfm import ENSFMLayer
    p = G["p"]
    m = ENSFMLayer(p["user_feature_emb.weight"].shape[0], p["item_bias.weight"].shape[0], p["H_i"].shape[0], device=device)
    assert sorted(m.state_dict()) == sorted(R.PARAMS)
    return m


def layer_state(m):
    p = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    acc = {k[len("ensfm.acc."):]: v.reshape(p[k[len("ensfm.acc."):]].shape) for k, v in m.extra_optimizer_state().items()}
    return p, acc


def check_layer(G, m, what):
    """The recorded batches through the layer as consecutive steps, each against ensfm_ref evaluated from the state the layer
    had before it; the first step is also held to the recording itself."""
    g, dev = G["g"], m.device
    m.set_dict(G["p"])
    attr = torch.as_tensor(g["attr"]).to(dev)
    for s in range(G["steps"]):
        p, acc = layer_state(m)
        r64, r32 = ref_step(G, p, acc, s)
        u, ur = torch.as_tensor(g["u_%d" % s]).to(dev), torch.as_tensor(g["ur_%d" % s]).to(dev)
        pre, pos_r, q_emb, p_emb, _ = m.forward(u, attr, ur, g["attr"].shape[0] - 1)
        loss = m.train_step(u, attr, ur, g["attr"].shape[0] - 1, lr=G["lr"], negative_weight=G["w"])
        fwd = {k: v.cpu().numpy() for k, v in dict(loss=loss, pre=pre, pos_r=pos_r, q_emb=q_emb, p_emb=p_emb).items()}
        grads = {k: v.cpu().numpy() for k, v in m.last_gradients().items()}
        newp, newa = layer_state(m)
        check_step(r64, r32, G["lr"], s, fwd, grads, newp, newa, what)
        assert int(m.status.item()) == 0 and int(m._group_status.item()) == 0
        if s == 0:
            for k in R.FWD:
                e = R.relerr(fwd[k].reshape(g["%s_0" % k].shape), g["%s_0" % k])
                assert e <= bound_of(G["r32"][0][k], G["r64"][0][k]), (what, k, e)


def check_infer(G, m, what):
    g = G["g"]
    m.set_dict(G["final"])
    (pre,) = m.forward(torch.as_tensor(g["inf_u"]).to(m.device), torch.as_tensor(g["attr"]).to(m.device))
    check_tensor(what, "infer pre", pre.cpu().numpy(), G["inf64"], G["inf32"])
    check_tensor(what, "infer pre (golden)", g["inf_pre"], G["inf64"], G["inf32"])
