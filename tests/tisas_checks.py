"""What tests/test_tisas.py and test_tisas_gpu.py share: the goldens evaluated once by tests/tisas_ref.py, the project's
tolerance and the comparisons of a layer (paddlerec_amd/tisas.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/mtl_checks.py), for EVERY tensor: err = max|got - ref64| / max|ref64|; the bound is 8 x
the same error of tisas_ref.py evaluated in float32 on the same inputs, floor 1e-6.  Parameters after Adam go through
helpers.assert_adam_weights_close.  The one exception is tisas_ref.structural_zero (K_w.bias of every block): its gradient
is zero in exact arithmetic, so it is held to a noise bound, 32 float32 epsilons (2^-24) times the sum of the magnitudes of
the terms that cancel (tisas_ref.backward's kbias_scale), and its parameter to what the Adam steps taken can move."""
import functools
import os

import numpy as np
import torch

import tisas_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close

FIXTURES = ("tisas_h1.npz", "tisas_h2.npz")
FWD = ("loss", "log_feats")
BATCH = ("seq", "tm", "pos", "neg")


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def ref_step(G, p, state, s, masks=None):
    """tisas_ref's train step of recorded batch s from (p, state) in float64 and in float32 -> (r64, r32), each
    {loss, log_feats, g, n, kbias}."""
    g, out = G["g"], []
    for dt in (np.float64, np.float32):
        c, gr, new, _ = R.train_step(p, *[g["%s_%d" % (n, s)] for n in BATCH], G["H"], G["lr"], state, masks, dt)
        out.append(dict(loss=c["loss"], log_feats=c["log_feats"], g=gr, n=new, kbias=c["kbias_scale"]))
    return out


@functools.lru_cache(maxsize=None)
def gold(name):
    """The golden and tisas_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE (the parameters
    the step before left and Adam's moments of the recorded gradients).  Computed once per session, never written
    afterwards."""
    g, p, lr, steps = R.load_golden(os.path.join(GOLDEN, name))
    G = dict(name=name, g=g, p=p, lr=lr, steps=steps, H=int(g["heads"][0]))
    r64, r32, cur, st = [], [], p, None
    for s in range(steps):
        a, b = ref_step(G, cur, st, s)
        r64.append(a)
        r32.append(b)
        rec = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        _, st = R.adam_step(cur, rec, lr, st)
        cur = {k: g["n_%d_%s" % (s, k)] for k in p}
    G.update(r64=r64, r32=r32, final=cur)
    return G


def check_tensor(what, name, got, r64, r32):
    e, b = R.relerr(np.asarray(got).reshape(np.shape(r64)), r64), bound_of(r32, r64)
    print("%-12s %-46s err %.3g  float32-ref err %.3g" % (what, name, e, b / 8))
    assert e <= b, (what, name, e, b)


def check_step(r64, r32, lr, s, fwd, grads, params, what, steps_taken=1):
    """One step's loss, log_feats, gradients and post-step parameters against the float64 reference."""
    for k in FWD:
        check_tensor(what, "step %d %s" % (s, k), fwd[k], r64[k], r32[k])
    assert sorted(grads) == sorted(r64["g"]), (what, sorted(set(grads) ^ set(r64["g"])))
    for k in r64["g"]:
        if R.structural_zero(k):
            noise = 32 * 2.0 ** -24 * r64["kbias"][k]
            print("%-12s step %d g_%-40s max %.3g  noise bound %.3g" % (what, s, k, np.abs(grads[k]).max(), noise))
            assert np.abs(grads[k]).max() <= noise, (what, s, k)
            cap = 2.0 * steps_taken * lr * 3.17              # helpers.assert_adam_weights_close's cap on one element
            assert np.abs(np.asarray(params[k], np.float64) - r64["n"][k]).max() <= cap, (what, s, k)
            continue
        check_tensor(what, "step %d g_%s" % (s, k), grads[k], r64["g"][k], r32["g"][k])
        assert_adam_weights_close(np.asarray(params[k]), r64["n"][k], lr, 1, err_msg="%s step %d %s" % (what, s, k))


def check_golden(G):
    """Every array the golden records against the float64 reference."""
    g = G["g"]
    for s in range(G["steps"]):
        grads = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        check_step(G["r64"][s], G["r32"][s], G["lr"], s, {k: g["%s_%d" % (k, s)] for k in FWD}, grads,
                   {k: g["n_%d_%s" % (s, k)] for k in G["p"]}, "golden")
    r64 = R.infer(G["final"], g["inf_seq"], g["inf_tm"], g["inf_items"], G["H"])
    r32 = R.infer(G["final"], g["inf_seq"], g["inf_tm"], g["inf_items"], G["H"], np.float32)
    check_tensor("golden", "infer logits", g["inf_logits"], r64, r32)


def layer_of(G, device="cpu", kernels=None, dropout_rate=0.0, **kw):
    """The mirror the golden's state_dict belongs to (its parameters are random until set_dict)."""
    from paddlerec_amd.tisas import TiSASRecLayer
    p = G["p"]
    N, D = p["item_emb.weight"].shape
    return TiSASRecLayer(5, N - 1, D, p["abs_pos_K_emb.weight"].shape[0], p["time_matrix_K_emb.weight"].shape[0] - 1,
                         R.num_blocks(p), G["H"], dropout_rate=dropout_rate, device=device, kernels=kernels, **kw)


def layer_state(m):
    """(state_dict, Adam state) of a layer as tisas_ref takes them."""
    p = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    ex = m.extra_optimizer_state()
    st = dict(t=m.step_count, m={k[6:]: v for k, v in ex.items() if k.startswith("mtl.m.")},
              v={k[6:]: v for k, v in ex.items() if k.startswith("mtl.v.")})
    return p, (st if m.step_count else None)


def feeds(G, s, device):
    return tuple(torch.as_tensor(G["g"]["%s_%d" % (n, s)]).to(device) for n in BATCH)


def check_layer(G, m, what, masks_of=None):
    """The recorded batches through the layer as consecutive steps, each against tisas_ref evaluated from the state the layer
    had before it (its float32 parameters and moments).  masks_of(m, step, B, L): the step's dropout masks for tisas_ref
    (None: the layer runs without dropout and the first step is also held to the recording itself)."""
    m.set_dict(G["p"])
    g = G["g"]
    for s in range(G["steps"]):
        p, st = layer_state(m)
        B, L = g["seq_%d" % s].shape
        masks = masks_of(m, s + 1, B, L) if masks_of is not None else None
        r64, r32 = ref_step(G, p, st, s, masks)
        loss, log_feats = m.train_step(*feeds(G, s, m.device), lr=G["lr"])
        grads = {k: v.cpu().numpy() for k, v in m.last_gradients().items()}
        fwd = dict(loss=loss.value().cpu().numpy(), log_feats=log_feats.cpu().numpy())
        check_step(r64, r32, G["lr"], s, fwd, grads, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, what)
        assert int(m.status.item()) == 0
        if s == 0 and masks is None:
            for k in FWD:
                e = R.relerr(fwd[k].reshape(g["%s_0" % k].shape), g["%s_0" % k])
                assert e <= bound_of(G["r32"][0][k], G["r64"][0][k]), (what, k, e)


def check_infer(G, m, what):
    g = G["g"]
    m.set_dict(G["final"])
    m.eval()
    logits = m.forward(*(torch.as_tensor(g[n]).to(m.device) for n in ("inf_seq", "inf_tm", "inf_items")))
    m.train()
    r64 = R.infer(G["final"], g["inf_seq"], g["inf_tm"], g["inf_items"], G["H"])
    r32 = R.infer(G["final"], g["inf_seq"], g["inf_tm"], g["inf_items"], G["H"], np.float32)
    check_tensor(what, "infer logits", logits.cpu().numpy(), r64, r32)
    check_tensor(what, "infer logits (golden)", g["inf_logits"], r64, r32)


def tisas_config(tmp_path, fixture="tisas_sample.txt", epochs=2, maxlen=8, time_span=16, hidden=8, heads=2, batch=2):
    """A flat trainer config over tests/golden/<fixture> for train and test."""
    from paddlerec_amd.reader import tisas_data_partition
    d = tmp_path / "data"
    d.mkdir(exist_ok=True)
    with open(os.path.join(GOLDEN, fixture)) as f:
        (d / fixture).write_text(f.read())
    part = tisas_data_partition(os.path.join(GOLDEN, fixture))
    return {"config_abs_dir": str(tmp_path), "runner.train_data_dir": str(d), "runner.test_data_dir": str(d),
            "runner.train_batch_size": batch, "runner.infer_batch_size": 1, "runner.epochs": epochs, "runner.print_interval": 1,
            "runner.model_save_path": str(tmp_path / "out"), "runner.infer_load_path": str(tmp_path / "out"),
            "runner.infer_start_epoch": epochs - 1, "runner.infer_end_epoch": epochs, "runner.seed": 7,
            "hyper_parameters.optimizer.learning_rate": 0.001, "hyper_parameters.num_users": part[3],
            "hyper_parameters.num_items": part[4], "hyper_parameters.num_blocks": 2, "hyper_parameters.num_heads": heads,
            "hyper_parameters.maxlen": maxlen, "hyper_parameters.hidden_units": hidden, "hyper_parameters.time_span": time_span}
