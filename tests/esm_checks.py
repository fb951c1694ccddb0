"""What tests/test_esmm.py, test_escm2.py and test_esm_gpu.py share: the goldens evaluated once by tests/esm_ref.py, the
project's tolerance and the comparisons of a layer (paddlerec_amd/esmm.py, escm2.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/mtl_checks.py), for EVERY tensor: err = max|got - ref64| / max|ref64|; the bound is 8 x
the same error of esm_ref.py evaluated in float32 on the same inputs, floor 1e-6.  Parameters after Adam go through
helpers.assert_adam_weights_close.  "outs" is net.py's out_list side by side (esm_ref.outs_of)."""
import functools
import os

import numpy as np
import torch

import esm_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close

FIXTURES = {"esmm": ("esmm_rand.npz",), "escm2": ("escm2_ipw_rand.npz", "escm2_dr_rand.npz")}


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def ref_step(p, state, ids, click, buy, lr, cfg):
    """esm_ref's train step from (p, state) in float64 and in float32 -> (r64, r32), each {outs, loss, g, n}."""
    out = []
    for dt in (np.float64, np.float32):
        c, gr, new, _ = R.train_step(p, ids, click, buy, lr, cfg, state, dtype=dt)
        out.append(dict(outs=R.outs_of(c["pred"]), loss=np.asarray(c["loss"]).reshape(1), g=gr, n=new))
    return out


@functools.lru_cache(maxsize=None)
def gold(name):
    """The golden `name` and esm_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE (the
    parameters the step before left and Adam's moments of the recorded gradients; mtl_checks.gold says why).  Computed
    once per session, never written afterwards."""
    g, p, lr, steps, cfg = R.load_golden(os.path.join(GOLDEN, name))
    r64, r32, cur, st = [], [], p, None
    for s in range(steps):
        a, b = ref_step(cur, st, g["ids_%d" % s], g["click_%d" % s], g["buy_%d" % s], lr, cfg)
        r64.append(a)
        r32.append(b)
        rec = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        _, st = R.adam_step(cur, rec, lr, st)
        cur = {k: g["n_%d_%s" % (s, k)] for k in p}
    return dict(name=name, g=g, p=p, lr=lr, steps=steps, cfg=cfg, r64=r64, r32=r32)


def check_step(r64, r32, p, lr, s, outs, loss, grads, params, what):
    """One step's outputs, loss, gradients and post-step parameters against the float64 reference of that step."""
    for k, got in (("outs", outs), ("loss", loss)):
        e, b = R.relerr(got, r64[k]), bound_of(r32[k], r64[k])
        print("%-14s step %d %-28s err %.3g  float32-ref err %.3g" % (what, s, k, e, b / 8))
        assert e <= b, (what, s, k, e, b)
    assert sorted(grads) == sorted(r64["g"]), (what, sorted(set(grads) ^ set(r64["g"])))
    for k in r64["g"]:
        e, b = R.relerr(grads[k], r64["g"][k]), bound_of(r32["g"][k], r64["g"][k])
        print("%-14s step %d %-28s err %.3g  float32-ref err %.3g" % (what, s, "g_" + k, e, b / 8))
        assert e <= b, (what, s, k, e, b)
    for k in p:
        assert_adam_weights_close(np.asarray(params[k]), r64["n"][k], lr, 1, err_msg="%s step %d %s" % (what, s, k))


def check_golden(G):
    """Every array the golden records against the float64 reference; the float32 restatement's parameters too (the
    property the fixtures' seed was searched for)."""
    g = G["g"]
    for s in range(G["steps"]):
        grads = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        check_step(G["r64"][s], G["r32"][s], G["p"], G["lr"], s, g["outs_%d" % s], g["loss_%d" % s], grads,
                   {k: g["n_%d_%s" % (s, k)] for k in G["p"]}, "golden")
        for k in G["p"]:
            assert_adam_weights_close(G["r32"][s]["n"][k], g["n_%d_%s" % (s, k)], G["lr"], 1, err_msg="float32 " + k)


def layer_of(G, device="cpu", kernels=None):
    """The mirror a golden's state_dict belongs to (its parameters are random until set_dict)."""
    p, cfg = G["p"], G["cfg"]
    N, D = p["embedding.weight"].shape
    _, F, L = G["g"]["ids_0"].shape
    if R.is_escm2(p):
        from paddlerec_amd.escm2 import ESCMLayer
        E = sum(1 for k in p if k.startswith("expert_") and k.endswith(".weight"))
        return ESCMLayer(N, D, F, None, None, E, p["expert_0.weight"].shape[1], p["tower_0.weight"].shape[1], cfg["mode"],
                         p["expert_0.weight"].shape[0], max_len=L, global_w=cfg["global_w"],
                         counterfactual_w=cfg["counterfactual_w"], device=device, kernels=kernels)
    from paddlerec_amd.esmm import ESMMLayer
    ctr, cvr = R.esmm_towers(p)
    widths = lambda idx: [p["linear_%d.weight" % i].shape[1] for i in idx[:-1]]
    return ESMMLayer(N, D, F, widths(ctr), widths(cvr), max_len=L, device=device, kernels=kernels)


def layer_state(m):
    """(state_dict, Adam state) of a layer as esm_ref takes them."""
    p = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    ex = m.extra_optimizer_state()
    st = dict(t=m.step_count, m={k[6:]: v for k, v in ex.items() if k.startswith("mtl.m.")},
              v={k[6:]: v for k, v in ex.items() if k.startswith("mtl.v.")})
    return p, (st if m.step_count else None)


def feeds(G, s, device):
    g = G["g"]
    return tuple(torch.as_tensor(g["%s_%d" % (n, s)]).to(device) for n in ("ids", "click", "buy"))


def check_layer(G, m, what, steps=None, recorded=True):
    """The recorded batches through the layer as consecutive steps, each against esm_ref evaluated from the state the
    layer had before it (its float32 parameters and moments).  recorded=False: G["p"] is not the recording's state_dict
    (another net over the recording's batches), so the first step is not held against the recorded outputs."""
    m.set_dict(G["p"])
    for s in range(G["steps"] if steps is None else steps):
        p, st = layer_state(m)
        g = G["g"]
        r64, r32 = ref_step(p, st, g["ids_%d" % s], g["click_%d" % s], g["buy_%d" % s], G["lr"], G["cfg"])
        loss, pred = m.train_step(*feeds(G, s, m.device), G["lr"])
        outs = R.outs_of(pred.cpu().numpy())
        grads = {k: v.cpu().numpy() for k, v in m.last_gradients().items()}
        check_step(r64, r32, G["p"], G["lr"], s, outs, loss.value().cpu().numpy(), grads,
                   {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, what)
        assert not m.state_dict()["embedding.weight"][0].any()          # the padding row never moves
        assert int(m.status.item()) == 0
        if s == 0 and recorded:      # the first step starts from the recording's own state: the recording holds for the layer as well
            e = R.relerr(outs, g["outs_0"])
            assert e <= bound_of(G["r32"][0]["outs"], G["r64"][0]["outs"]), (what, e)


def aliccp_config(tmp_path, model, epochs=2, mode="DR", **hyper):
    """A flat trainer config over tests/golden/aliccp_sample.txt (train and test): the shipped YAML's values, but a table
    of 1000 rows instead of 737946 (the sample's ids stop at 916; the full table is 35 MB, three times with Adam's moments,
    rewritten by every CPU step and every checkpoint)."""
    data = tmp_path / "data"
    data.mkdir(exist_ok=True)
    with open(os.path.join(GOLDEN, "aliccp_sample.txt")) as f:
        (data / "small.txt").write_text(f.read())
    cfg = {"runner.train_data_dir": str(data), "runner.test_data_dir": str(data), "runner.train_batch_size": 2,
           "runner.infer_batch_size": 2, "runner.epochs": epochs, "runner.print_interval": 2, "runner.use_auc": True,
           "runner.model_save_path": str(tmp_path / "out"), "runner.infer_load_path": str(tmp_path / "out"),
           "runner.infer_start_epoch": 0, "runner.infer_end_epoch": epochs, "runner.use_gpu": False,
           "hyper_parameters.sparse_feature_number": 1000, "hyper_parameters.sparse_feature_dim": 12,
           "hyper_parameters.num_field": 23, "hyper_parameters.ctr_fc_sizes": [256, 64], "hyper_parameters.cvr_fc_sizes": [256, 64],
           "hyper_parameters.optimizer.learning_rate": 0.001}
    if model == "escm2":
        cfg.update({"runner.counterfact_mode": mode, "hyper_parameters.global_w": 1.0, "hyper_parameters.counterfactual_w": 0.01,
                    "hyper_parameters.feature_size": 276, "hyper_parameters.expert_num": 8, "hyper_parameters.gate_num": 3,
                    "hyper_parameters.expert_size": 16, "hyper_parameters.tower_size": 8})
    cfg.update({"hyper_parameters." + k: v for k, v in hyper.items()})
    return cfg
