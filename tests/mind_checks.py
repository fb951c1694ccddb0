"""What tests/test_mind.py and test_mind_gpu.py share: the golden evaluated once by tests/mind_ref.py, the project's tolerance
and the comparisons of a layer (paddlerec_amd/mind.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/mtl_checks.py), for EVERY tensor: err = max|got - ref64| / max|ref64|; the bound is 8 x
the same error of mind_ref.py evaluated in float32 on the same inputs, floor 1e-6.  Parameters after Adam go through
helpers.assert_adam_weights_close; the two frozen tensors must come back bit for bit."""
import functools
import os

import numpy as np
import torch

import mind_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close

FIXTURE = "mind_rand.npz"
FWD = (("loss", "loss"), ("user_cap", "caps2"), ("W", "W"))      # (name in the golden, name in mind_ref's forward record)


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def ref_step(G, p, state, s):
    """mind_ref's train step of recorded batch s from (p, state) in float64 and in float32 -> (r64, r32), each
    {loss, user_cap, W, g, n}."""
    g, out = G["g"], []
    for dt in (np.float64, np.float32):
        c, gr, new, _ = R.train_step(p, g["hist_%d" % s], g["seq_len_%d" % s], g["label_%d" % s], g["neg_%d" % s], g["log_q"],
                                     G["lr"], state, G["pow_p"], G["iters"], dtype=dt)
        out.append(dict(loss=np.asarray(c["loss"]).reshape(1), user_cap=c["caps2"], W=c["W"], g=gr, n=new))
    return out


@functools.lru_cache(maxsize=None)
def gold(name=FIXTURE):
    """The golden and mind_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE (the parameters
    the step before left and Adam's moments of the recorded gradients; mtl_checks.gold says why).  Computed once per
    session, never written afterwards."""
    g, p, lr, steps = R.load_golden(os.path.join(GOLDEN, name))
    G = dict(name=name, g=g, p=p, lr=lr, steps=steps, pow_p=float(g["pow_p"][0]), iters=int(g["iters"][0]))
    r64, r32, cur, st = [], [], p, None
    for s in range(steps):
        a, b = ref_step(G, cur, st, s)
        r64.append(a)
        r32.append(b)
        rec = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        _, st = R.adam_step(cur, rec, lr, st)
        cur = {k: g["n_%d_%s" % (s, k)] for k in p}
    G.update(r64=r64, r32=r32)
    return G


def check_step(r64, r32, p, lr, s, fwd, grads, params, what):
    """One step's loss, capsules, coupling weights, gradients and post-step parameters against the float64 reference."""
    for k, _ in FWD:
        e, b = R.relerr(np.asarray(fwd[k]).reshape(r64[k].shape), r64[k]), bound_of(r32[k], r64[k])
        print("%-14s step %d %-44s err %.3g  float32-ref err %.3g" % (what, s, k, e, b / 8))
        assert e <= b, (what, s, k, e, b)
    assert sorted(grads) == sorted(r64["g"]), (what, sorted(set(grads) ^ set(r64["g"])))
    for k in r64["g"]:
        e, b = R.relerr(grads[k], r64["g"][k]), bound_of(r32["g"][k], r64["g"][k])
        print("%-14s step %d %-44s err %.3g  float32-ref err %.3g" % (what, s, "g_" + k, e, b / 8))
        assert e <= b, (what, s, k, e, b)
    for k in p:
        if k in R.FROZEN:
            assert np.array_equal(np.asarray(params[k]), np.asarray(p[k])), (what, s, k)          # never stepped
        else:
            assert_adam_weights_close(np.asarray(params[k]), r64["n"][k], lr, 1, err_msg="%s step %d %s" % (what, s, k))


def check_golden(G):
    """Every array the golden records against the float64 reference; the float32 restatement's parameters too (the
    property the fixture's seed was searched for)."""
    g = G["g"]
    for s in range(G["steps"]):
        grads = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        check_step(G["r64"][s], G["r32"][s], G["p"], G["lr"], s, {k: g["%s_%d" % (k, s)] for k, _ in FWD}, grads,
                   {k: g["n_%d_%s" % (s, k)] for k in G["p"]}, "golden")
        for k in G["p"]:
            assert_adam_weights_close(G["r32"][s]["n"][k], g["n_%d_%s" % (s, k)], G["lr"], 1, err_msg="float32 " + k)


def layer_of(G, device="cpu", kernels=None):
    """The mirror the golden's state_dict belongs to (its parameters are random until set_dict)."""
    from paddlerec_amd.mind import MindLayer
    p, g = G["p"], G["g"]
    N, E = p["item_emb.weight"].shape
    _, K, T = p["capsual_layer.routing_logits"].shape
    H = p["capsual_layer.bilinear_mapping_matrix"].shape[1]
    return MindLayer(N, E, H, len(g["neg_0"]), T, G["pow_p"], G["iters"], K, device=device, kernels=kernels)


def layer_state(m):
    """(state_dict, Adam state) of a layer as mind_ref takes them."""
    p = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    ex = m.extra_optimizer_state()
    st = dict(t=m.step_count, m={k[6:]: v for k, v in ex.items() if k.startswith("mtl.m.")},
              v={k[6:]: v for k, v in ex.items() if k.startswith("mtl.v.")})
    return p, (st if m.step_count else None)


def feeds(G, s, device):
    g = G["g"]
    return tuple(torch.as_tensor(g["%s_%d" % (n, s)]).to(device) for n in ("hist", "seq_len", "label", "neg"))


def check_layer(G, m, what, steps=None):
    """The recorded batches through the layer as consecutive steps, each against mind_ref evaluated from the state the
    layer had before it (its float32 parameters and moments); the first step starts from the recording's own state, so the
    recording holds for the layer there as well."""
    m.set_dict(G["p"])
    g = G["g"]
    assert np.array_equal(m.log_q_host.numpy().view(np.uint32), g["log_q"].view(np.uint32))
    for s in range(G["steps"] if steps is None else steps):
        p, st = layer_state(m)
        r64, r32 = ref_step(G, p, st, s)
        hist, seq, label, neg = feeds(G, s, m.device)
        loss, user_cap, W = m.train_step(hist, seq, label, G["lr"], neg=neg)
        grads = {k: v.cpu().numpy() for k, v in m.last_gradients().items()}
        fwd = dict(loss=loss.value().cpu().numpy(), user_cap=user_cap.cpu().numpy(), W=W.cpu().numpy())
        check_step(r64, r32, p, G["lr"], s, fwd, grads, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, what)
        assert int(m.status.item()) == 0
        if s == 0:
            for k, _ in FWD:
                e = R.relerr(fwd[k].reshape(g["%s_0" % k].shape), g["%s_0" % k])
                assert e <= bound_of(G["r32"][0][k], G["r64"][0][k]), (what, k, e)


def mind_config(tmp_path, epochs=2, **hyper):
    """A flat trainer config over tests/golden/mind_sample.txt (train) and mind_valid_sample.txt (test): the shipped YAML's
    keys, the table cut to just above the samples' largest id and the sizes cut to the samples'."""
    train, test = tmp_path / "train", tmp_path / "valid"
    top = 0
    for d, name in ((train, "mind_sample.txt"), (test, "mind_valid_sample.txt")):
        d.mkdir(exist_ok=True)
        with open(os.path.join(GOLDEN, name)) as f:
            text = f.read()
        (d / name).write_text(text)
        top = max([top] + [int(x) for x in __import__("re").findall(r"(?:,|_item:)(\d+)", text)])
    cfg = {"runner.train_data_dir": str(train), "runner.test_data_dir": str(test), "runner.train_batch_size": 4,
           "runner.infer_batch_size": 4, "runner.epochs": epochs, "runner.print_interval": 2, "runner.batches_per_epoch": 3,
           "runner.model_save_path": str(tmp_path / "out"), "runner.infer_load_path": str(tmp_path / "out"),
           "runner.infer_start_epoch": 0, "runner.infer_end_epoch": epochs, "runner.use_gpu": False, "runner.use_auc": False,
           "hyper_parameters.item_count": top + 1, "hyper_parameters.embedding_dim": 8, "hyper_parameters.hidden_size": 8,
           "hyper_parameters.neg_samples": 16, "hyper_parameters.maxlen": 6, "hyper_parameters.pow_p": 1.0,
           "hyper_parameters.optimizer.learning_rate": 0.005}
    cfg.update({"hyper_parameters." + k: v for k, v in hyper.items()})
    return cfg
