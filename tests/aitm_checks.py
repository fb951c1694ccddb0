"""What tests/test_aitm.py and test_aitm_gpu.py share: the golden evaluated once by tests/aitm_ref.py, the project's tolerance
and the comparisons of a layer (paddlerec_amd/aitm.py) against them — TEST INFRASTRUCTURE ONLY.

Tolerance, the project's rule (tests/mtl_checks.py), for EVERY tensor: err = max|got - ref64| / max|ref64|; the bound is 8 x
the same error of aitm_ref.py evaluated in float32 on the same inputs, floor 1e-6.  Parameters after Adam go through
helpers.assert_adam_weights_close.  Gradients are the ones the optimizer applies: WITH the L2 term g + 1e-6 w."""
import functools
import os

import numpy as np
import torch

import aitm_ref as R
from conftest import GOLDEN
from helpers import assert_adam_weights_close

FIXTURE = "aitm_rand.npz"


def bound_of(ref32, ref64):
    return max(8 * R.relerr(ref32, ref64), 1e-6)


def ref_step(p, state, ids, click, buy, lr, masks=None):
    """aitm_ref's train step from (p, state) in float64 and in float32 -> (r64, r32), each {pred, loss, g, n}."""
    out = []
    for dt in (np.float64, np.float32):
        c, gr, new, _ = R.train_step(p, ids, click, buy, lr, state, masks, dtype=dt)
        out.append(dict(pred=c["pred"], loss=np.asarray(c["loss"]).reshape(1), g=gr, n=new))
    return out


@functools.lru_cache(maxsize=None)
def gold(name=FIXTURE):
    """The golden and aitm_ref's float64 / float32 evaluation of each recorded step FROM THE RECORDED STATE (the parameters
    the step before left and Adam's moments of the recorded gradients; mtl_checks.gold says why).  Computed once per
    session, never written afterwards."""
    g, p, lr, steps = R.load_golden(os.path.join(GOLDEN, name))
    r64, r32, cur, st = [], [], p, None
    for s in range(steps):
        a, b = ref_step(cur, st, g["ids_%d" % s], g["click_%d" % s], g["buy_%d" % s], lr)
        r64.append(a)
        r32.append(b)
        rec = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        _, st = R.adam_step(cur, rec, lr, st)
        cur = {k: g["n_%d_%s" % (s, k)] for k in p}
    return dict(name=name, g=g, p=p, lr=lr, steps=steps, r64=r64, r32=r32)


def check_step(r64, r32, p, lr, s, pred, loss, grads, params, what):
    """One step's predictions, loss, gradients and post-step parameters against the float64 reference of that step."""
    for k, got in (("pred", pred), ("loss", loss)):
        e, b = R.relerr(got, r64[k]), bound_of(r32[k], r64[k])
        print("%-14s step %d %-36s err %.3g  float32-ref err %.3g" % (what, s, k, e, b / 8))
        assert e <= b, (what, s, k, e, b)
    assert sorted(grads) == sorted(r64["g"]), (what, sorted(set(grads) ^ set(r64["g"])))
    for k in r64["g"]:
        e, b = R.relerr(grads[k], r64["g"][k]), bound_of(r32["g"][k], r64["g"][k])
        print("%-14s step %d %-36s err %.3g  float32-ref err %.3g" % (what, s, "g_" + k, e, b / 8))
        assert e <= b, (what, s, k, e, b)
    for k in p:
        assert_adam_weights_close(np.asarray(params[k]), r64["n"][k], lr, 1, err_msg="%s step %d %s" % (what, s, k))


def check_golden(G):
    """Every array the golden records against the float64 reference; the float32 restatement's parameters too (the
    property the fixture's seed was searched for)."""
    g = G["g"]
    for s in range(G["steps"]):
        grads = {k[len("g_%d_" % s):]: g[k] for k in g if k.startswith("g_%d_" % s)}
        check_step(G["r64"][s], G["r32"][s], G["p"], G["lr"], s, g["pred_%d" % s], g["loss_%d" % s], grads,
                   {k: g["n_%d_%s" % (s, k)] for k in G["p"]}, "golden")
        for k in G["p"]:
            assert_adam_weights_close(G["r32"][s]["n"][k], g["n_%d_%s" % (s, k)], G["lr"], 1, err_msg="float32 " + k)


def vocab_of(G):
    p = G["p"]
    return [[str(n), p["embedding_dict.%d.weight" % i].shape[0]] for i, n in enumerate(G["g"]["names"])]


def layer_of(G, device="cpu", kernels=None, drop_prob=(0.0, 0.0, 0.0)):
    """The mirror the golden's state_dict belongs to (its parameters are random until set_dict)."""
    from paddlerec_amd.aitm import AITMLayer
    p = G["p"]
    dims = [p["click_tower.layer.%d.weight" % j].shape[1] for j in (0, 3, 6)]
    m = AITMLayer(vocab_of(G), p["embedding_dict.0.weight"].shape[1], dims, drop_prob, device=device, kernels=kernels)
    m.keep_table_for_gradients = True
    return m


def layer_state(m):
    """(state_dict, Adam state) of a layer as aitm_ref takes them."""
    p = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    ex = m.extra_optimizer_state()
    st = dict(t=m.step_count, m={k[6:]: v for k, v in ex.items() if k.startswith("mtl.m.")},
              v={k[6:]: v for k, v in ex.items() if k.startswith("mtl.v.")})
    return p, (st if m.step_count else None)


def feeds(G, s, device):
    g = G["g"]
    return tuple(torch.as_tensor(g["%s_%d" % (n, s)]).to(device) for n in ("ids", "click", "buy"))


def masks_of(m, step, B, dropout):
    """The Dropout factors of training step `step` of layer m, per site of aitm_ref: rebuilt from m.dropout_streams with
    `dropout` (ops.dropout or the stand-in's) on ones.  The layer's "l0" site is one pass over both towers' first layers."""
    h0, h1, d = m.dims
    shape = dict(l0=(B, 2 * h0), click1=(B, h1), conv1=(B, h1), click2=(B, d), conv2=(B, d), info=(B, d))
    out = {}
    for site, (stream, rate) in m.dropout_streams(step).items():
        f = dropout(torch.ones(shape[site], dtype=torch.float32, device=m.device), rate, m.dropout_seed, stream).cpu().numpy()
        if site == "l0":
            out["click0"], out["conv0"] = f[:, :h0], f[:, h0:]
        else:
            out[site] = f
    return out


def check_layer(G, m, what, steps=None, recorded=True, dropout=None):
    """The recorded batches through the layer as consecutive steps, each against aitm_ref evaluated from the state the
    layer had before it (its float32 parameters and moments).  dropout: the op that rebuilds the step's masks when the
    layer has Dropout (then the first step is not held against the recording, which has none).  With Dropout the
    parameters after the step are held against Adam restated in float64 on the LAYER'S OWN gradients, which the lines before
    have just held against the reference: the fixture's seed was searched so that no element of a recorded step sits where
    float32 noise in a near-zero gradient decides the sign of Adam's first steps (tools/make_golden_aitm.py), and a step
    under other masks has no such guarantee — a unit that only saturated samples keep alive gives a whole row of such
    elements."""
    m.set_dict(G["p"])
    g = G["g"]
    for s in range(G["steps"] if steps is None else steps):
        p, st = layer_state(m)
        ids, click, buy = g["ids_%d" % s], g["click_%d" % s], g["buy_%d" % s]
        masks = masks_of(m, m.step_count + 1, len(ids), dropout) if dropout is not None else None
        r64, r32 = ref_step(p, st, ids, click, buy, G["lr"], masks)
        loss, pred = m.train_step(*feeds(G, s, m.device), G["lr"])
        grads = {k: v.cpu().numpy() for k, v in m.last_gradients().items()}
        if dropout is not None:
            r64 = dict(r64, n=R.adam_step(p, grads, G["lr"], st)[0])
        check_step(r64, r32, G["p"], G["lr"], s, pred.cpu().numpy(), loss.value().cpu().numpy(), grads,
                   {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, what)
        assert int(m.status.item()) == 0
        if s == 0 and recorded and dropout is None:      # the first step starts from the recording's own state
            e = R.relerr(pred.cpu().numpy(), g["pred_0"])
            assert e <= bound_of(G["r32"][0]["pred"], G["r64"][0]["pred"]), (what, e)


def aitm_config(tmp_path, epochs=2, **hyper):
    """A flat trainer config over tests/golden/aitm_sample.txt (train and test): the shipped YAML's values, but the big
    tables cut to just above the sample's largest id per field (the full tables are 1.35 M rows, three times with Adam's
    moments, rewritten by every CPU step and every checkpoint)."""
    names = "101 121 122 124 125 126 127 128 129 205 206 207 216 508 509 702 853 301".split()
    sizes = [238635, 98, 14, 3, 8, 4, 4, 3, 5, 467298, 6929, 263942, 106399, 5888, 104830, 51878, 37148, 4]
    ids = np.loadtxt(os.path.join(GOLDEN, "aitm_sample.txt"), delimiter=",", skiprows=1, dtype=np.int64)[:, 2:]
    small = [min(n, int(ids[:, i].max()) + 1) for i, n in enumerate(sizes)]
    for sub in ("train", "test"):
        d = tmp_path / sub
        d.mkdir(exist_ok=True)
        with open(os.path.join(GOLDEN, "aitm_sample.txt")) as f:
            (d / "sample.csv").write_text(f.read())
        (d / "unread_second_file.csv").write_text("not,a,data,line\n")        # only file_list[0] is read
    cfg = {"runner.train_data_dir": str(tmp_path / "train"), "runner.test_data_dir": str(tmp_path / "test"),
           "runner.train_batch_size": 4, "runner.infer_batch_size": 4, "runner.epochs": epochs, "runner.print_interval": 2,
           "runner.model_save_path": str(tmp_path / "out"), "runner.infer_load_path": str(tmp_path / "out"),
           "runner.infer_start_epoch": 0, "runner.infer_end_epoch": epochs, "runner.use_gpu": False,
           "hyper_parameters.feature_vocabulary": [[n, s] for n, s in zip(names, small)], "hyper_parameters.embedding_size": 5,
           "hyper_parameters.dims": [128, 64, 32], "hyper_parameters.drop_prob": [0.1, 0.3, 0.3],
           "hyper_parameters.optimizer.learning_rate": 0.0001}
    cfg.update({"hyper_parameters." + k: v for k, v in hyper.items()})
    return cfg
