#!/usr/bin/env python3
"""Generate tests/golden/autofis_D5.npz by executing the reference's UNMODIFIED models/rank/autofis/net.py and
optimizer.py over the paddle shim (oracle/paddle_shim), the way tools/make_golden_flen.py pins rank/flen.  Runs only in
the build container (needs the reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_autofis.py     # rewrites tests/golden/autofis_D5.npz deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: nn.BatchNorm (the shim's BatchNorm1D),
nn.Identity, paddle.gather for a [P,1] index on axis 1 (net.py:93-96), paddle.abs, paddle.sign (optimizer.py:51-52),
F.binary_cross_entropy (dygraph_model.py:47), Tensor.set_value (optimizer.py:58) and, where absent, F.relu / F.sigmoid.
Stage 1 loads comb_mask.npy from the working directory (net.py:70), so the script runs in a temporary one.  N 40, S 6, D 5, width 8, depth 2, B 10; the ids hold duplicates and the id 0 (a live row:
neither table has a padding row); Linear and BatchNorm biases are non-zero and BatchNorm weights differ from 1.  Records:
  (a) `a_*`: a stage-0 train step: pred, loss, every gradient (the tables' dense) and the running statistics after it;
  (b) `grda_*`: three SimpleGrda.step()s on `mask` from recorded accumulators and gradients, with c large enough that at
      least one entry reaches exactly 0: the mask, the accumulator and l1_accumulation after every step;
  (c) `c_*`: a stage-1 train step whose comb_mask drops pairs so that one field is in no pair;
  (d) `d_*`: eval-mode pred of the stage-0 model on running statistics of their own.
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)

N, S, D, WIDTH, DEPTH, B = 40, 6, 5, 8, 2, 10
GRDA_C, GRDA_MU = 0.25, 0.8


def _bce(input, label):  # noqa: A002  paddle.nn.functional.binary_cross_entropy, reduction="mean": log clamped at -100
    return -(label * torch.clamp(torch.log(input), min=-100.0)
             + (1.0 - label) * torch.clamp(torch.log(1.0 - input), min=-100.0)).mean()


def _gather(x, index, axis=0):
    return torch.index_select(x, int(axis), torch.as_tensor(index).reshape(-1))


def _patch_shim():
    import paddle  # the shim
    import paddle.nn as nn
    import paddle.nn.functional as F
    if not hasattr(nn, "BatchNorm"):
        nn.BatchNorm = nn.BatchNorm1D
    if not hasattr(nn, "Identity"):
        nn.Identity = torch.nn.Identity
    paddle.gather = _gather                       # the shim's (if any) does not take a [P,1] index
    if not hasattr(paddle, "abs"):
        paddle.abs = torch.abs
    if not hasattr(paddle, "sign"):
        paddle.sign = torch.sign
    if not hasattr(F, "binary_cross_entropy"):
        F.binary_cross_entropy = _bce
    if not hasattr(torch.Tensor, "set_value"):    # optimizer.py:58
        torch.Tensor.set_value = lambda self, value: self.data.copy_(torch.as_tensor(value).detach())
    for name in ("relu", "sigmoid"):              # net.py:90, 101
        if not hasattr(F, name):
            setattr(F, name, getattr(torch, name))
    return paddle, F


def _perturb(model, rng):
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    bns = list(model.bn) + [model.bn2]
    with torch.no_grad():
        for m in list(model.linear) + bns:       # Constant(0.0) biases would hide a swapped or dropped term
            m.bias.copy_(f32(0.1 * rng.standard_normal(tuple(m.bias.shape))))
        for m in bns:
            m.weight.copy_(f32(1.0 + 0.2 * rng.standard_normal(tuple(m.weight.shape))))
    return bns


def _train_record(paddle, F, model, ids, label, g, pre):
    for k, v in model.state_dict().items():
        g[pre + k] = npy(v)
    model.train()
    pred = model.forward(paddle.to_tensor(ids))
    loss = F.binary_cross_entropy(pred, paddle.to_tensor(label.astype(np.float32)))
    loss.backward()
    g[pre + "pred"], g[pre + "loss"] = npy(pred), npy(loss).reshape(1)
    for k, v in model.state_dict(keep_vars=True).items():
        if isinstance(v, torch.nn.Parameter):
            gr = v.grad
            g[pre + "g_" + k] = np.zeros(tuple(v.shape), np.float32) if gr is None \
                else npy(gr.to_dense() if gr.is_sparse else gr)
    for k, v in model.state_dict().items():
        if k.endswith("._mean") or k.endswith("._variance"):
            g[pre + "rs_" + k] = npy(v)


def golden_autofis(seed):
    paddle, F = _patch_shim()
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    net = load_ref_module("models/rank/autofis/net.py", "ref_autofis_net")
    opt = load_ref_module("models/rank/autofis/optimizer.py", "ref_autofis_optimizer")
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    P = S * (S - 1) // 2
    ids = make_ids(rng, B, S, N)
    ids[0, 1] = ids[3, 5] = ids[7, 0] = 0
    label = (rng.random(B) < 0.5).astype(np.int64)
    g = dict(ids=ids, label=label, sizes=np.asarray([N, S, D, WIDTH, DEPTH, B], np.int64),
             grda=np.asarray([GRDA_C, GRDA_MU], np.float64))
    # (a) stage 0, one train step
    model = net.AutoDeepFMLayer(S, N, D, WIDTH, DEPTH, P, 0)
    bns = _perturb(model, rng)
    _train_record(paddle, F, model, ids, label, g, "a_")
    # (b) three SimpleGrda steps on mask, from recorded accumulators and recorded gradients
    grda = opt.SimpleGrda([model.mask], 1, GRDA_C, GRDA_MU)
    g["grda_acc0"], g["grda_mask0"] = npy(grda.accumulators[0]), npy(model.mask)
    for t in range(3):
        grad = (0.05 * rng.standard_normal((1, P))).astype(np.float32)
        model.mask.grad = torch.as_tensor(grad)
        grda.step()
        g["grda_grad%d" % (t + 1)] = grad
        g["grda_mask%d" % (t + 1)], g["grda_acc%d" % (t + 1)] = npy(model.mask), npy(grda.accumulators[0])
        g["grda_l1_%d" % (t + 1)] = np.asarray([grda.l1_accumulation], np.float64)
    assert (g["grda_mask3"] == 0).any() and (g["grda_mask3"] != 0).any(), "choose c so that some, not all, entries are 0"
    # (d) eval mode of the stage-0 model (mask as GRDA left it) on running statistics of their own
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    with torch.no_grad():
        for m in bns:
            m._mean.copy_(f32(0.3 * rng.standard_normal(tuple(m._mean.shape))))
            m._variance.copy_(f32(0.5 + rng.random(tuple(m._variance.shape))))
    for k, v in model.state_dict().items():
        g["d_" + k] = npy(v)
    model.eval()
    with torch.no_grad():
        g["d_pred"] = npy(model.forward(paddle.to_tensor(ids)))
    # (c) stage 1: a comb_mask that leaves field 2 in no pair (and drops two more pairs)
    import itertools
    comb = np.asarray([0 if 2 in pr or pr in ((0, 1), (3, 5)) else 1 for pr in itertools.combinations(range(S), 2)],
                      np.int64)
    g["c_comb_mask"] = comb
    np.save("comb_mask.npy", comb)
    model1 = net.AutoDeepFMLayer(S, N, D, WIDTH, DEPTH, P, 1)
    _perturb(model1, rng)
    _train_record(paddle, F, model1, ids, label, g, "c_")
    path = os.path.join(OUT, "autofis_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("autofis D=%d loss0=%.6f loss1=%.6f zeros=%d keys=%s -> %s (%d bytes)" % (
        D, float(g["a_loss"][0]), float(g["c_loss"][0]), int((g["grda_mask3"] == 0).sum()),
        sorted(model.state_dict().keys()), path, os.path.getsize(path)))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        golden_autofis(seed=29)
