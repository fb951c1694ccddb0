#!/usr/bin/env python3
"""Generate tests/golden/dien_D8.npz, tests/golden/dien_sample.txt and tests/golden/dien_reader.npz by executing the
reference's UNMODIFIED models/rank/dien/net.py and dien_reader.py over the paddle shim (oracle/paddle_shim), the way
tools/make_golden_autofis.py pins rank/autofis.  Runs only in the build container (needs the reference tree); the GPU
box uses the committed fixtures.

    python tools/make_golden_dien.py     # rewrites the three fixtures deterministically

What the shim lacks is set here, at run time, and nothing under oracle/ changes: nn.GRU and nn.GRUCell over torch's
(same gate order r, z, c and the same Uniform(+-1/sqrt(H)) start; Paddle's return shapes: GRU -> (outputs, state),
GRUCell -> (h, h)), paddle.slice, paddle.subtract, paddle.log, paddle.clip without bounds (net.py:235: the identity), paddle.zeros, paddle.io.IterableDataset, F.softmax, and
Tensor.unsqueeze(axis=[0]) (net.py:271).  That torch's GRU equals Paddle's rests on Paddle's documented formula: Paddle
itself is not installable here.  The reader writes ./tmp.txt (dien_reader.py:44), so the script runs in a temporary
directory.

dien_D8.npz: item dim 4, cat dim 4, B 5, T 6, lengths 6 4 1 3 6, tables of 31 / 29 rows; duplicate ids, the id 0 at a
valid position of every id feed; every bias (Linear, attention Linear, GRU, item_b) is non-zero.  Records the ten feeds,
state_dict (`p_*`), the attention MLP that state_dict does not list (`att_w*`, `att_b*`), logit, aux, loss, cost, every
gradient (`g_*`, tables dense) and the parameters after one SGD step at lr 0.85 (`n_*`).
dien_reader.npz: the reference reader's first batches on dien_sample.txt at batch size 4 (`b<i>_<feed>`), once with
the counts of config.yaml and once with item_count 30000 (the count filter drops lines).
"""
import os
import random
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, REF, load_ref_module, npy   # noqa: E402  (puts the shim on sys.path)

EI, EC, B, T, ITEMS, CATS, LR = 4, 4, 5, 6, 31, 29, 0.85
LENS = (6, 4, 1, 3, 6)
SAMPLE_LINES = 60
FEEDS = ("hist_item_seq", "hist_cat_seq", "target_item", "target_cat", "label", "mask", "target_item_seq",
         "target_cat_seq", "neg_hist_item_seq", "neg_hist_cat_seq")


class _GRU(torch.nn.GRU):
    def __init__(self, input_size, hidden_size, num_layers=1, direction="forward", time_major=False, dropout=0.0, **kw):
        super().__init__(input_size, hidden_size, num_layers=num_layers, batch_first=not time_major)

    def forward(self, inputs, initial_states=None, sequence_length=None):
        return super().forward(inputs, initial_states)


class _GRUCell(torch.nn.GRUCell):
    def __init__(self, input_size, hidden_size, **kw):
        super().__init__(input_size, hidden_size)

    def forward(self, inputs, states=None):
        h = super().forward(inputs, states)
        return h, h


def _slice(x, axes, starts, ends):
    idx = [slice(None)] * x.dim()
    for a, s, e in zip(axes, starts, ends):
        idx[a] = slice(s, e)
    return x[tuple(idx)]


def _patch_shim():
    import types
    import paddle  # the shim
    import paddle.nn as nn
    import paddle.nn.functional as F
    nn.GRU, nn.GRUCell = _GRU, _GRUCell
    paddle.slice = _slice
    paddle.subtract = lambda x, y: x - y
    paddle.log = torch.log
    paddle.clip = lambda x, min=None, max=None: x if min is None and max is None else torch.clamp(x, min=min, max=max)
    paddle.zeros = lambda shape, dtype="float32": torch.zeros(list(shape), dtype=getattr(torch, dtype))
    if not hasattr(F, "softmax"):
        F.softmax = lambda x, axis=-1: torch.softmax(x, dim=axis)
    if "paddle.io" not in sys.modules:
        io = types.ModuleType("paddle.io")
        io.IterableDataset = object
        sys.modules["paddle.io"] = paddle.io = io
    orig = torch.Tensor.unsqueeze
    if not getattr(orig, "_dien", False):
        def unsqueeze(self, dim=None, axis=None):
            a = dim if axis is None else axis
            return orig(self, a[0] if isinstance(a, (list, tuple)) else a)
        unsqueeze._dien = True
        torch.Tensor.unsqueeze = unsqueeze
    return paddle, F


def golden_dien(seed):
    paddle, F = _patch_shim()
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    net = load_ref_module("models/rank/dien/net.py", "ref_dien_net")
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = net.DIENLayer(EI, EC, "sigmoid", False, False, ITEMS, CATS)
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    with torch.no_grad():                        # Constant(0.0) biases would hide a dropped or swapped term
        for m in list(model.attention_layer) + list(model.top_layer):
            if hasattr(m, "bias"):
                m.bias.copy_(f32(0.1 * rng.standard_normal(tuple(m.bias.shape))))
        model.item_b_attr.weight.copy_(f32(0.1 * rng.standard_normal((ITEMS, 1))))
    lens = np.asarray(LENS)
    valid = np.arange(T)[None, :] < lens[:, None]
    hi = np.where(valid, rng.integers(1, ITEMS, (B, T)), 0).astype(np.int64)
    hc = np.where(valid, rng.integers(1, CATS, (B, T)), 0).astype(np.int64)
    hi[0, 2], hc[0, 2] = hi[0, 0], hc[0, 0]      # duplicates inside a sample and across samples
    hi[4, 1], hc[4, 1] = hi[0, 0], hc[0, 0]
    hi[1, 1] = hc[3, 0] = 0                      # the padding id at a VALID position
    ti = rng.integers(1, ITEMS, B).astype(np.int64)
    tc = rng.integers(1, CATS, B).astype(np.int64)
    ti[3], tc[3] = ti[0], tc[0]
    ti[1] = tc[2] = 0
    label = (rng.random(B) < 0.5).astype(np.float32)
    mask = np.where(valid, 0.0, -1e9).astype(np.float32).reshape(B, T, 1)
    ni = rng.integers(0, ITEMS, (B, T)).astype(np.int64)
    nc = rng.integers(0, CATS, (B, T)).astype(np.int64)
    ni[0, 1], nc[2, 2] = 0, 0
    ni[1, 3] = ni[0, 2]
    feeds = (hi, hc, ti, tc, label, mask, np.repeat(ti[:, None], T, 1), np.repeat(tc[:, None], T, 1), ni, nc)
    g = dict(sizes=np.asarray([EI, EC, B, T, ITEMS, CATS], np.int64), lr=np.asarray([LR], np.float64),
             lens=lens.astype(np.int64))
    for name, a in zip(FEEDS, feeds):
        g[name] = a
    for k, v in model.state_dict().items():
        g["p_" + k] = npy(v)
    lin = [m for m in model.attention_layer if hasattr(m, "weight")]
    for i, m in enumerate(lin):
        g["att_w%d" % i], g["att_b%d" % i] = npy(m.weight), npy(m.bias)
    dm = load_ref_dygraph(net)
    tt = [paddle.to_tensor(a) for a in feeds]
    logit, aux = model.forward(tt[0], tt[1], tt[2], tt[3], tt[4].reshape(-1, 1), *tt[5:])
    loss = dm.create_loss(logit, tt[4].reshape(-1, 1))
    cost = loss + aux
    opt = torch.optim.SGD(model.parameters(), lr=LR)
    cost.backward()
    g["logit"], g["aux"], g["loss"], g["cost"] = npy(logit), npy(aux).reshape(1), npy(loss).reshape(1), npy(cost).reshape(1)
    for k, v in model.state_dict(keep_vars=True).items():
        gr = v.grad
        g["g_" + k] = np.zeros(tuple(v.shape), np.float32) if gr is None else npy(gr)
    for m in lin:
        assert m.weight.grad is not None and not any(m.weight is q for q in model.parameters())   # used, never trained
    before = [npy(m.weight) for m in lin]
    opt.step()
    for k, v in model.state_dict().items():
        g["n_" + k] = npy(v)
    assert all((npy(m.weight) == b).all() for m, b in zip(lin, before))
    path = os.path.join(OUT, "dien_D%d.npz" % (EI + EC))
    np.savez_compressed(path, **g)
    print("dien logit0=%.6f aux=%.6f cost=%.6f keys=%s -> %s (%d bytes)" % (
        float(g["logit"][0, 0]), float(g["aux"][0]), float(g["cost"][0]), sorted(model.state_dict().keys()), path,
        os.path.getsize(path)))


def load_ref_dygraph(net):
    sys.modules["net"] = net                                              # dygraph_model.py: `import net`
    return load_ref_module("models/rank/dien/dygraph_model.py", "ref_dien_dygraph").DygraphModel()


def golden_reader():
    _patch_shim()
    src = os.path.join(REF, "models/rank/dien/data/train_data/sample_data.txt")
    sample = os.path.join(OUT, "dien_sample.txt")
    with open(src) as f, open(sample, "w") as o:
        o.writelines(f.readlines()[:SAMPLE_LINES])
    rd = load_ref_module("models/rank/dien/dien_reader.py", "ref_dien_reader")
    g = {}
    for tag, items in (("a", 63001), ("f", 30000)):
        cfg = {"runner.train_batch_size": 4, "hyper_parameters.item_count": items, "hyper_parameters.cat_count": 801}
        random.seed(0)
        rows = list(rd.RecDataset([sample], cfg))
        g[tag + "_count"] = np.asarray([len(rows)], np.int64)
        for b in range(min(3, len(rows) // 4)):
            for j, name in enumerate(FEEDS):
                g["%s%d_%s" % (tag, b, name)] = np.stack([np.asarray(r[j]) for r in rows[4 * b:4 * b + 4]])
    path = os.path.join(OUT, "dien_reader.npz")
    np.savez_compressed(path, **g)
    print("dien reader: %d / %d samples -> %s (%d bytes)" % (int(g["a_count"][0]), int(g["f_count"][0]), path,
                                                             os.path.getsize(path)))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        golden_dien(seed=31)
        golden_reader()
