#!/usr/bin/env python3
"""Generate tests/golden/fat_deepffm_D9.npz by executing the reference's UNMODIFIED models/rank/fat_deepffm/net.py over the
paddle shim (oracle/paddle_shim), the way tools/make_golden_gatenet.py pins rank/gatenet.  Runs only in the build container
(needs the reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_fat_deepffm.py     # rewrites tests/golden/fat_deepffm_D9.npz deterministically

The shim has no paddle.flatten / tile / split, no nn.Sequential of (name, layer) pairs and no nn.layer.AdaptiveMaxPool1D
(net.py:97-103,131-145): stand-ins are set here, at run time, and nothing under oracle/ changes.  The pool is
torch.nn.functional.adaptive_max_pool1d on the CPU, whose backward puts the gradient on the FIRST index among equal
maxima.  The net runs in eval() mode (no Dropout): the fixture holds the bare layer's arithmetic.

With the reference's own initialisers the logit saturates (every predict 1.0, every gradient 0), so the table and
cen.dense_w are drawn at std 0.25 instead; the tool asserts that every predict lies in (0.05, 0.95) and that every
gradient tensor has max|g| >= 1e-4.  One dense field's cen.dense_w row stays constant and one dense value is 0: every
slice of those rows is a tie of the max pool.  The ids hold duplicates and the id 0, an ordinary trained row here.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)


def _stand_ins(paddle):
    nn = paddle.nn
    if not hasattr(paddle, "flatten"):
        paddle.flatten = lambda x, start_axis=0, stop_axis=-1, name=None: torch.flatten(x, start_axis, stop_axis)
    if not hasattr(paddle, "tile"):
        paddle.tile = lambda x, repeat_times: x.repeat(*([1] * (x.dim() - len(repeat_times)) + list(repeat_times)))
    if not hasattr(paddle, "split"):
        paddle.split = lambda x, num_or_sections, axis=0: list(torch.split(x, x.shape[axis] // num_or_sections, dim=axis))
    if not hasattr(nn, "Sequential"):
        class Sequential(nn.Layer):
            def __init__(self, *pairs):
                super().__init__()
                for name, layer in pairs:
                    self.add_sublayer(name, layer)

            def forward(self, x):
                for layer in self._modules.values():
                    x = layer(x)
                return x
        nn.Sequential = Sequential
    if not hasattr(nn, "layer"):
        class AdaptiveMaxPool1D(nn.Layer):
            def __init__(self, output_size):
                super().__init__()
                self.output_size = output_size

            def forward(self, x):
                return torch.nn.functional.adaptive_max_pool1d(x, self.output_size)
        nn.layer = types.SimpleNamespace(AdaptiveMaxPool1D=AdaptiveMaxPool1D)


def golden_fat_deepffm(D, seed):
    """models/rank/fat_deepffm/net.py:22-251 + fat_deepffm/dygraph_model.py:52-58 (loss = mean log_loss)."""
    import paddle  # the shim
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    _stand_ins(paddle)
    net = load_ref_module("models/rank/fat_deepffm/net.py", "ref_fat_deepffm_net")
    rng = np.random.default_rng(seed)
    N, S, Dn, B, fc = 301, 6, 3, 10, [16, 8]
    R = (S + Dn) * D
    torch.manual_seed(seed)
    # dygraph_model.py:24-36: sparse_num_field = sparse_inputs_slots - 1
    model = net.FAT_DeepFFMLayer(N, D, Dn, S, fc)
    model.eval()
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    with torch.no_grad():
        model.cen.embedding.weight.copy_(f32(0.25 * rng.standard_normal((N, R))))
        dw = 0.25 * rng.standard_normal((1, Dn, R))
        dw[0, 1, :] = 0.25                       # one dense field keeps a constant row (the rescaled Constant(1.0)): all
                                                 # of its slices tie
        model.cen.dense_w.copy_(f32(dw))
        # Constant(0.0) biases would hide a swapped or dropped term
        lins = [model.cen.fc.ReductionLinear, model.cen.fc.AdditionLinear] + \
            [getattr(model.dnn, "linear_%d" % i) for i in range(len(fc) + 1)]
        for lin in lins:
            lin.bias.copy_(f32(0.1 * rng.standard_normal(tuple(lin.bias.shape))))
        model.bias.copy_(f32(0.1 * rng.standard_normal(1)))
    ids = make_ids(rng, B, S, N)                 # duplicates + ids 0 (a live row here)
    ids[0, 0] = ids[3, 5] = 0
    dense = rng.random((B, Dn), dtype=np.float32)
    dense[2, 0] = 0.0                            # a whole row of zeros: every slice ties
    label = (rng.random((B, 1)) < 0.5).astype(np.int64)
    sparse_inputs = [paddle.to_tensor(ids[:, s:s + 1]) for s in range(S)]
    pred = model.forward(sparse_inputs, paddle.to_tensor(dense))
    cost = paddle.nn.functional.log_loss(input=pred, label=paddle.cast(paddle.to_tensor(label), "float32"))
    loss = paddle.mean(cost)
    loss.backward()
    g = dict(ids=ids, dense=dense, label=label, D=np.int64(D), fc=np.asarray(fc, np.int64), pred=npy(pred),
             loss=npy(loss).reshape(1))
    for k, v in model.state_dict().items():
        g[k] = npy(v)
    for k, v in model.named_parameters():
        gr = v.grad
        g["g_" + k] = npy(gr.to_dense() if gr.is_sparse else gr)      # cen.embedding.weight: densified
    assert sorted(k for k in g if k.startswith("g_")) == sorted("g_" + k for k in model.state_dict().keys())
    assert 0.05 < g["pred"].min() and g["pred"].max() < 0.95, (g["pred"].min(), g["pred"].max())
    gmax = {k: float(np.abs(v).max()) for k, v in g.items() if k.startswith("g_")}
    assert min(gmax.values()) >= 1e-4, gmax
    path = os.path.join(OUT, "fat_deepffm_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("fat_deepffm D=%d loss=%.6f pred %.3f..%.3f min max|g| %.2e (%s) keys=%s -> %s (%d bytes)" % (
        D, float(loss.detach()), g["pred"].min(), g["pred"].max(), min(gmax.values()), min(gmax, key=gmax.get),
        sorted(model.state_dict().keys()), path, os.path.getsize(path)))


if __name__ == "__main__":
    golden_fat_deepffm(9, seed=17)
