#!/usr/bin/env python3
"""Generate tests/golden/gatenet_D9.npz by executing the reference's UNMODIFIED models/rank/gatenet/net.py over the paddle
shim (oracle/paddle_shim), the way tools/make_golden_dcn.py pins rank/dcn.  Runs only in the build container (needs the
reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_gatenet.py     # rewrites tests/golden/gatenet_D9.npz deterministically

The shim's paddle.create_parameter takes no name= (gatenet/net.py:34-38,76-81) and its Layer has no add_parameter
(net.py:42,82): both are set here, at run time, and nothing under oracle/ changes.  Both gates are on; the ids hold
duplicates and the id 0, which is an ordinary trainable row in this net (the Embedding has no padding_idx).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)


def golden_gatenet(D, seed):
    """models/rank/gatenet/net.py:20-121 + gatenet/dygraph_model.py:56-60 (loss = mean log_loss)."""
    import paddle  # the shim
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    plain_create = paddle.create_parameter
    if "name" not in plain_create.__code__.co_varnames:
        paddle.create_parameter = lambda shape, dtype="float32", name=None, **kw: plain_create(list(shape), dtype, **kw)
    if not hasattr(paddle.nn.Layer, "add_parameter"):
        paddle.nn.Layer.add_parameter = lambda self, name, p: self.register_parameter(name, p)
    net = load_ref_module("models/rank/gatenet/net.py", "ref_gatenet_net")
    rng = np.random.default_rng(seed)
    N, S, Dn, B, fc = 301, 26, 13, 10, [16, 8]
    torch.manual_seed(seed)
    # dygraph_model.py:36-39: num_field = sparse_inputs_slots - 1
    model = net.GateDNNLayer(N, D, Dn, S, fc, True, True)
    with torch.no_grad():
        # Constant(0.0) biases would hide a swapped or dropped term
        for lin in [getattr(model, "linear_%d" % i) for i in range(len(fc))] + [model.last_layer]:
            lin.bias.copy_(torch.as_tensor((0.1 * rng.standard_normal(tuple(lin.bias.shape))).astype(np.float32)))
    ids = make_ids(rng, B, S, N)                 # duplicates + ids 0 (a live row here)
    ids[0, 0] = ids[3, 5] = 0
    dense = (rng.standard_normal((B, Dn)) * 1.5).astype(np.float32)
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
        g["g_" + k] = npy(gr.to_dense() if gr.is_sparse else gr)      # embedding.weight: densified
    assert sorted(k for k in g if k.startswith("g_")) == sorted("g_" + k for k in model.state_dict().keys())
    path = os.path.join(OUT, "gatenet_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("gatenet D=%d loss=%.6f keys=%s -> %s (%d bytes)" % (
        D, float(loss.detach()), sorted(model.state_dict().keys()), path, os.path.getsize(path)))


if __name__ == "__main__":
    golden_gatenet(9, seed=17)
