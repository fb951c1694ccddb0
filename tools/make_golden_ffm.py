#!/usr/bin/env python3
"""Generate tests/golden/ffm_D9.npz by executing the reference's UNMODIFIED models/rank/ffm/net.py over the paddle shim
(oracle/paddle_shim), the way oracle/make_golden.py pins the other nets.  Runs only in the build container (needs the
reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_ffm.py          # rewrites tests/golden/ffm_D9.npz deterministically

The shim has no paddle.add_n (ffm/net.py:132 sums the 741 pair terms with it): it is set here, at run time, to the
left-to-right sum of the list, and nothing under oracle/ changes.
"""
import functools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)


def golden_ffm(D, seed):
    """models/rank/ffm/net.py:21-133 + ffm/dygraph_model.py:50-55 (loss)."""
    import paddle  # the shim
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    paddle.add_n = lambda xs: functools.reduce(torch.add, xs)
    net = load_ref_module("models/rank/ffm/net.py", "ref_ffm_net")
    rng = np.random.default_rng(seed)
    N, S, Dn, B = 144, 26, 13, 10
    F = S + Dn                                   # dygraph_model.py:31-32: sparse_inputs_slots - 1 + dense_input_dim
    torch.manual_seed(seed)
    model = net.FFMLayer(N, D, Dn, F)
    with torch.no_grad():
        # the Constant(1.0) dense weights saturate the sigmoid (a toy batch gives loss 6.91: pred is 0 or 1 and every
        # gradient vanishes) and, being all equal, would hide a swapped or dropped weight; Constant(0.0) bias likewise
        model.ffm.dense_w_one.copy_(torch.as_tensor(0.05 * (1.0 + 0.5 * rng.standard_normal(Dn)).astype(np.float32)))
        model.ffm.dense_w.copy_(torch.as_tensor(
            0.05 * (1.0 + 0.5 * rng.standard_normal((1, Dn, F * D))).astype(np.float32)))
        model.bias.copy_(torch.as_tensor(np.asarray([-0.63], np.float32)))
    ids = make_ids(rng, B, S, N)                 # duplicates + id 0 (an ordinary row here: no padding_idx)
    ids[0, 0] = ids[3, 5] = 0
    dense = rng.random((B, Dn), dtype=np.float32)
    label = (rng.random((B, 1)) < 0.5).astype(np.int64)
    sparse_inputs = [paddle.to_tensor(ids[:, s:s + 1]) for s in range(S)]
    pred = model.forward(sparse_inputs, paddle.to_tensor(dense))
    cost = paddle.nn.functional.log_loss(input=pred, label=paddle.cast(paddle.to_tensor(label), dtype="float32"))
    loss = paddle.mean(x=cost)
    y1, y2 = model.ffm.forward(sparse_inputs, paddle.to_tensor(dense))
    loss.backward()
    g = dict(ids=ids, dense=dense, label=label, D=np.int64(D),
             W=npy(model.ffm.embedding.weight), W1=npy(model.ffm.embedding_one.weight),
             dense_w=npy(model.ffm.dense_w), dense_w_one=npy(model.ffm.dense_w_one), bias=npy(model.bias),
             pred=npy(pred), loss=npy(loss), y1=npy(y1), y2=npy(y2),
             gW=npy(model.ffm.embedding.weight.grad), gW1=npy(model.ffm.embedding_one.weight.grad),
             g_dense_w=npy(model.ffm.dense_w.grad), g_dense_w_one=npy(model.ffm.dense_w_one.grad),
             g_bias=npy(model.bias.grad))
    path = os.path.join(OUT, "ffm_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("ffm D=%d loss=%.6f -> %s (%d bytes)" % (D, float(loss.detach()), path, os.path.getsize(path)))


if __name__ == "__main__":
    golden_ffm(9, seed=9)
