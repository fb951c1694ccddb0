#!/usr/bin/env python3
"""Generate tests/golden/deepfefm_D9.npz by executing the reference's UNMODIFIED models/rank/deepfefm/net.py over the
paddle shim (oracle/paddle_shim), the way tools/make_golden_ffm.py pins rank/ffm.  Runs only in the build container
(needs the reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_deepfefm.py     # rewrites tests/golden/deepfefm_D9.npz deterministically

The shim has no paddle.squeeze and no paddle.shape (deepfefm/net.py:153-158, myutils.batch_dot): both are set here, at
run time, and nothing under oracle/ changes.  net.py does `from myutils import *`, so the model directory goes on
sys.path.  The dense inputs are drawn as -10 + u * 1e-3: the ids net.py:138 derives from them then fall in 2 .. 102 and
a table of 160 rows holds them (with the reader's [0, 1] values they start at 1 000 002).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, REF, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)


def golden_deepfefm(D, seed):
    """models/rank/deepfefm/net.py:23-234 in eval mode + deepfefm/dygraph_model.py (loss)."""
    import paddle  # the shim
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    paddle.squeeze = lambda x, axis=None: torch.squeeze(x) if axis is None else torch.squeeze(x, axis)
    paddle.shape = lambda x: torch.as_tensor(x.shape)
    sys.path.insert(0, os.path.join(REF, "models/rank/deepfefm"))
    net = load_ref_module("models/rank/deepfefm/net.py", "ref_deepfefm_net")
    rng = np.random.default_rng(seed)
    N, S, Dn, B, fc = 160, 26, 13, 10, [16, 8]
    F = S + Dn
    torch.manual_seed(seed)
    model = net.DeepFEFMLayer(N, D, Dn, S, fc)   # dygraph_model.py:34-36: sparse_num_field = sparse_inputs_slots - 1
    model.eval()
    pairs = [str(i) + "-" + str(j) for i in range(F) for j in range(i + 1, F)]      # itertools.combinations order
    assert list(model.fefm.field_embeddings.keys()) == pairs
    with torch.no_grad():
        # Constant(0.0) values (bias, the Linear biases) would hide a swapped or dropped term
        model.bias.copy_(torch.as_tensor(np.asarray([-0.63], np.float32)))
        for i in range(len(fc) + 1):
            b = getattr(model.dnn, "linear_%d" % i).bias
            b.copy_(torch.as_tensor((0.1 * rng.standard_normal(tuple(b.shape))).astype(np.float32)))
    ids = make_ids(rng, B, S, N)                 # duplicates + padding ids (0)
    ids[0, 0] = ids[3, 5] = 0
    dense = (np.float32(-10.0) + rng.random((B, Dn), dtype=np.float32) * np.float32(1e-3)).astype(np.float32)
    dense_ids = (dense * np.float32(1e5) + np.float32(1e6) + np.float32(2)).astype(np.int64)
    assert dense_ids.min() >= 2 and dense_ids.max() < N, (dense_ids.min(), dense_ids.max())
    label = (rng.random((B, 1)) < 0.5).astype(np.int64)
    sparse_inputs = [paddle.to_tensor(ids[:, s:s + 1]) for s in range(S)]
    fe = [model.fefm.field_embeddings[k] for k in pairs]
    pred = model.forward(sparse_inputs, paddle.to_tensor(dense))
    cost = paddle.nn.functional.log_loss(input=pred, label=paddle.cast(paddle.to_tensor(label), dtype="float32"))
    loss = paddle.mean(x=cost)
    y1, y2, dnn_in = model.fefm.forward(sparse_inputs, paddle.to_tensor(dense))
    loss.backward()
    assert model.bias.grad is None               # registered, never used by forward
    g = dict(ids=ids, dense=dense, label=label, D=np.int64(D), fc=np.asarray(fc, np.int64), dense_ids=dense_ids,
             W=npy(model.fefm.embedding.weight), W1=npy(model.fefm.embedding_one.weight),
             dense_w_one=npy(model.fefm.dense_w_one), bias=npy(model.bias), FE=np.stack([npy(t) for t in fe]),
             pred=npy(pred), loss=npy(loss), y1=npy(y1), y2=npy(y2), t=npy(dnn_in)[:, S * D + Dn:],
             gW=npy(model.fefm.embedding.weight.grad), gW1=npy(model.fefm.embedding_one.weight.grad),
             g_dense_w_one=npy(model.fefm.dense_w_one.grad), gFE=np.stack([npy(t.grad) for t in fe]))
    for i in range(len(fc) + 1):
        lin = getattr(model.dnn, "linear_%d" % i)
        g["lin_w%d" % i], g["lin_b%d" % i] = npy(lin.weight), npy(lin.bias)
        g["g_lin_w%d" % i], g["g_lin_b%d" % i] = npy(lin.weight.grad), npy(lin.bias.grad)
    path = os.path.join(OUT, "deepfefm_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("deepfefm D=%d loss=%.6f dense ids %d..%d -> %s (%d bytes)" % (
        D, float(loss.detach()), dense_ids.min(), dense_ids.max(), path, os.path.getsize(path)))


if __name__ == "__main__":
    golden_deepfefm(9, seed=9)
