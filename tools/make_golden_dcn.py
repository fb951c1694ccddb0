#!/usr/bin/env python3
"""Generate tests/golden/dcn_D9.npz by executing the reference's UNMODIFIED models/rank/dcn/net.py over the paddle shim
(oracle/paddle_shim), the way tools/make_golden_deepfefm.py pins rank/deepfefm.  Runs only in the build container (needs
the reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_dcn.py     # rewrites tests/golden/dcn_D9.npz deterministically

The shim has no paddle.add_n (dcn/net.py:134) and no paddle.is_compiled_with_custom_device (net.py:40): both are set
here, at run time, and nothing under oracle/ changes.  cross_num = 3 so that a middle layer exists; the dense inputs are
raw values of mixed sign and size (the reader applies no log1p for this model).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)


def golden_dcn(D, seed):
    """models/rank/dcn/net.py:21-158 + dcn/dygraph_model.py:68-75,91-98 (loss = mean log_loss + l2)."""
    import paddle  # the shim
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    if not hasattr(paddle, "add_n"):
        paddle.add_n = lambda xs: sum(xs[1:], xs[0])
    if not hasattr(paddle, "is_compiled_with_custom_device"):
        paddle.is_compiled_with_custom_device = lambda name: False
    net = load_ref_module("models/rank/dcn/net.py", "ref_dcn_net")
    rng = np.random.default_rng(seed)
    N, S, Dn, B, fc, L = 301, 26, 13, 10, [16, 8], 3
    torch.manual_seed(seed)
    # dygraph_model.py:37-41: sparse_num_field = sparse_inputs_slots - 1; clip_by_norm / l2_reg_cross / is_sparse unused
    model = net.DeepCroLayer(N, D, Dn, S, fc, L, 100.0, 0.00005, False)
    with torch.no_grad():
        # Constant(0.0) biases would hide a swapped or dropped term
        for lin in [getattr(model, "linear_%d" % i) for i in range(len(fc))] + [model.fc]:
            lin.bias.copy_(torch.as_tensor((0.1 * rng.standard_normal(tuple(lin.bias.shape))).astype(np.float32)))
    ids = make_ids(rng, B, S, N)                 # duplicates + padding ids (0)
    ids[0, 0] = ids[3, 5] = 0
    dense = (rng.standard_normal((B, Dn)) * 1.5).astype(np.float32)
    label = (rng.random((B, 1)) < 0.5).astype(np.int64)
    sparse_inputs = [paddle.to_tensor(ids[:, s:s + 1]) for s in range(S)]
    feat = model._create_embedding_input(sparse_inputs, paddle.to_tensor(dense))
    cross_out, _ = model._cross_net(feat, L)
    pred, l2 = model.forward(sparse_inputs, paddle.to_tensor(dense))
    cost = paddle.nn.functional.log_loss(input=pred, label=paddle.cast(paddle.to_tensor(label), dtype="float32"))
    loss = paddle.mean(x=cost) + l2
    loss.backward()
    g = dict(ids=ids, dense=dense, label=label, D=np.int64(D), fc=np.asarray(fc, np.int64), cross_num=np.int64(L),
             pred=npy(pred), l2=npy(l2).reshape(1), loss=npy(loss).reshape(1), cross_out=npy(cross_out))
    for k, v in model.state_dict().items():
        g[k] = npy(v)
    for k, v in model.named_parameters():
        g["g_" + k] = npy(v.grad)
    assert sorted(k for k in g if k.startswith("g_")) == sorted("g_" + k for k in model.state_dict().keys())
    path = os.path.join(OUT, "dcn_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("dcn D=%d loss=%.6f l2=%.6f keys=%s -> %s (%d bytes)" % (
        D, float(loss.detach()), float(l2.detach()), sorted(model.state_dict().keys()), path, os.path.getsize(path)))


if __name__ == "__main__":
    golden_dcn(9, seed=13)
