#!/usr/bin/env python3
"""Generate tests/golden/flen_D8.npz by executing the reference's UNMODIFIED models/rank/flen/net.py over the paddle shim
(oracle/paddle_shim), the way tools/make_golden_gatenet.py pins rank/gatenet.  Runs only in the build container (needs the
reference tree); the GPU box uses the committed fixture.

    python tools/make_golden_flen.py     # rewrites tests/golden/flen_D8.npz deterministically

The shim has no paddle.gather (flen/net.py:222-224) and no F.binary_cross_entropy (flen/dygraph_model.py:54-58): both are
set here, at run time, and nothing under oracle/ changes.  The fixture holds two records from ONE parameter set:
  (a) train() mode with the p of every Dropout instance set to 0: pred, loss, every gradient (the table's densified;
      kernel_fm, which forward never uses, gets zeros) and the running statistics after the step (`rs_<key>`);
  (b) eval() mode after non-trivial running statistics (`eval_<key>`) were set: `pred_eval` only.
The Linear and BatchNorm biases are non-zero so that a dropped term shows; the ids hold duplicates and the id 0, an
ordinary trainable row in this net (the Embedding has no padding_idx); column 0 of the 23 inputs is never used.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np   # noqa: E402
import torch         # noqa: E402

from oracle.make_golden import OUT, load_ref_module, make_ids, npy   # noqa: E402  (puts the shim on sys.path)


def _bce(input, label):  # noqa: A002  paddle.nn.functional.binary_cross_entropy, reduction="mean": log clamped at -100
    return -(label * torch.clamp(torch.log(input), min=-100.0)
             + (1.0 - label) * torch.clamp(torch.log(1.0 - input), min=-100.0)).mean()


def golden_flen(D, seed):
    """models/rank/flen/net.py:24-257 + flen/dygraph_model.py:53-60 (loss = mean binary_cross_entropy)."""
    import paddle  # the shim
    import paddle.nn.functional as F
    torch.set_num_threads(1)                     # the CPU embedding backward sums duplicate rows in thread order
    if not hasattr(paddle, "gather"):
        paddle.gather = lambda x, index, axis=0: torch.index_select(x, int(axis), index)
    if not hasattr(F, "binary_cross_entropy"):
        F.binary_cross_entropy = _bce
    net = load_ref_module("models/rank/flen/net.py", "ref_flen_net")
    rng = np.random.default_rng(seed)
    N, S, G, B, sizes = 40, 22, 3, 10, [16, 8]
    torch.manual_seed(seed)
    model = net.FLENLayer(N, D, S, G, sizes)
    bns = [model.fwbi_bn] + [getattr(model._DNNLayer, "norm_%d" % i) for i in range(len(sizes))]
    lins = [model.fwbi_fc_32, model.linear] + [getattr(model._DNNLayer, "linear_%d" % i) for i in range(len(sizes))]
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    with torch.no_grad():
        for m in lins + bns:                     # Constant(0.0) biases would hide a swapped or dropped term
            m.bias.copy_(f32(0.1 * rng.standard_normal(tuple(m.bias.shape))))
        for m in bns:
            m.weight.copy_(f32(1.0 + 0.2 * rng.standard_normal(tuple(m.weight.shape))))
    ids = make_ids(rng, B, S + 1, N)             # duplicates + ids 0 (a live row here); column 0 is dead
    ids[0, 1] = ids[3, 5] = ids[7, 22] = 0
    label = (rng.random((B, 1)) < 0.5).astype(np.int64)
    g = dict(ids=ids, label=label, D=np.int64(D), sizes=np.asarray(sizes, np.int64))
    for k, v in model.state_dict().items():
        g[k] = npy(v)
    # (a) train mode, dropout off
    model.train()
    for m in model.modules():
        if isinstance(m, paddle.nn.Dropout):
            m.p = 0.0
    sparse_inputs = [paddle.to_tensor(ids[:, s:s + 1]) for s in range(S + 1)]
    pred = model.forward(sparse_inputs)
    loss = paddle.mean(F.binary_cross_entropy(input=pred, label=paddle.cast(paddle.to_tensor(label), "float32")))
    loss.backward()
    g.update(pred=npy(pred), loss=npy(loss).reshape(1))
    params = {k: v for k, v in model.state_dict(keep_vars=True).items() if isinstance(v, torch.nn.Parameter)}
    for k, v in params.items():                  # both aliases linear.* / linear_out.* of the head are listed
        gr = v.grad
        g["g_" + k] = np.zeros(tuple(v.shape), np.float32) if gr is None else npy(gr.to_dense() if gr.is_sparse else gr)
    assert not g["g__FieldWiseBiInteraction.kernel_fm"].any()
    for k, v in model.state_dict().items():
        if k.endswith("._mean") or k.endswith("._variance"):
            g["rs_" + k] = npy(v)
    # (b) eval mode on running statistics of their own
    with torch.no_grad():
        for m in bns:
            m._mean.copy_(f32(0.3 * rng.standard_normal(tuple(m._mean.shape))))
            m._variance.copy_(f32(0.5 + rng.random(tuple(m._variance.shape))))
    for k, v in model.state_dict().items():
        if k.endswith("._mean") or k.endswith("._variance"):
            g["eval_" + k] = npy(v)
    model.eval()
    with torch.no_grad():
        g["pred_eval"] = npy(model.forward(sparse_inputs))
    path = os.path.join(OUT, "flen_D%d.npz" % D)
    np.savez_compressed(path, **g)
    print("flen D=%d loss=%.6f keys=%s -> %s (%d bytes)" % (
        D, float(loss.detach()), sorted(model.state_dict().keys()), path, os.path.getsize(path)))


if __name__ == "__main__":
    golden_flen(8, seed=23)
