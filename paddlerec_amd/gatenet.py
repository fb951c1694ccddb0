"""rank/gatenet on the engine — GateNet's embedding gate fused into the lookup and its hidden gate around the tower's GEMMs,
on the HIP kernels of csrc/gate_ops.hip.

Host mirror of the reference's models/rank/gatenet/net.py (`GateDNNLayer`) and gatenet/dygraph_model.py (`DygraphModel`):
    e_s       = embedding(ids[:, s]);  out_s = e_s * sigmoid(w_s * sum_k e_s[k])                       net.py:88-103
    feat      = [out_0 | .. | out_{S-1} | dense (Dn, raw)]                                             net.py:110
    y_i       = relu(x @ W_i + b_i);  x = y_i * tanh(y_i @ G_i)      every layer, the last included     net.py:112-118
    pred      = sigmoid(last_layer(x))                                                                 net.py:119-120
    loss      = mean log_loss(pred, label)                                                             dygraph_model.py:56-60
Quirks of the reference that are mirrored (the rank/gatenet section):
  * the embedding gate's weight is ONE scalar per field (`shape=[1]`), not a vector as in the GateNet paper: the gate of a
    lookup is sigmoid(w_s * sum_k e_k).  state_dict() holds the S scalars under `embedding_gate_weight_0 .. _{S-1}`; the
    layer keeps them as one [S] vector (`embedding_gate_weight` of the flat parameter buffer);
  * the Embedding has no padding_idx: id 0 is an ordinary trainable row (padding_idx is None here);
  * the table is drawn U[-1, 1] (`Uniform()`), the gate scalars N(0, 1);
  * the dygraph Adam is not lazy: every row's moments move each step (lazy_mode=False).  lazy_mode=True (an extension)
    touches only the batch's rows.
`use_embedding_gate=False` is the plain lookup (rec_emb_gather), `use_hidden_gate=False` the plain ReLU tower; the
state_dict then has no gate keys, as in the reference.
The table is the line-aligned record buffer of dcn.py: rec [N, round_up(D, 32)], `embedding.weight` the [:, :D] view.  The
feature rows are kept at a row stride rounded up to 4 floats; rec_gate_emb_fwd writes the gated lookups into their head
and rec_gate_emb_bwd turns the layer-0 dX into d loss / d e in the same slots, where the sparse Adam reads it.  The only
torch arithmetic of a step is plumbing: the [B, Dn] dense values copied into the feature row.  There is no autograd tape
and no CPU fallback.
"""
import math

import torch

from .deepfm import _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up

GATE_VEC = "embedding_gate_weight"          # the [S] vector behind the keys embedding_gate_weight_%d


class GateDNNLayer(SlotLayerBase):
    """gatenet/net.py:20-121.  forward(sparse_inputs, dense_inputs) -> pred [B,1]."""
    lazy_mode = False   # the dygraph default; the trainer's hyper_parameters.optimizer.lazy_mode sets it

    def __init__(self, sparse_feature_number, sparse_feature_dim, dense_feature_dim, num_field, layer_sizes,
                 use_embedding_gate=True, use_hidden_gate=True, device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = N = sparse_feature_number
        self.sparse_feature_dim = D = sparse_feature_dim
        self.dense_feature_dim = Dn = dense_feature_dim
        self.num_field = S = num_field
        self.layer_sizes = list(layer_sizes)
        self.use_embedding_gate, self.use_hidden_gate = bool(use_embedding_gate), bool(use_hidden_gate)
        if not self.layer_sizes:
            raise ValueError("gatenet needs at least one tower layer")
        self.d = d = S * D + Dn
        self.d_pad = _round_up(d, 4)
        self.padding_idx = None                                              # net.py:44-50: no padding row
        f32 = dict(dtype=torch.float32, device=self.device)
        self.rec = torch.zeros(N, _round_up(D, 32), **f32)
        self.embedding = self.rec[:, :D]
        self.embedding.uniform_(-1.0, 1.0)                                   # net.py:50 Uniform()
        sizes = [d] + self.layer_sizes
        shapes = [(GATE_VEC, (S,))] if self.use_embedding_gate else []
        for i in range(len(self.layer_sizes)):
            shapes += [("linear_%d.weight" % i, (sizes[i], sizes[i + 1])), ("linear_%d.bias" % i, (sizes[i + 1],))]
            if self.use_hidden_gate:
                shapes.append(("hidden_gate_weight_%d" % i, (sizes[i + 1], sizes[i + 1])))
        shapes += [("last_layer.weight", (sizes[-1], 1)), ("last_layer.bias", (1,))]
        self.dense = _FlatParams(shapes, self.device)
        p = self.dense.p
        if self.use_embedding_gate:
            p[GATE_VEC].normal_(0.0, 1.0)                                    # net.py:34-38
        for i in range(len(self.layer_sizes)):
            p["linear_%d.weight" % i].normal_(0.0, 1.0 / math.sqrt(sizes[i]))                # net.py:63-68
            if self.use_hidden_gate:
                p["hidden_gate_weight_%d" % i].normal_(0.0, 1.0 / math.sqrt(sizes[i + 1]))   # net.py:76-81
        p["last_layer.weight"].normal_(0.0, 1.0 / math.sqrt(sizes[-1]))                      # net.py:55-60

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def _named(self, tensors):
        out = {}
        for k, v in tensors.items():
            if k == GATE_VEC:
                out.update(("%s_%d" % (GATE_VEC, s), v[s:s + 1]) for s in range(self.num_field))
            else:
                out[k] = v
        return out

    def state_dict(self):
        sd = {"embedding.weight": self.embedding}
        sd.update(self._named(self.dense.p))
        return sd

    def grad_dict(self):
        return self._named(self.dense.g)

    # -- forward pieces ---------------------------------------------------------------------------
    def _feat(self, ids, dense_inputs):
        """net.py:87-110: the (gated) lookups written straight into the head of the feature row, the raw dense values
        behind them.  -> the [B, d] view of a [B, d_pad] buffer."""
        B, S = ids.shape
        D, d = self.sparse_feature_dim, self.d
        buf = torch.empty(B, self.d_pad, dtype=torch.float32, device=self.device)
        if self.use_embedding_gate:
            self.k.gate_emb_fwd(ids, self.embedding, self.dense.p[GATE_VEC], self.padding_idx, self.status,
                                out=buf[:, :S * D])
        else:
            self.k.emb_gather(ids.reshape(-1), self.embedding, self.padding_idx, self.status, out=buf, out_group=S,
                              out_group_stride=self.d_pad)
        buf[:, S * D:d].copy_(dense_inputs)
        return buf[:, :d]

    def _logit(self, ids, dense_inputs):
        """-> (logit [B,1], saved): xs[i] the input of tower layer i (xs[-1] the last_layer's), ys[i] its ReLU output,
        hs[i] = tanh(ys[i] @ G_i) (with the hidden gate)."""
        k, p = self.k, self.dense.p
        W, b, _, _ = self._linears("linear_%d", len(self.layer_sizes))
        x = self._feat(ids, dense_inputs)
        xs, ys, hs = [x], [], []
        for i in range(len(W)):
            y = k.gemm(x, W[i], self.ws, epilogue="bias_relu", bias=b[i])            # net.py:113 Linear + ReLU
            x = y
            if self.use_hidden_gate:                                                 # net.py:114-118
                t = k.gemm(y, p["hidden_gate_weight_%d" % i], self.ws)
                x, h = k.gate_hidden_fwd(y, t)
                hs.append(h)
            ys.append(y)
            xs.append(x)
        logit = k.gemm(x, p["last_layer.weight"], self.ws, epilogue="bias", bias=p["last_layer.bias"])
        return logit, dict(xs=xs, ys=ys, hs=hs)

    def forward(self, sparse_inputs, dense_inputs):
        ids = self._concat_ids(sparse_inputs)
        logit, _ = self._logit(ids, dense_inputs)
        return torch.sigmoid(logit)                                                  # net.py:120

    __call__ = forward

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, dense_inputs, label, lr=1e-3, auc_stats=None):
        """gatenet/dygraph_model.py:78-90 + tools/trainer.py backward / step.  label [B,1] int64.
        Returns (loss [1] device tensor = mean log-loss, pred [B,1])."""
        k, p, g = self.k, self.dense.p, self.dense.g
        ids = self._concat_ids(sparse_inputs)
        B, S = ids.shape
        D, d = self.sparse_feature_dim, self.d
        t, cur, side, groups = self._begin_step(B * S)
        with _OnSide(side, cur):                                   # the merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, self.padding_idx, self.ws_group, None, self.status, groups)
        logit, sv = self._logit(ids, dense_inputs)
        pred, dz, loss = k.sigmoid_logloss(logit, None, None, label, self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        xs, ys, hs = sv["xs"], sv["ys"], sv["hs"]
        W, _, dW, db = self._linears("linear_%d", len(self.layer_sizes))
        n = len(W)
        lw = p["last_layer.weight"]
        k.gemm(xs[n], dz, self.ws, trans_a=True, out=g["last_layer.weight"], b_colsum=g["last_layer.bias"])
        dfeat_buf = self._buf("_dfeat", (B, self.d_pad))
        dfeat = dfeat_buf[:, :d]
        if self.use_hidden_gate:
            u = k.gemm(dz, lw, self.ws, trans_b=True)                                # d loss / d x of the top layer
            for i in reversed(range(n)):
                G = p["hidden_gate_weight_%d" % i]
                dt, uh = k.gate_hidden_bwd(u, ys[i], hs[i])
                k.gemm(ys[i], dt, self.ws, trans_a=True, out=g["hidden_gate_weight_%d" % i])
                dy = k.gemm(dt, G, self.ws, trans_b=True, epilogue="add", aux1=uh)   # through the gate's GEMM + direct
                k.relu_mask_(dy, ys[i])                                              # the ReLU's mask is y's
                u = k.linear_backward(xs[i], dy, W[i], self.ws, dW[i], db[i], out=dfeat if i == 0 else None)
        else:
            gy = k.gemm(dz, lw, self.ws, trans_b=True, epilogue="relu_mask", aux0=xs[n])
            for i in reversed(range(n)):
                gy = k.linear_backward(xs[i], gy, W[i], self.ws, dW[i], db[i], relu_src=xs[i] if i > 0 else None,
                                       out=dfeat if i == 0 else None)
        if self.use_embedding_gate:                                # d loss / d out -> d loss / d e, in the same slots
            k.gate_emb_bwd(ids, self.embedding, p[GATE_VEC], dfeat_buf[:, :S * D], self.ws, self.padding_idx, self.status,
                           out=g[GATE_VEC])
        st = self.sparse_state
        self._update_rows(t, lr, cur, side, (groups, dfeat_buf, 1, self.embedding, st["m"], st["v"]),
                          grad_group=S, grad_group_stride=self.d_pad)     # lookup (b, s) = dfeat[b, s*D : (s+1)*D]
        self._finish_step(t, lr, cur, side)
        self._last_dfeat = dfeat
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """gatenet/dygraph_model.py:23-100."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return GateDNNLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                            g("hyper_parameters.dense_input_dim"), g("hyper_parameters.sparse_inputs_slots") - 1,
                            g("hyper_parameters.fc_sizes"), g("hyper_parameters.use_embedding_gate"),
                            g("hyper_parameters.use_hidden_gate"), device=device, kernels=kernels)
