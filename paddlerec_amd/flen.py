"""rank/flen on the engine — FLEN's field-wise bi-interaction fused into the lookup (csrc/flen_ops.hip), its towers on the
engine's GEMM / BatchNorm / dropout kernels, and paddle.optimizer.Adagrad on rec_adagrad_rows / rec_adagrad_dense.

Host mirror of the reference's models/rank/flen/net.py (`FLENLayer`, `EmbeddingLayer`, `DNNLayer`,
`FieldWiseBiInteraction`) and flen/dygraph_model.py (`DygraphModel`):
    E[b,s]  = embedding(sparse_inputs[1 + s]), s < S = 22;   X0 = [E_0 | .. | E_{S-1}]                  net.py:67-79
    FW[b,g] = sum of E[b,s] over the slots of field group g (user 13, item 3, context 6)               net.py:205-210
    h_mf    = sum over the group pairs i < j of kernel_mf[p] * FW_i * FW_j                              net.py:215-229
    fwbi    = drop(BN(relu(h_mf @ W + b)))                                                             net.py:84-87
    dnn     = X0 through Linear, drop, ReLU, drop, BN, drop per layer                                  net.py:157-164
    pred    = sigmoid(linear([fwbi | dnn]))                                                            net.py:89-95
    loss    = mean binary_cross_entropy(pred, label)                                         dygraph_model.py:53-60
Quirks of the reference that are mirrored (FLEN):
  * the inputs are 23 columns and column 0 is never used: the net takes sparse_inputs[1:14], [14:17] and [17:];
    `sparse_inputs_slots` (22) counts the lookups, not the columns;
  * one shared Embedding, raw ids, no padding_idx (id 0 is an ordinary, trained row), XavierUniform;
  * the "FM module" (net.py:234-255) is dead code: forward returns h_mf only, so kernel_fm is a parameter of the
    state_dict that never gets a gradient;
  * Dropout(0.2) follows EVERY element of the DNN's layer list — three per layer, the last layer included, none on the
    input.  relu(drop(z)) = drop(relu(z)), so a layer is the GEMM's bias+ReLU epilogue, one dropout pass with two mask
    streams, BN, and one more dropout pass: 3n + 1 mask streams per step with fwbi_drop;
  * BatchNorm1D has Paddle's semantics (momentum 0.9, eps 1e-5, biased variance); at batch size 1 (the sample
    config.yaml) every BN output equals its bias, pred = sigmoid(linear.bias) and nothing upstream of a BN moves;
  * `linear` and `linear_out` are two names of the head (net.py:58-64): both keys of state_dict() are one tensor.
Optimizer: paddle.optimizer.Adagrad(lr, epsilon=1e-6, initial_accumulator_value=1e-3) over all parameters
(dygraph_model.py:63-73).  The sparse=True table's gradient is a SelectedRows: duplicates are merged first, then the rule
runs on the touched rows; a zero gradient is an exact no-op, so there is no lazy / non-lazy distinction and kernel_fm sits
in the flat dense buffer with a zero gradient.  The accumulators live where checkpoint.optimizer_state looks for Adam's
first moments: sparse_state["m"] and dense.m.
The table is the line-aligned record buffer of dcn.py: rec [N, round_up(D, 32)], the embedding its [:, :D] view (D = 32:
one 128-byte line per row).  The bare layer defaults to dropout_rate 0 (what the golden fixture holds);
DygraphModel.create_model builds it with the reference's 0.2.  The only torch arithmetic of a step is plumbing: dropping
column 0 of the ids and the label's cast to float32.  There is no autograd tape and no CPU fallback.
"""
import itertools
import math

import torch

from .deepfm import _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up

EMB = "_EmbeddingLayer.embedding.weight"
KMF, KFM = "_FieldWiseBiInteraction.kernel_mf", "_FieldWiseBiInteraction.kernel_fm"
LIN, NORM = "_DNNLayer.linear_%d", "_DNNLayer.norm_%d"
FC, FBN, HEAD, HEAD_ALIAS = "fwbi_fc_32", "fwbi_bn", "linear", "linear_out"
BN_MOMENTUM, BN_EPS = 0.9, 1e-5
ADAGRAD_EPS, ADAGRAD_INIT = 1e-6, 1e-3             # dygraph_model.py:68-72
DROPOUT = 0.2                                      # net.py:56, 128


class FLENLayer(SlotLayerBase):
    """flen/net.py:24-95.  forward(sparse_inputs) -> predict [B,1] (eval mode: running statistics, no dropout);
    sparse_inputs: the 23 [B,1] tensors or one [B,23] tensor."""

    def __init__(self, sparse_feature_number, sparse_feature_dim, sparse_inputs_slots, sparse_num_field, layer_sizes_dnn,
                 field_sizes=None, device="cuda", kernels=None, dropout_rate=0.0, dropout_seed=2025):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = N = int(sparse_feature_number)
        self.sparse_feature_dim = D = int(sparse_feature_dim)
        self.sparse_inputs_slots = S = int(sparse_inputs_slots)
        self.sparse_num_field = G = int(sparse_num_field)
        self.layer_sizes_dnn = sizes_dnn = [int(x) for x in layer_sizes_dnn]
        self.dropout_rate, self.dropout_seed = float(dropout_rate), int(dropout_seed)
        if field_sizes is None:                                              # net.py:67-69: [1:14], [14:17], [17:]
            field_sizes = (13, 3, S - 16)
        self.field_sizes = tuple(int(x) for x in field_sizes)
        if len(self.field_sizes) != G or min(self.field_sizes) < 1 or sum(self.field_sizes) != S:
            raise ValueError("field_sizes %s must be %d positive group sizes that sum to sparse_inputs_slots = %d"
                             % (self.field_sizes, G, S))
        if not sizes_dnn or sizes_dnn[-1] != D:                              # net.py:58-60, 89-92: the head is Linear(2D -> 1)
            raise ValueError("layer_sizes_dnn %s must end in sparse_feature_dim = %d: the head is Linear(2 * %d -> 1) over "
                             "[fwbi | dnn]" % (sizes_dnn, D, D))
        self.group_begin = [0] + list(itertools.accumulate(self.field_sizes))
        self.num_pairs = P = G * (G - 1) // 2
        self.ld_x0 = _round_up(S * D, 4)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.rec = torch.zeros(N, _round_up(D, 32), **f32)
        self.embedding = self.rec[:, :D]
        xavier = lambda t, fan_in, fan_out: t.uniform_(-math.sqrt(6.0 / (fan_in + fan_out)),
                                                       math.sqrt(6.0 / (fan_in + fan_out)))
        xavier(self.embedding, N, D)                                         # net.py:106-111
        sizes = [S * D] + sizes_dnn
        shapes = [(KMF, (P, 1)), (KFM, (G, 1)), (FC + ".weight", (D, D)), (FC + ".bias", (D,)),
                  (FBN + ".weight", (D,)), (FBN + ".bias", (D,))]
        for i in range(len(sizes_dnn)):
            shapes += [(LIN % i + ".weight", (sizes[i], sizes[i + 1])), (LIN % i + ".bias", (sizes[i + 1],)),
                       (NORM % i + ".weight", (sizes[i + 1],)), (NORM % i + ".bias", (sizes[i + 1],))]
        shapes += [(HEAD + ".weight", (2 * D, 1)), (HEAD + ".bias", (1,))]
        self.dense = _FlatParams(shapes, self.device)
        self.dense.m.fill_(ADAGRAD_INIT)                                     # dense.m: the Adagrad accumulator
        p = self.dense.p
        xavier(p[KMF], P, 1)                                                 # net.py:179-187
        xavier(p[KFM], G, 1)
        xavier(p[FC + ".weight"], D, D)
        xavier(p[HEAD + ".weight"], 2 * D, 1)
        self.buffers = {}
        for name, n in [(FBN, D)] + [(NORM % i, sizes[i + 1]) for i in range(len(sizes_dnn))]:
            p[name + ".weight"].fill_(1.0)
            self.buffers[name + "._mean"] = torch.zeros(n, **f32)
            self.buffers[name + "._variance"] = torch.ones(n, **f32)
        for i in range(len(sizes_dnn)):
            xavier(p[LIN % i + ".weight"], sizes[i], sizes[i + 1])           # net.py:140-144
        self.ws_bn = self.k.Workspace(self.device)
        self.ws_bwd = self.k.Workspace(self.device)

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def state_dict(self):
        sd = {EMB: self.embedding}
        sd.update(self.dense.p)
        sd.update(self.buffers)
        for nm in (".weight", ".bias"):                                      # net.py:64: add_sublayer('linear_out', self.linear)
            sd[HEAD_ALIAS + nm] = sd[HEAD + nm]
        return sd

    def parameters(self):
        return [self.embedding] + list(self.dense.p.values())                # the running statistics are buffers

    def grad_dict(self):
        g = dict(self.dense.g)
        for nm in (".weight", ".bias"):
            g[HEAD_ALIAS + nm] = g[HEAD + nm]
        return g

    # -- paddle.optimizer.Adagrad in place of the base's Adam -------------------------------------
    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            acc = torch.full_like(self.rec, ADAGRAD_INIT)
            self.sparse_state = dict(acc=acc, m=acc[:, :self.sparse_feature_dim])

    def _rows_update(self, t, lr, groups, grad, div, P, M, V, **kw):
        self.k.adagrad_rows(groups, grad, div, P, M, lr, ADAGRAD_EPS, **kw)

    def _dense_update(self, t, lr, p, m, v, g):
        self.k.adagrad_dense(p, m, g, lr, ADAGRAD_EPS)

    # -- forward ------------------------------------------------------------------------------------
    def _ids(self, sparse_inputs):
        ids = self._concat_ids(sparse_inputs)
        if ids.dim() != 2 or ids.shape[1] != self.sparse_inputs_slots + 1:
            raise ValueError("flen takes %d sparse inputs (column 0 is unused), got %s"
                             % (self.sparse_inputs_slots + 1, tuple(ids.shape)))
        return ids[:, 1:].contiguous()                                       # net.py:67-69

    def _bn(self, name, x, training, out=None):
        p = self.dense.p
        return self.k.batchnorm_fwd(x, p[name + ".weight"], p[name + ".bias"], self.buffers[name + "._mean"],
                                    self.buffers[name + "._variance"], self.ws_bn, training, BN_MOMENTUM, BN_EPS, out=out)

    def _logit(self, ids, training, streams=None):
        """-> (logit [B,1], saved).  streams: the first dropout mask stream of this step (train mode with dropout), or
        None.  The two halves of the head's input are written straight into one [B, 2D] buffer."""
        k, p = self.k, self.dense.p
        B, S = ids.shape
        D, G, n = self.sparse_feature_dim, self.sparse_num_field, len(self.layer_sizes_dnn)
        rate, seed, ns = self.dropout_rate, self.dropout_seed, 3 * n + 1
        X0, h, FW, _ = k.flen_fwd(ids, self.embedding, self.group_begin, p[KMF], self.status,
                                  out=(self._buf("_x0", (B, self.ld_x0))[:, :S * D], self._buf("_h", (B, D)),
                                       self._buf("_fw", (B, G * D))))
        cat = self._buf("_cat", (B, 2 * D))
        W, b, _, _ = self._linears(LIN, n)
        x, cache = X0, []
        for i in range(n):
            z = k.gemm(x, W[i], self.ws, epilogue="bias_relu", bias=b[i])             # Linear, (drop), ReLU
            if streams is not None:
                k.dropout(z, rate, seed, streams + 3 * i, streams + 3 * i + 1, step_stride=ns)
            y, mu, invstd = self._bn(NORM % i, z, training, out=cat[:, D:] if i == n - 1 else None)
            if streams is not None:
                k.dropout(y, rate, seed, streams + 3 * i + 2, step_stride=ns)
            cache.append((x, z, mu, invstd))
            x = y
        fz = k.gemm(h, p[FC + ".weight"], self.ws, epilogue="bias_relu", bias=p[FC + ".bias"])    # net.py:84-85
        fy, fmu, finvstd = self._bn(FBN, fz, training, out=cat[:, :D])
        if streams is not None:
            k.dropout(fy, rate, seed, streams + 3 * n, step_stride=ns)
        logit = k.gemm(cat, p[HEAD + ".weight"], self.ws, epilogue="bias", bias=p[HEAD + ".bias"])
        return logit, dict(h=h, FW=FW, cat=cat, cache=cache, fz=fz, fmu=fmu, finvstd=finvstd)

    def forward(self, sparse_inputs):
        logit, _ = self._logit(self._ids(sparse_inputs), False)
        return torch.sigmoid(logit)                                                  # net.py:93

    __call__ = forward

    def eval_loss(self, sparse_inputs, label):
        """Eval-mode (pred [B,1], mean binary cross entropy [1]) — what the reference's infer_forward prints."""
        logit, _ = self._logit(self._ids(sparse_inputs), False)
        pred, _, loss = self.k.bce_with_logits(logit, label.to(torch.float32).reshape(-1, 1).contiguous(), self.ws)
        return pred, loss

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, label, lr=1e-3, auc_stats=None):
        """flen/dygraph_model.py:84-96 + tools/trainer.py backward / step.  label [B,1] int64.
        Returns (loss [1] device tensor = mean binary cross entropy, pred [B,1])."""
        k, p, g = self.k, self.dense.p, self.dense.g
        ids = self._ids(sparse_inputs)
        B, S = ids.shape
        D, n = self.sparse_feature_dim, len(self.layer_sizes_dnn)
        rate, seed, ns = self.dropout_rate, self.dropout_seed, 3 * n + 1
        t, cur, side, groups = self._begin_step(B * S)
        with _OnSide(side, cur):                                   # the merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, None, self.ws_group, None, self.status, groups)
        streams = t * ns if rate > 0.0 else None
        logit, sv = self._logit(ids, True, streams)
        # sigmoid + F.binary_cross_entropy = BCE with logits wherever sigmoid(logit) is not exactly 0 or 1 in float32
        # (Paddle clamps log at -100 there and its gradient vanishes)
        pred, dz, loss = k.bce_with_logits(logit, label.to(torch.float32).reshape(-1, 1).contiguous(), self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        cat = sv["cat"]
        k.gemm(cat, dz, self.ws, trans_a=True, out=g[HEAD + ".weight"], b_colsum=g[HEAD + ".bias"])
        dcat = k.gemm(dz, p[HEAD + ".weight"], self.ws, trans_b=True)
        # the fwbi branch: drop <- BN <- ReLU <- Linear <- h_mf
        dfy = dcat[:, :D]
        if streams is not None:
            k.dropout(dfy, rate, seed, streams + 3 * n, step_stride=ns)
        dfz, _, _ = k.batchnorm_bwd(sv["fz"], dfy, p[FBN + ".weight"], sv["fmu"], sv["finvstd"], self.ws_bn, relu_mask=True,
                                    dgamma=g[FBN + ".weight"], dbeta=g[FBN + ".bias"])
        dH = k.linear_backward(sv["h"], dfz, p[FC + ".weight"], self.ws, g[FC + ".weight"], g[FC + ".bias"])
        # the DNN: the BN's input is a dropped ReLU output, so its ReLU-mask form covers the ReLU and the zeroed lanes; the
        # dropout pass behind it restores the kept lanes' scale
        W, _, dW, db = self._linears(LIN, n)
        dx0_buf = self._buf("_dx0", (B, self.ld_x0))
        dx = dcat[:, D:]
        for i in reversed(range(n)):
            x, z, mu, invstd = sv["cache"][i]
            if streams is not None:
                k.dropout(dx, rate, seed, streams + 3 * i + 2, step_stride=ns)
            dz_i, _, _ = k.batchnorm_bwd(z, dx, p[NORM % i + ".weight"], mu, invstd, self.ws_bn, relu_mask=True,
                                         dgamma=g[NORM % i + ".weight"], dbeta=g[NORM % i + ".bias"])
            if streams is not None:
                k.dropout(dz_i, rate, seed, streams + 3 * i, streams + 3 * i + 1, step_stride=ns)
            dx = k.linear_backward(x, dz_i, W[i], self.ws, dW[i], db[i], out=dx0_buf[:, :S * D] if i == 0 else None)
        # d loss / d X0 -> the per-lookup row gradient, in the same slots; kernel_fm's gradient stays zero
        k.flen_bwd(ids, self.sparse_feature_number, self.group_begin, p[KMF], sv["FW"], dH, dx, self.ws_bwd, self.status,
                   out=g[KMF].view(-1))
        self._update_rows(t, lr, cur, side, (groups, dx0_buf, 1, self.embedding, self.sparse_state["m"], None),
                          grad_group=S, grad_group_stride=self.ld_x0)    # lookup (b, s) = dx0[b, s*D : (s+1)*D]
        self._finish_step(t, lr, cur, side)
        self._last = dict(row_grad=dx, dH=dH, dz=dz)
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """flen/dygraph_model.py:24-109."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return FLENLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                         g("hyper_parameters.sparse_inputs_slots"), g("hyper_parameters.sparse_num_field"),
                         g("hyper_parameters.layer_sizes_dnn"), device=device, kernels=kernels,
                         dropout_rate=DROPOUT,                           # net.py:56, 128: no YAML key
                         dropout_seed=g("runner.seed", 12345))

    def create_feeds(self, batch_data, config, device="cuda"):
        """dygraph_model.py:43-50: the label is the LAST of the 24 columns and there is no dense input.  -> (label [B,1]
        i64, sparse).  batch_data: the reference's 24 arrays (sparse = list of 23 [B,1] tensors) or the (label [B,1],
        ids [B,23]) device tensors of paddlerec_amd.reader.AvazuReader (sparse = the [B,23] tensor)."""
        if len(batch_data) == 2 and torch.is_tensor(batch_data[1]) and batch_data[1].dim() == 2 \
                and batch_data[1].shape[1] > 1:
            return batch_data[0].to(device), batch_data[1].to(device)
        sparse = [torch.as_tensor(b).to(torch.int64).reshape(-1, 1).to(device) for b in batch_data]
        return sparse[-1], sparse[:-1]

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        label, sparse = self.create_feeds(batch_data, config, dy_model.device)
        lr = config.get("hyper_parameters.optimizer.learning_rate", 0.001)
        loss, _ = dy_model.train_step(sparse, label, lr, metrics_list[0] if metrics_list else None)
        return loss, metrics_list, {"loss": loss}                        # dygraph_model.py:95

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        label, sparse = self.create_feeds(batch_data, config, dy_model.device)
        pred, loss = dy_model.eval_loss(sparse, label)
        if metrics_list:
            dy_model.k.auc_histogram(pred.contiguous(), label.contiguous(), metrics_list[0][0], metrics_list[0][1],
                                     NUM_THRESHOLDS)
        return metrics_list, {"logloss": loss}                           # dygraph_model.py:108
