"""rank/deepfefm on the engine — field-embedded FM + DNN on the HIP kernels of csrc/fefm_ops.hip.

Host mirror of the reference's models/rank/deepfefm/net.py (`DeepFEFMLayer`, `FEFM`, `DNN`) and deepfefm/dygraph_model.py:
    predict = sigmoid(y_first_order + y_field_emb_second_order + y_dnn)                     net.py:43-52
    x[b,f]  = embedding[id[b,f]], id of dense field k = int64(dense_k * 1e5 + 1e6 + 2)       net.py:135-146
    t[b,p]  = x_i^T (FE_p + FE_p^T) x_j for the P = F(F-1)/2 field pairs                    net.py:149-169
    dnn_in  = [x of the sparse fields | dense * dense_w_one | t]                             net.py:179-185
(rec_fefm_fwd / rec_fefm_bwd).  Quirks of the reference that are mirrored, DESIGN.md section 8:
  * the dense values are looked up in the SAME embedding table through the derived id (padding_idx 0 on both tables);
  * `bias` is a registered parameter that forward never uses: it is in the state_dict and never moves;
  * the pair matrices live in a plain dict, so the dygraph reference neither trains nor saves them.  Default here:
    frozen at their initial draw (train_field_embeddings=False); True trains them (d_FE, L2Decay(1e-7), Adam) as the
    static-graph model does.  Either way they are saved under the extra key `fefm.field_embeddings` [P, D, D].
  * Dropout(0.2) follows EVERY element of the DNN's layer list: twice per hidden layer, once after the last Linear.
Regularizers: L2Decay(1e-6) on embedding, embedding_one, dense_w_one; L2Decay(1e-7) on the Linear weights and the pair
matrices.  Both Embeddings are sparse=False: under the dygraph default (lazy_mode=False) every row moves every step with
g + 1e-6 * w (rec_adam_rows_all_l2); lazy_mode=True (an extension) decays only the rows a batch touches.
The table is kept at a row stride of round_up(D, 4) floats; `fefm.embedding.weight` is the [:, :D] view and the pad
columns stay 0.  The bare layer defaults to dropout_rate 0 (the reference's eval() arithmetic, what the golden fixture
holds); DygraphModel.create_model builds it with the reference's 0.2.  There is no autograd tape and no CPU fallback.
"""
import math

import torch

from .deepfm import _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up

L2_EMB = 1e-6       # net.py:77,90,96
L2_DNN = 1e-7       # net.py:111,219
FE_KEY = "fefm.field_embeddings"


class DeepFEFMLayer(SlotLayerBase):
    """deepfefm/net.py:23-52.  forward(sparse_inputs, dense_inputs) -> predict [B,1] (eval mode: no dropout).
    set_dict with a dict without `fefm.field_embeddings` (a checkpoint of the reference) keeps the current matrices;
    grad_dict()'s gradients include the L2 terms."""
    lazy_mode = False   # the dygraph default; the trainer's hyper_parameters.optimizer.lazy_mode sets it

    def __init__(self, sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field, layer_sizes,
                 device="cuda", kernels=None, dropout_rate=0.0, dropout_seed=2025, train_field_embeddings=False):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = N = sparse_feature_number
        self.sparse_feature_dim = D = sparse_feature_dim
        self.dense_feature_dim = Dn = dense_feature_dim
        self.sparse_num_field = S = sparse_num_field
        self.layer_sizes = list(layer_sizes)
        self.dropout_rate, self.dropout_seed = float(dropout_rate), int(dropout_seed)
        self.train_field_embeddings = bool(train_field_embeddings)
        self.num_fields = F = S + Dn
        self.num_pairs = P = F * (F - 1) // 2
        self.input_size = S * D + Dn + P                                     # net.py:205-207
        self.row_pad = _round_up(D, 4)
        std = 0.1 / math.sqrt(float(D))                                      # net.py:64-116 TruncatedNormal
        f32 = dict(dtype=torch.float32, device=self.device)
        self.emb_table = torch.zeros(N, self.row_pad, **f32)
        self.embedding = self.emb_table[:, :D]
        self.embedding_one = torch.zeros(N, 1, **f32)
        for t in (self.embedding_one, self.embedding):
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std)
            t[0].zero_()                                                     # padding_idx = 0
        sizes = [self.input_size] + self.layer_sizes + [1]
        shapes = [("bias", (1,)), ("fefm.dense_w_one", (Dn,))]
        for i in range(len(sizes) - 1):
            shapes += [("dnn.linear_%d.weight" % i, (sizes[i], sizes[i + 1])), ("dnn.linear_%d.bias" % i, (sizes[i + 1],))]
        shapes += [(FE_KEY, (P, D, D))]
        self.dense = _FlatParams(shapes, self.device)
        p = self.dense.p
        torch.nn.init.trunc_normal_(p["fefm.dense_w_one"], 0.0, std, -2 * std, 2 * std)
        torch.nn.init.trunc_normal_(p[FE_KEY], 0.0, std, -2 * std, 2 * std)
        for i in range(len(sizes) - 1):
            p["dnn.linear_%d.weight" % i].normal_(0.0, 1.0 / math.sqrt(sizes[i]))   # net.py:220-221
        self.ws_fefm = self.k.Workspace(self.device)

    # -- parameters under the reference's state_dict keys (+ fefm.field_embeddings) ---------------
    def state_dict(self):
        sd = {"fefm.embedding_one.weight": self.embedding_one, "fefm.embedding.weight": self.embedding}
        sd.update(self.dense.p)
        return sd

    def _fefm(self, ids, dense_inputs):
        """rec_fefm_fwd writes the MLP's input in place: a [B, input_size] view of rows padded to 4 floats."""
        p = self.dense.p
        B = ids.shape[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        buf = torch.empty(B, _round_up(self.input_size, 4), **f32)
        out = (torch.empty(B, 1, **f32), torch.empty(B, 1, **f32), buf[:, :self.input_size],
               torch.empty(B, self.num_fields, dtype=torch.int64, device=self.device))
        return self.k.fefm_fwd(ids, dense_inputs, self.emb_table, self.embedding_one, p["fefm.dense_w_one"], p[FE_KEY],
                               self.sparse_feature_dim, self.ws_fefm, status=self.status, out=out)

    def forward(self, sparse_inputs, dense_inputs):
        ids = self._concat_ids(sparse_inputs)
        y1, y2, dnn_in, _, _ = self._fefm(ids, dense_inputs)
        W, b, _, _ = self._linears("dnn.linear_%d", len(self.layer_sizes) + 1)
        y_dnn, _ = self.k.mlp_forward(dnn_in, W, b, self.ws)
        return torch.sigmoid(y1 + y2 + y_dnn)

    __call__ = forward

    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            self.sparse_state = self._separate_moments(*self.emb_table.shape)

    def _drop(self):
        return self.dropout_rate > 0.0

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, dense_inputs, label, lr=1e-3, auc_stats=None):
        """deepfefm/dygraph_model.py train_forward + tools/trainer.py backward / step.  label [B,1] int64.
        Returns (loss [1] device tensor, pred [B,1])."""
        k, p, g = self.k, self.dense.p, self.dense.g
        ids = self._concat_ids(sparse_inputs)                      # net.py:120-121
        B, S = ids.shape
        D, F = self.sparse_feature_dim, self.num_fields
        t, cur, side, (groups, groups1) = self._begin_step(B * F, B * S)
        y1, y2, dnn_in, ids_all, _ = self._fefm(ids, dense_inputs)
        with _OnSide(side, cur):                                   # merge keys: the table's are ids_all, W1's the sparse ids
            k.ids_group(ids_all, self.sparse_feature_number, 0, self.ws_group, None, self.status, groups)
            k.ids_group(ids, self.sparse_feature_number, 0, self.ws_group, None, self.status, groups1)
        # DNN.forward (net.py:229-234): Dropout after every element of _mlp_layers; relu(drop(z)) = drop(relu(z)), so a
        # hidden layer is the GEMM's bias+ReLU epilogue followed by ONE dropout pass with two mask streams
        n = len(self.layer_sizes)
        W, b, dW, db = self._linears("dnn.linear_%d", n + 1)
        drop, rate, seed = self._drop(), self.dropout_rate, self.dropout_seed
        nstreams = 2 * n + 1
        base = t * nstreams
        acts, x = [], dnn_in
        for i in range(n):
            acts.append(x)
            x = k.gemm(x, W[i], self.ws, epilogue="bias_relu", bias=b[i])
            if drop:
                k.dropout(x, rate, seed, base + 2 * i, base + 2 * i + 1, step_stride=nstreams)
        acts.append(x)
        y_dnn = k.gemm(x, W[n], self.ws, epilogue="bias", bias=b[n])
        if drop:
            k.dropout(y_dnn, rate, seed, base + 2 * n, step_stride=nstreams)
        pred, dz, loss = k.sigmoid_logloss(y1, y2, y_dnn, label, self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        # backward of the tower
        gy = dz.reshape(B, 1)
        if drop:
            gy = k.dropout(gy, rate, seed, base + 2 * n, out=torch.empty_like(gy), step_stride=nstreams)
        for i in reversed(range(n + 1)):
            k.gemm(acts[i], gy, self.ws, trans_a=True, out=dW[i], b_colsum=db[i])
            if i > 0:
                gy = k.gemm(gy, W[i], self.ws, trans_b=True, epilogue="relu_mask", aux0=acts[i])
                if drop:
                    k.dropout(gy, rate, seed, base + 2 * (i - 1), base + 2 * (i - 1) + 1, step_stride=nstreams)
            else:
                gy = k.gemm(gy, W[0], self.ws, trans_b=True)
        d_dnn_in = gy
        tfe = self.train_field_embeddings
        row_grad, _, _ = k.fefm_bwd(ids_all, dense_inputs, self.emb_table, p[FE_KEY], dz, d_dnn_in, S, D, self.ws_fefm,
                                    want_d_fe=tfe, status=self.status,
                                    out=(self._buf("_rg", (B * F, self.row_pad)), g["fefm.dense_w_one"],
                                         g[FE_KEY] if tfe else None))
        st = self.sparse_state
        self._update_rows(t, lr, cur, side, (groups, row_grad, 1, self.emb_table, st["m"], st["v"]),
                          (groups1, dz, S, self.embedding_one, st["m1"], st["v1"]), l2=L2_EMB)
        k.l2_decay_grad(g["fefm.dense_w_one"], p["fefm.dense_w_one"], L2_EMB)
        for i in range(n + 1):
            k.l2_decay_grad(dW[i].reshape(-1), W[i].reshape(-1), L2_DNN)
        if tfe:
            k.l2_decay_grad(g[FE_KEY].reshape(-1), p[FE_KEY].reshape(-1), L2_DNN)
        # `bias` keeps a zero gradient and zero moments: Adam moves it by exactly 0.  The pair matrices are the LAST tensor of
        # the flat buffer: frozen, the Adam launch stops in front of them (no pass over them, and moments loaded from a
        # checkpoint of a run that trained them cannot move them)
        self._finish_step(t, lr, cur, side, n_adam=self.dense.data.numel() if tfe else self.dense.offsets[FE_KEY])
        self._last = dict(row_grad=row_grad, ids_all=ids_all, dz=dz)
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """deepfefm/dygraph_model.py."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return DeepFEFMLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                             g("hyper_parameters.dense_input_dim"), g("hyper_parameters.sparse_inputs_slots") - 1,
                             g("hyper_parameters.fc_sizes"), device=device, kernels=kernels,
                             dropout_rate=0.2,                       # the DNN constructor's default (net.py:197), no YAML key
                             dropout_seed=g("runner.seed", 12345),
                             train_field_embeddings=bool(g("hyper_parameters.train_field_embeddings", False)))
