"""rank/fat_deepffm on the engine — CENet field attention + field-pair Hadamard DNN on the HIP kernels of
csrc/fatffm_ops.hip.

Host mirror of the reference's models/rank/fat_deepffm/net.py (`FAT_DeepFFMLayer`, `CENLayer`, `DeepFFM`, `DNNLayer`) and
fat_deepffm/dygraph_model.py (`DygraphModel`):
    predict = sigmoid(y_first_order + y_dnn + bias)                                      net.py:47-57
    E[i, j, :] = block j of field i's R = F*D wide row: W[id_i] or dense_k * dense_w[k]   net.py:108-122
    a       = relu(relu(max_d E @ W_red + b_red) @ W_add + b_add)   over the F*F slices   net.py:126-137 (reduction = 1)
    y_first_order = sum of the whole scaled cube a * E, the diagonal slices included      net.py:221-222
    H[p]    = a[i,j] E[i,j,:] * a[j,i] E[j,i,:] for the P = F(F-1)/2 pairs i < j          net.py:231-249
    y_dnn   = Linear(P*D -> ..) relu .. Linear(.. -> 1)                                    net.py:180-203
(rec_fatffm_pool_fwd / _inter_fwd / _attn_bwd / _bwd; the Linears are the engine's GEMMs).  F = S + Dn: the constructor's
sparse_num_field is the number of sparse slots S (dygraph_model.py:33-35), unlike ffm's.  Quirks of the reference that
are mirrored (FAT-DeepFFM):
  * the max pool's backward puts the gradient on the FIRST index among equal maxima; dense_w starts at Constant(1.0), so
    every slice of a dense field is one tie;
  * the Embedding has NO padding_idx (id 0 is an ordinary, trained row) and there is no separate first-order table;
  * Dropout(0.5) follows EVERY element of the DNN's layer list: twice per hidden layer and once after the last Linear's
    [B,1] output (net.py:200-202);
  * L2Decay(1e-7) on the three DNN Linear weights only;
  * with the reference's own initialisers and sizes (F 39, D 10) the logit saturates on dense values of order 1: every
    such predict is 1.0 in float32 and every gradient is 0.  The engine reproduces that; it is not "fixed".
Optimizer: paddle.optimizer.Adam (dygraph_model.py:60-64), lazy_mode=False unless the trainer switches it.
The table is kept at a padded row width Rp = round_up(R, 4) (392 for the reference's 390) so that its rows load as
16-byte vectors; `cen.embedding.weight` is the [:, :R] view and the pad columns stay 0, as in ffm.py.  The matrices
between the kernels and the GEMMs (pooled, a, H and their gradients) are allocated with leading dimensions rounded up to
4 floats.  The bare layer defaults to dropout_rate 0 and no L2 (the reference's eval() arithmetic, what the golden
fixture holds); DygraphModel.create_model builds it with the reference's 0.5 and 1e-7.  There is no autograd tape and no
CPU fallback.
"""
import math

import torch

from .deepfm import _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up

L2_DNN = 1e-7       # net.py:188
RED, ADD = "cen.fc.ReductionLinear", "cen.fc.AdditionLinear"


class FAT_DeepFFMLayer(SlotLayerBase):
    """fat_deepffm/net.py:22-57.  forward(sparse_inputs, dense_inputs) -> predict [B,1] (eval mode: no dropout).
    grad_dict()'s gradients include the L2 terms."""
    lazy_mode = False   # the dygraph default; the trainer's hyper_parameters.optimizer.lazy_mode sets it

    def __init__(self, sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field, layer_sizes,
                 device="cuda", kernels=None, dropout_rate=0.0, dropout_seed=2025, l2_dnn=0.0):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = N = sparse_feature_number
        self.sparse_feature_dim = D = sparse_feature_dim
        self.dense_feature_dim = Dn = dense_feature_dim
        self.sparse_num_field = S = sparse_num_field
        self.layer_sizes = list(layer_sizes)
        self.dropout_rate, self.dropout_seed, self.l2_dnn = float(dropout_rate), int(dropout_seed), float(l2_dnn)
        self.num_fields = F = S + Dn                                         # net.py:31
        self.num_slices = F2 = F * F
        self.num_pairs = P = F * (F - 1) // 2
        self.input_size = P * D                                              # net.py:172-174
        self.row_width = R = F * D
        self.row_pad = _round_up(R, 4)
        self.ld_attn, self.ld_pair = _round_up(F2, 4), _round_up(max(P * D, 1), 4)
        std = 0.1 / math.sqrt(float(D))                                      # net.py:76-84 TruncatedNormal
        self.emb_table = torch.zeros(N, self.row_pad, dtype=torch.float32, device=self.device)
        self.embedding = self.emb_table[:, :R]
        torch.nn.init.trunc_normal_(self.embedding, 0.0, std, -2 * std, 2 * std)
        sizes = [self.input_size] + self.layer_sizes + [1]
        shapes = [("bias", (1,)), ("cen.dense_w", (1, Dn, R))]
        for name in (RED, ADD):                                              # reduction = 1: both are F2 x F2
            shapes += [(name + ".weight", (F2, F2)), (name + ".bias", (F2,))]
        for i in range(len(sizes) - 1):
            shapes += [("dnn.linear_%d.weight" % i, (sizes[i], sizes[i + 1])), ("dnn.linear_%d.bias" % i, (sizes[i + 1],))]
        self.dense = _FlatParams(shapes, self.device)
        p = self.dense.p
        p["cen.dense_w"].fill_(1.0)                                          # net.py:87-92 Constant(1.0)
        bound = math.sqrt(6.0 / (F2 + F2))                                   # paddle.nn.Linear default: XavierUniform
        for name in (RED, ADD):
            p[name + ".weight"].uniform_(-bound, bound)
        for i in range(len(sizes) - 1):
            p["dnn.linear_%d.weight" % i].normal_(0.0, 1.0 / math.sqrt(sizes[i]))   # net.py:189-190
        self.ws_bwd = self.k.Workspace(self.device)

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def state_dict(self):
        sd = {"cen.embedding.weight": self.embedding}
        sd.update(self.dense.p)
        return sd

    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            z = lambda: torch.zeros_like(self.emb_table)
            self.sparse_state = dict(m=z(), v=z())

    def _mat(self, name, B, cols, ld):
        """The [B, cols] view of the buffer `name`, whose rows are ld floats apart."""
        return self._buf(name, (B, ld))[:, :cols]

    def _cen_forward(self, ids, dense_inputs):
        """-> pooled, z1, a [B, F2] and H [B, P*D], y1 [B,1]."""
        k, p = self.k, self.dense.p
        B, D, F2 = ids.shape[0], self.sparse_feature_dim, self.num_slices
        pooled, _ = k.fatffm_pool_fwd(ids, dense_inputs, self.emb_table, p["cen.dense_w"], D, self.status,
                                      out=self._mat("_pooled", B, F2, self.ld_attn))
        z1 = k.gemm(pooled, p[RED + ".weight"], self.ws, epilogue="bias_relu", bias=p[RED + ".bias"],
                    out=self._mat("_z1", B, F2, self.ld_attn))
        a = k.gemm(z1, p[ADD + ".weight"], self.ws, epilogue="bias_relu", bias=p[ADD + ".bias"],
                   out=self._mat("_a", B, F2, self.ld_attn))
        H, y1, _ = k.fatffm_inter_fwd(ids, dense_inputs, self.emb_table, p["cen.dense_w"], a, D, self.status,
                                      out=(self._mat("_H", B, self.input_size, self.ld_pair), None))
        return pooled, z1, a, H, y1

    def forward(self, sparse_inputs, dense_inputs):
        ids = self._concat_ids(sparse_inputs)
        _, _, _, H, y1 = self._cen_forward(ids, dense_inputs)
        W, b, _, _ = self._linears("dnn.linear_%d", len(self.layer_sizes) + 1)
        y_dnn, _ = self.k.mlp_forward(H, W, b, self.ws)
        return torch.sigmoid(y1 + y_dnn + self.dense.p["bias"])

    __call__ = forward

    def _drop(self):
        return self.dropout_rate > 0.0

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, dense_inputs, label, lr=1e-4, auc_stats=None):
        """fat_deepffm/dygraph_model.py:77-93 + tools/trainer.py backward / step.  label [B,1] int64.
        Returns (loss [1] device tensor, pred [B,1])."""
        k, p, g = self.k, self.dense.p, self.dense.g
        ids = self._concat_ids(sparse_inputs)                      # net.py:108-109
        B, S = ids.shape
        D, Dn, R, F2 = self.sparse_feature_dim, self.dense_feature_dim, self.row_width, self.num_slices
        t, cur, side, groups = self._begin_step(B * S)
        pooled, z1, a, H, y1 = self._cen_forward(ids, dense_inputs)
        with _OnSide(side, cur):                                   # merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, None, self.ws_group, None, self.status, groups)
        # DNNLayer.forward (net.py:198-203): Dropout after every element of _mlp_layers; relu(drop(z)) = drop(relu(z)), so a
        # hidden layer is the GEMM's bias+ReLU epilogue followed by ONE dropout pass with two mask streams, and the last
        # Linear's [B,1] output is dropped too
        n = len(self.layer_sizes)
        W, b, dW, db = self._linears("dnn.linear_%d", n + 1)
        drop, rate, seed = self._drop(), self.dropout_rate, self.dropout_seed
        nstreams = 2 * n + 1
        base = t * nstreams
        acts, x = [], H
        for i in range(n):
            acts.append(x)
            x = k.gemm(x, W[i], self.ws, epilogue="bias_relu", bias=b[i])
            if drop:
                k.dropout(x, rate, seed, base + 2 * i, base + 2 * i + 1, step_stride=nstreams)
        acts.append(x)
        y_dnn = k.gemm(x, W[n], self.ws, epilogue="bias", bias=b[n])
        if drop:
            k.dropout(y_dnn, rate, seed, base + 2 * n, step_stride=nstreams)
        bias_col = p["bias"].expand(B, 1).contiguous()             # the logit's third term, one value per sample
        pred, dz, loss = k.sigmoid_logloss(y1, y_dnn, bias_col, label, self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        k.colsum(dz, self.ws, out=g["bias"])                       # d loss / d bias = sum_b dz[b]
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
                gy = k.gemm(gy, W[0], self.ws, trans_b=True, out=self._mat("_dH", B, self.input_size, self.ld_pair))
        dH = gy
        # backward of the CENet: d_a from the cube, the two Linear+ReLU, d_pooled back into the cube's gradient
        dense_w = p["cen.dense_w"]
        d_a, _ = k.fatffm_attn_bwd(ids, dense_inputs, self.emb_table, dense_w, a, dH, dz, D, self.status,
                                   out=self._mat("_d_a", B, F2, self.ld_attn))
        k.relu_mask_(d_a, a)
        k.gemm(z1, d_a, self.ws, trans_a=True, out=g[ADD + ".weight"], b_colsum=g[ADD + ".bias"])
        d_z1 = k.gemm(d_a, p[ADD + ".weight"], self.ws, trans_b=True, epilogue="relu_mask", aux0=z1,
                      out=self._mat("_d_z1", B, F2, self.ld_attn))
        k.gemm(pooled, d_z1, self.ws, trans_a=True, out=g[RED + ".weight"], b_colsum=g[RED + ".bias"])
        d_pooled = k.gemm(d_z1, p[RED + ".weight"], self.ws, trans_b=True, out=self._mat("_d_pooled", B, F2, self.ld_attn))
        row_grad, _, _ = k.fatffm_bwd(ids, dense_inputs, self.emb_table, dense_w, a, dH, dz, d_pooled, D, self.ws_bwd,
                                      out=(self._buf("_rg", (B * S, self.row_pad)), g["cen.dense_w"].view(Dn, R)),
                                      status=self.status)
        st = self.sparse_state
        self._update_rows(t, lr, cur, side, (groups, row_grad, 1, self.emb_table, st["m"], st["v"]))
        if self.l2_dnn:
            for i in range(n + 1):
                k.l2_decay_grad(dW[i].reshape(-1), W[i].reshape(-1), self.l2_dnn)
        self._finish_step(t, lr, cur, side)
        self._last = dict(row_grad=row_grad, dz=dz)
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """fat_deepffm/dygraph_model.py:22-113."""
    print_loss = True       # dygraph_model.py:92

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return FAT_DeepFFMLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                                g("hyper_parameters.dense_input_dim"),
                                g("hyper_parameters.sparse_inputs_slots") - 1,      # dygraph_model.py:24-36
                                g("hyper_parameters.layer_sizes_dnn"), device=device, kernels=kernels,
                                dropout_rate=0.5,                    # the DNN constructor's default (net.py:161), no YAML key
                                dropout_seed=g("runner.seed", 12345), l2_dnn=L2_DNN)
