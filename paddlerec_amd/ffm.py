"""rank/ffm on the engine — the field-aware factorisation machine on the HIP kernels of csrc/ffm_ops.hip.

Host mirror of the reference's models/rank/ffm/net.py (`FFMLayer`, `FFM`) and ffm/dygraph_model.py (`DygraphModel`):
    predict = sigmoid(y_first_order + y_field_aware_second_order + bias)            net.py:39-46
    y_first_order = sum_s W1[id_s] + sum_k dense_k * dense_w_one[k]                  net.py:101-108
    y_second_order = sum_{i<j} <E[i, j, :], E[j, i, :]>                              net.py:110-132
over the F = S + Dn fields of a sample, each an R = F*D wide row: W[id_s] or dense_k * dense_w[k] (rec_ffm_fwd).
The Embeddings have NO padding_idx (id 0 is an ordinary, trained row) and the dense weights start at Constant(1.0).
Optimizer: paddle.optimizer.Adam (dygraph_model.py:56-61), lazy_mode=False unless the trainer switches it.
The table is kept at a padded row width Rp = round_up(R, 4) (352 for the reference's 351) so that its rows load as
16-byte vectors; `ffm.embedding.weight` is the [:, :R] view.  The backward writes 0 into the pad column and Adam moves
a zero-gradient, zero-moment element by exactly 0, so the pad stays 0 under both Adam forms.
There is no autograd tape and no CPU fallback.
"""
import math

import torch

from .deepfm import _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up


class FFMLayer(SlotLayerBase):
    """ffm/net.py:21-46.  forward(sparse_inputs, dense_inputs) -> predict [B,1]."""
    lazy_mode = False   # the dygraph default; the trainer's hyper_parameters.optimizer.lazy_mode sets it

    def __init__(self, sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field,
                 device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = sparse_feature_number
        self.sparse_feature_dim = sparse_feature_dim
        self.dense_feature_dim = dense_feature_dim
        self.sparse_num_field = sparse_num_field                             # F = sparse slots + dense fields
        N, D, Dn, F = sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field
        if F <= Dn:
            raise ValueError("sparse_num_field %d must exceed dense_feature_dim %d" % (F, Dn))
        R = F * D
        self.row_width = R
        self.row_pad = _round_up(R, 4)
        std = 0.1 / math.sqrt(float(D))                                      # net.py:59-75 TruncatedNormal
        # (not `table`: checkpoint.py reads a `table` attribute as a PS accessor table)
        self.emb_table = torch.zeros(N, self.row_pad, dtype=torch.float32, device=self.device)
        self.embedding = self.emb_table[:, :R]
        self.embedding_one = torch.zeros(N, 1, dtype=torch.float32, device=self.device)
        for t in (self.embedding_one, self.embedding):
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std)
        self.dense = _FlatParams([("ffm.dense_w_one", (Dn,)), ("ffm.dense_w", (1, Dn, R)), ("bias", (1,))],
                                 self.device)
        self.dense.p["ffm.dense_w_one"].fill_(1.0)                           # net.py:78-82 Constant(1.0)
        self.dense.p["ffm.dense_w"].fill_(1.0)                               # net.py:84-91
        self.ws_bwd = self.k.Workspace(self.device)

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def state_dict(self):
        sd = {"ffm.embedding_one.weight": self.embedding_one, "ffm.embedding.weight": self.embedding}
        sd.update(self.dense.p)
        return sd

    def _fwd(self, ids, dense_inputs):
        return self.k.ffm_fwd(ids, dense_inputs, self.emb_table, self.embedding_one, self.dense.p["ffm.dense_w"],
                              self.dense.p["ffm.dense_w_one"], self.sparse_feature_dim, self.status)

    def forward(self, sparse_inputs, dense_inputs):
        ids = self._concat_ids(sparse_inputs)
        y1, y2, _ = self._fwd(ids, dense_inputs)
        return torch.sigmoid(y1 + y2 + self.dense.p["bias"])

    __call__ = forward

    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            self.sparse_state = self._separate_moments(*self.emb_table.shape)

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, dense_inputs, label, lr=1e-3, auc_stats=None):
        """ffm/dygraph_model.py:69-84 + tools/trainer.py:148-152.  label [B,1] int64.
        Returns (loss [1] device tensor, pred [B,1])."""
        k = self.k
        ids = self._concat_ids(sparse_inputs)                      # net.py:94
        B, S = ids.shape
        D, Dn, R = self.sparse_feature_dim, self.dense_feature_dim, self.row_width
        t, cur, side, groups = self._begin_step(B * S)
        y1, y2, _ = self._fwd(ids, dense_inputs)
        with _OnSide(side, cur):                                   # merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, None, self.ws_group, None, self.status, groups)
        bias_col = self.dense.p["bias"].expand(B, 1).contiguous()  # the logit's third term, one value per sample
        pred, dz, loss = k.sigmoid_logloss(y1, y2, bias_col, label, self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        k.colsum(dz, self.ws, out=self.dense.g["bias"])            # d loss / d bias = sum_b dz[b]
        row_grad, _, _ = k.ffm_bwd(
            ids, dense_inputs, self.emb_table, self.dense.p["ffm.dense_w"], dz, D, self.ws_bwd,
            out=(self._buf("_rg", (B * S, self.row_pad)), self.dense.g["ffm.dense_w"].view(Dn, R),
                 self.dense.g["ffm.dense_w_one"]),
            status=self.status)
        st = self.sparse_state
        self._update_rows(t, lr, cur, side, (groups, row_grad, 1, self.emb_table, st["m"], st["v"]),
                          (groups, dz, S, self.embedding_one, st["m1"], st["v1"]))
        self._finish_step(t, lr, cur, side)
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """ffm/dygraph_model.py:20-99."""

    def create_model(self, config, device="cuda", kernels=None):
        dense_dim = config.get("hyper_parameters.dense_input_dim")
        return FFMLayer(config.get("hyper_parameters.sparse_feature_number"),
                        config.get("hyper_parameters.sparse_feature_dim"), dense_dim,
                        config.get("hyper_parameters.sparse_inputs_slots") - 1 + dense_dim,   # dygraph_model.py:31-32
                        device=device, kernels=kernels)
