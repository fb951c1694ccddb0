"""rank/fm on the engine — a sibling net that reuses the DeepFM kernels.

Host mirror of /root/reference/models/rank/fm/net.py (`FMLayer`, `FM`) and fm/dygraph_model.py (`DygraphModel`):
    predict = sigmoid(y_first_order + y_second_order + bias)                      net.py:31-38
with the FM block of net.py:90-124 = `rec_deepfm_fm_fwd` / `_bwd` (the same arithmetic as deepfm/net.py:105-139).
What differs from DeepFM (oracle/fm_ref.py): no DNN tower (the backward gets a zero d_feat_dnn), the scalar `bias`
IS part of the logit, the Embeddings have NO padding_idx (id 0 is an ordinary, trained row), and the dense weights
start at Constant(1.0).  Optimizer: Adam (dygraph_model.py:60-65), lazy rows by default as in deepfm.py.
There is no autograd tape and no CPU fallback.
"""
import torch

from .deepfm import FM, _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide


class FMLayer(SlotLayerBase):
    """fm/net.py:20-38.  forward(sparse_inputs, dense_inputs) -> predict [B,1]."""

    def __init__(self, sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field,
                 device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = sparse_feature_number
        self.sparse_feature_dim = sparse_feature_dim
        self.dense_feature_dim = dense_feature_dim
        self.sparse_num_field = sparse_num_field
        self.fm = FM(sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field, self.device,
                     None, zero_padding_row=False)
        self.fm.padding_idx = None                                           # net.py:55-73: no padding_idx
        D, Dn = sparse_feature_dim, dense_feature_dim
        self.dense = _FlatParams([("fm.dense_w_one", (Dn,)), ("fm.dense_w", (1, Dn, D)), ("bias", (1,))],
                                 self.device)
        self.dense.p["fm.dense_w_one"].fill_(1.0)                            # net.py:78-82 Constant(1.0)
        self.dense.p["fm.dense_w"].fill_(1.0)                                # net.py:84-88
        self.lazy_mode = True

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def state_dict(self):
        sd = {"fm.embedding_one.weight": self.fm.embedding_one, "fm.embedding.weight": self.fm.embedding}
        sd.update(self.dense.p)
        return sd

    def _fm_fwd(self, ids, dense_inputs):
        return self.k.deepfm_fm_fwd(ids, dense_inputs, self.fm.embedding, self.fm.embedding_one,
                                    self.dense.p["fm.dense_w"], self.dense.p["fm.dense_w_one"], None, None,
                                    self.status)

    def forward(self, sparse_inputs, dense_inputs):
        ids = self._concat_ids(sparse_inputs)
        y1, y2, _, _, _ = self._fm_fwd(ids, dense_inputs)
        return torch.sigmoid(y1 + y2 + self.dense.p["bias"])

    __call__ = forward

    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            D = self.sparse_feature_dim
            self.sparse_state = dict(self._packed_moments(self.fm.rec.shape[0], D),
                                     m1=self.fm.rec[:, D + 1:D + 2], v1=self.fm.rec[:, D + 2:D + 3])

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, dense_inputs, label, lr=1e-3, auc_stats=None):
        """fm/dygraph_model.py:74-88 + tools/trainer.py:148-152.  label [B,1] int64.
        Returns (loss [1] device tensor, pred [B,1])."""
        k = self.k
        ids = self._concat_ids(sparse_inputs)                      # net.py:92
        B, S = ids.shape
        D, Dn = self.sparse_feature_dim, self.dense_feature_dim
        t, cur, side, groups = self._begin_step(B * S)
        y1, y2, feat, sum_emb, _ = self._fm_fwd(ids, dense_inputs)
        with _OnSide(side, cur):                                   # merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, None, self.ws_group, None, self.status, groups)
        bias_col = self.dense.p["bias"].expand(B, 1).contiguous()  # the logit's third term, one value per sample
        pred, dz, loss = k.sigmoid_logloss(y1, y2, bias_col, label, self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        k.colsum(dz, self.ws, out=self.dense.g["bias"])            # d loss / d bias = sum_b dz[b]
        zero_dfeat = self._buf("_zero_dfeat", feat.shape, zero=True)          # no DNN tower: d_feat_dnn = 0
        row_grad, _, _ = k.deepfm_fm_bwd(
            dense_inputs, feat, sum_emb, zero_dfeat, dz, dz, S, self.ws,
            out=(self._buf("_rg", (B * S, D)), self.dense.g["fm.dense_w"].view(Dn, D), self.dense.g["fm.dense_w_one"]))
        st = self.sparse_state
        self._update_rows(t, lr, cur, side, (groups, row_grad, 1, self.fm.embedding, st["m"], st["v"]),
                          (groups, dz, S, self.fm.embedding_one, st["m1"], st["v1"]))
        self._finish_step(t, lr, cur, side)
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """fm/dygraph_model.py:23-100."""

    def create_model(self, config, device="cuda", kernels=None):
        return FMLayer(config.get("hyper_parameters.sparse_feature_number"),
                       config.get("hyper_parameters.sparse_feature_dim"),
                       config.get("hyper_parameters.dense_input_dim"),
                       config.get("hyper_parameters.sparse_inputs_slots") - 1, device=device, kernels=kernels)
