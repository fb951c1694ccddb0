"""rank/dcn on the engine — Deep & Cross with the vector-form cross network on the HIP kernels of csrc/dcn_cross.hip.

Host mirror of the reference's models/rank/dcn/net.py (`DeepCroLayer`) and dcn/dygraph_model.py (`DygraphModel`):
    feat      = [embedding(ids) (S*D) | dense (Dn, raw: no dense_emb, no log1p)]            net.py:107-115
    s_l       = <x_l, layer_w>,  x_{l+1} = x_0 * s_l + layer_b + x_l   (x_0 = feat)         net.py:117-126
    l2        = sum_l sum_{b,k} (x_l[b,k] * layer_w[k])^2  — a sum over the batch           net.py:128-138
    predict   = sigmoid(fc([DNN(feat) | x_L]))                                              net.py:140-158
    loss      = mean log_loss(predict, label) + l2                                          dygraph_model.py:97-98
Quirks of the reference that are mirrored (the rank/dcn section):
  * ONE layer_w and ONE layer_b are shared by all cross_num layers; their gradients are sums over the layers;
  * the l2 term enters the loss with coefficient 1 and is NOT divided by the batch; `l2_reg_cross` and `clip_by_norm`
    are read from the config, stored on the layer and never used by the dygraph path;
  * fc.weight is drawn with std 1/sqrt(last_width + sparse_num_field + Dn): the field COUNT, not S*D (net.py:100-104);
  * the Embedding is sparse=True with padding_idx=0 whatever `is_sparse` says; the dygraph Adam is not lazy: every
    row's moments move each step (lazy_mode=False).  lazy_mode=True (an extension) touches only the batch's rows.
The table is the line-aligned record buffer of dcn_v2.py: rec [N, round_up(D, 32)], `embedding.weight` the [:, :D] view.
The feature rows and the fc input are kept at row strides rounded up to 4 floats, so the cross kernels move them as
16-byte vectors; rec_dcn_cross_fwd writes x_L straight into columns [H, H + d) of the fc input and rec_dcn_cross_bwd
ADDS d loss / d feat of the stack (and of the l2 term) into the DNN's layer-0 dX, taking its upstream gradient in the
rank-1 form dz[b] * fc.weight[H + k].  The only torch arithmetic of a step is plumbing: the [B, Dn] dense values copied
into the feature row and the two scalars of the reported loss added.  There is no autograd tape and no CPU fallback.
"""
import math

import torch

from .deepfm import _FlatParams
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up

L2_COEFF = 1.0      # dygraph_model.py:98: `create_loss(pred, label) + l2_loss`


class DeepCroLayer(SlotLayerBase):
    """dcn/net.py:21-158.  forward(sparse_inputs, dense_inputs) -> predict [B,1] (the reference also returns the l2
    term: forward_with_l2).  grad_dict()'s layer_w / layer_b are summed over the cross layers, the l2 term included."""
    lazy_mode = False   # the dygraph default; the trainer's hyper_parameters.optimizer.lazy_mode sets it

    def __init__(self, sparse_feature_number, sparse_feature_dim, dense_feature_dim, sparse_num_field, layer_sizes,
                 cross_num, clip_by_norm=None, l2_reg_cross=None, is_sparse=None, device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        self.sparse_feature_number = N = sparse_feature_number
        self.sparse_feature_dim = D = sparse_feature_dim
        self.dense_feature_dim = Dn = dense_feature_dim
        self.sparse_num_field = S = sparse_num_field
        self.layer_sizes = list(layer_sizes)
        self.cross_num = int(cross_num)
        self.clip_by_norm, self.l2_reg_cross, self.is_sparse = clip_by_norm, l2_reg_cross, is_sparse   # stored, unused
        if self.cross_num < 1 or not self.layer_sizes:
            raise ValueError("dcn needs cross_num >= 1 and at least one DNN layer")
        self.num_field = self.d = d = Dn + S * D                             # net.py:79 (a width, despite its name)
        self.d_pad = _round_up(d, 4)
        self.padding_idx = 0
        f32 = dict(dtype=torch.float32, device=self.device)
        self.rec = torch.zeros(N, _round_up(D, 32), **f32)
        self.embedding = self.rec[:, :D]
        std = 0.1 / math.sqrt(float(D))                                      # net.py:47-51,59-62,71-74 TruncatedNormal
        torch.nn.init.trunc_normal_(self.embedding, 0.0, std, -2 * std, 2 * std)
        self.embedding[0].zero_()
        sizes = [d] + self.layer_sizes
        shapes = [("layer_w", (d,)), ("layer_b", (d,))]
        for i in range(len(self.layer_sizes)):
            shapes += [("linear_%d.weight" % i, (sizes[i], sizes[i + 1])), ("linear_%d.bias" % i, (sizes[i + 1],))]
        H = self.layer_sizes[-1]
        shapes += [("fc.weight", (H + d, 1)), ("fc.bias", (1,))]
        self.dense = _FlatParams(shapes, self.device)
        p = self.dense.p
        for name in ("layer_w", "layer_b"):
            torch.nn.init.trunc_normal_(p[name], 0.0, std, -2 * std, 2 * std)
        for i in range(len(self.layer_sizes)):
            p["linear_%d.weight" % i].normal_(0.0, 1.0 / math.sqrt(sizes[i]))            # net.py:86-90
        p["fc.weight"].normal_(0.0, 1.0 / math.sqrt(H + S + Dn))                         # net.py:100-104
        self.ws_cross = self.k.Workspace(self.device)

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def state_dict(self):
        sd = {"embedding.weight": self.embedding}
        sd.update(self.dense.p)
        return sd

    # -- forward pieces ---------------------------------------------------------------------------
    def _feat(self, ids, dense_inputs):
        """net.py:107-115: the lookup written straight into the head of the feature row, the raw dense values behind
        it.  -> the [B, d] view of a [B, d_pad] buffer."""
        B, S = ids.shape
        D, d = self.sparse_feature_dim, self.d
        buf = torch.empty(B, self.d_pad, dtype=torch.float32, device=self.device)
        self.k.emb_gather(ids.reshape(-1), self.embedding, self.padding_idx, self.status, out=buf, out_group=S,
                          out_group_stride=self.d_pad)
        buf[:, S * D:d].copy_(dense_inputs)
        return buf[:, :d]

    def _logit(self, ids, dense_inputs, train):
        """-> (logit [B,1], l2 [1] or None, saved): the DNN tower into columns [0, H) of the fc input, the cross stack
        into [H, H + d) beside it, then the fc GEMM."""
        k, p = self.k, self.dense.p
        B = ids.shape[0]
        d, H = self.d, self.layer_sizes[-1]
        feat = self._feat(ids, dense_inputs)
        last_buf = torch.empty(B, _round_up(H + d, 4), dtype=torch.float32, device=self.device)
        last = last_buf[:, :H + d]
        W, b, _, _ = self._linears("linear_%d", len(self.layer_sizes))
        n = len(W)
        acts, x = [], feat
        for i in range(n):                                                   # net.py:147-148: Linear + ReLU each
            acts.append(x)
            x = k.gemm(x, W[i], self.ws, epilogue="bias_relu", bias=b[i], out=last[:, :H] if i == n - 1 else None)
        _, saved, l2 = k.dcn_cross_fwd(feat, p["layer_w"], p["layer_b"], self.cross_num, self.ws_cross,
                                       l2_coeff=L2_COEFF, want_saved=train, want_l2=train,
                                       out=(last[:, H:], None, None))
        logit = k.gemm(last, p["fc.weight"], self.ws, epilogue="bias", bias=p["fc.bias"])   # net.py:150-152
        return logit, l2, dict(feat=feat, acts=acts, last=last, saved=saved)

    def forward(self, sparse_inputs, dense_inputs):
        ids = self._concat_ids(sparse_inputs)                                # net.py:108
        logit, _, _ = self._logit(ids, dense_inputs, train=False)
        return torch.sigmoid(logit)                                          # net.py:154

    __call__ = forward

    def forward_with_l2(self, sparse_inputs, dense_inputs):
        """The reference's forward signature: (predict [B,1], l2_reg_cross_loss [1])."""
        ids = self._concat_ids(sparse_inputs)
        logit, l2, _ = self._logit(ids, dense_inputs, train=True)
        return torch.sigmoid(logit), l2

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, sparse_inputs, dense_inputs, label, lr=1e-3, auc_stats=None):
        """dcn/dygraph_model.py:91-107 + tools/trainer.py backward / step.  label [B,1] int64.
        Returns (loss [1] device tensor = mean log-loss + l2, pred [B,1]); the two addends stay in self.last_losses."""
        k, p, g = self.k, self.dense.p, self.dense.g
        ids = self._concat_ids(sparse_inputs)
        B, S = ids.shape
        d, H = self.d, self.layer_sizes[-1]
        t, cur, side, groups = self._begin_step(B * S)
        with _OnSide(side, cur):                                   # the merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, self.padding_idx, self.ws_group, None, self.status, groups)
        logit, l2, sv = self._logit(ids, dense_inputs, train=True)
        pred, dz, logloss = k.sigmoid_logloss(logit, None, None, label, self.ws)
        if auc_stats is not None:
            k.auc_histogram(pred, label, auc_stats[0], auc_stats[1], NUM_THRESHOLDS)
        self.last_losses = (logloss, l2)
        loss = logloss + l2                                        # dygraph_model.py:98
        # backward.  fc: dW / db over the whole [DNN | cross] input; its dX only for the DNN columns — the cross columns'
        # upstream gradient is dz[b] * fc.weight[H + k], which rec_dcn_cross_bwd forms in registers
        feat, acts, last = sv["feat"], sv["acts"], sv["last"]
        fcw = p["fc.weight"]
        k.gemm(last, dz, self.ws, trans_a=True, out=g["fc.weight"], b_colsum=g["fc.bias"])
        gy = k.gemm(dz, fcw[:H], self.ws, trans_b=True, epilogue="relu_mask", aux0=last[:, :H])
        W, _, dW, db = self._linears("linear_%d", len(self.layer_sizes))
        dfeat_buf = self._buf("_dfeat", (B, self.d_pad))
        dfeat = dfeat_buf[:, :d]
        for i in reversed(range(len(W))):
            gy = k.linear_backward(acts[i], gy, W[i], self.ws, dW[i], db[i], relu_src=acts[i] if i > 0 else None,
                                   out=dfeat if i == 0 else None)
        k.dcn_cross_bwd(feat, p["layer_w"], p["layer_b"], sv["saved"], None, self.ws_cross, l2_coeff=L2_COEFF,
                        accumulate=True, out=(dfeat, g["layer_w"], g["layer_b"]), dz=dz, u=fcw[H:].reshape(-1))
        st = self.sparse_state
        self._update_rows(t, lr, cur, side, (groups, dfeat_buf, 1, self.embedding, st["m"], st["v"]),
                          grad_group=S, grad_group_stride=self.d_pad)     # lookup (b, s) = dfeat[b, s*D : (s+1)*D]
        self._finish_step(t, lr, cur, side)
        self._last_dfeat = dfeat
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """dcn/dygraph_model.py:22-120."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return DeepCroLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                            g("hyper_parameters.dense_input_dim"), g("hyper_parameters.sparse_inputs_slots") - 1,
                            g("hyper_parameters.fc_sizes"), g("hyper_parameters.cross_num"),
                            g("hyper_parameters.clip_by_norm", None), g("hyper_parameters.l2_reg_cross", None),
                            g("hyper_parameters.is_sparse", None), device=device, kernels=kernels)
