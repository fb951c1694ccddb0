"""Host-side mirror of the reference's ESCM2 plugin (models/multitask/escm2/net.py:21-161 ESCMLayer, dygraph_model.py) on the
recengine HIP kernels: an MMoE trunk over the padded multi-field embedding sum-pool, with the entire-space losses and a
counterfactual CVR term in IPW or DR form.

The trunk is an mtl.py plan of one level: expert_num experts and gate_num gates read the pooled features (ONE packed
image, one GEMM), gate g's mixture feeds tower_g (ReLU) -> tower_out_g.  gate_num is 3 in the DR mode (ctr, cvr and the
imputation tower) and 2 otherwise, as net.py:35-38 decides it.  What differs from MMoE: rec_field_sumpool_fwd makes the
features, rec_esm_head replaces rec_mtl_head (MtlLayer._head), and level 0 also returns dX (MtlLayer.level0_dx), which
drives the table's non-lazy Adam (esm.py).  Kept as the reference writes it (QUIRKS)."""
import math

import torch

from .esm import EsmDygraphModel, EsmLoss, FieldTable, out_list
from .mtl import MtlLayer

QUIRKS = ("hyper_parameters.ctr_fc_sizes, cvr_fc_sizes and gate_num are read and ignored (net.py stores the first two and "
          "never uses them; gate_num is 3 when runner.counterfact_mode is DR and 2 otherwise, net.py:35-38); the softmax outputs "
          "are clipped to [1e-15, 1 - 1e-15] in float32, where the upper bound is 1; log_loss has epsilon 1e-4; the IPW "
          "propensity is 1 / max(pCTR * clicks in the batch, 1e-6) clipped to [-15, 15] and multiplied by the batch size, the "
          "DR one click / max(pCTR, 1e-6) clipped alike, both under stop-gradient; the reference's infer_forward unpacks "
          "seven outputs and therefore only runs in the DR mode, this one runs in both; Linear weights are XavierUniform "
          "with bias 0.1 (drawn with torch, not Paddle's random stream), the table Uniform(-1, 1) with row 0 zero; Adam "
          "(beta 0.9 / 0.999, epsilon 1e-8, non-lazy: every table row moves) at hyper_parameters.optimizer.learning_rate")

MODES = ("IPW", "DR")


def _xavier(t):
    lim = math.sqrt(6.0 / (t.shape[0] + t.shape[1]))
    t.uniform_(-lim, lim)


def escm2_plan(feature_size, expert_num, expert_size, tower_size, gate_num):
    """The mtl.py plan of ESCMLayer's trunk: the Linears in state_dict order (net.py:54-105)."""
    F, E, S, G, T = int(feature_size), int(expert_num), int(expert_size), int(gate_num), int(tower_size)
    if min(F, E, S, T) < 1:
        raise ValueError("ESCM2: feature_size, expert_num, expert_size and tower_size must be positive")
    params = [("expert_%d" % i, F, S, _xavier, 0.1) for i in range(E)]
    for i in range(G):
        params += [("gate_%d" % i, F, E, _xavier, 0.1), ("tower_%d" % i, S, T, _xavier, 0.1), ("tower_out_%d" % i, T, 2, _xavier, 0.1)]
    level = dict(slots=[("expert_%d" % i, 0) for i in range(E)], gates=[("gate_%d" % i, 0, (0, E, 0, 0)) for i in range(G)])
    return dict(params=params, aliases={}, levels=[level], n_inputs=1, tasks=G)


class ESCMLayer(MtlLayer):
    """escm2/net.py:21-161.  forward(ids [B, num_field, max_len] int64) -> net.py's out_list; train_step(ids, click [B],
    buy [B], lr) -> (loss, pred [B, 2G+2])."""

    def __init__(self, sparse_feature_number, sparse_feature_dim, num_field, ctr_layer_sizes, cvr_layer_sizes, expert_num,
                 expert_size, tower_size, counterfact_mode, feature_size, max_len=3, global_w=0.5, counterfactual_w=0.5,
                 device="cuda", kernels=None):
        if counterfact_mode not in MODES:
            raise ValueError("ESCM2: unknown runner.counterfact_mode %r (known: %s)" % (counterfact_mode, ", ".join(MODES)))
        if int(feature_size) != int(num_field) * int(sparse_feature_dim):
            raise ValueError("ESCM2: hyper_parameters.feature_size is %d but the pooled features are num_field * "
                             "sparse_feature_dim = %d * %d = %d wide (the reference fails in its first matmul)"
                             % (feature_size, num_field, sparse_feature_dim, int(num_field) * int(sparse_feature_dim)))
        self.counterfact_mode = counterfact_mode
        self.gate_num = self.n_tasks = 3 if counterfact_mode == "DR" else 2
        super().__init__(escm2_plan(feature_size, expert_num, expert_size, tower_size, self.gate_num), device, kernels)
        self.ctr_layer_sizes, self.cvr_layer_sizes = ctr_layer_sizes, cvr_layer_sizes          # stored, never used
        self.expert_num, self.expert_size, self.tower_size, self.feature_size = expert_num, expert_size, tower_size, feature_size
        self.global_w, self.counterfactual_w = float(global_w), float(counterfactual_w)
        self.emb = FieldTable(sparse_feature_number, sparse_feature_dim, num_field, max_len, self.device, self.k)
        self.level0_dx = True

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        sd = {"embedding.weight": self.emb.weight}
        sd.update(super().state_dict())
        return sd

    def parameters(self):
        return [self.emb.weight] + super().parameters()

    def _optimizer_views(self):
        return dict(super()._optimizer_views(), **self.emb.moment_views())

    # ---------------------------------------------------------------- forward
    def predict(self, ids):
        """-> pred [B, 2G+2]: every task's clipped softmax side by side, then (1 - pCTCVR, pCTCVR)."""
        z = self._run(self.emb.pool(ids, self.status))
        none = torch.zeros(z.shape[0], dtype=torch.int64, device=self.device)
        return self.k.esm_head(z, none, none, self.counterfact_mode, self.global_w, self.counterfactual_w, 1.0, want_grad=False)[0]

    def forward(self, ids):
        return out_list(self.predict(ids), self.n_tasks)

    __call__ = forward

    # ---------------------------------------------------------------- training
    def _head(self, z, label, B):
        click, buy = label
        return self.k.esm_head(z, click, buy, self.counterfact_mode, self.global_w, self.counterfactual_w, 1.0 / B)

    def _loss(self, cost):
        return EsmLoss(cost, self.global_w, self.counterfactual_w)

    def train_step(self, ids, click, buy, lr=1e-3):
        """dygraph_model.py train_forward + backward + Adam.  -> (loss: an EsmLoss, pred [B, 2G+2])."""
        x = self.emb.pool(ids, self.status)
        if tuple(click.shape) != (x.shape[0],) or tuple(buy.shape) != (x.shape[0],):
            raise ValueError("click and buy must be int64 [B], got %s and %s" % (tuple(click.shape), tuple(buy.shape)))
        loss, pred = super().train_step(x, (click, buy), lr)
        self._last["ids"] = ids
        self.emb.step(ids, self._last["dX"], self.step_count, lr, self.status)
        return loss, pred

    def last_gradients(self):
        g = super().last_gradients()
        g["embedding.weight"] = self.emb.dense_gradient(self._last["ids"], self._last["dX"])
        return g


class DygraphModel(EsmDygraphModel):
    """escm2/dygraph_model.py — same method names."""
    METRICS = (("auc_ctr", 0, 0), ("auc_cvr", 1, 1), ("auc_ctcvr", "ctcvr", 1))

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return ESCMLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                         g("hyper_parameters.num_field"), g("hyper_parameters.ctr_fc_sizes"), g("hyper_parameters.cvr_fc_sizes"),
                         g("hyper_parameters.expert_num"), g("hyper_parameters.expert_size"), g("hyper_parameters.tower_size"),
                         g("runner.counterfact_mode"), g("hyper_parameters.feature_size"),
                         max_len=g("hyper_parameters.max_len", 3), global_w=g("hyper_parameters.global_w", 0.5),
                         counterfactual_w=g("hyper_parameters.counterfactual_w", 0.5), device=device, kernels=kernels)
