"""What the host mirrors of the reference's entire-space multitask nets share (models/multitask/esmm, escm2: net.py,
dygraph_model.py, esmm_reader.py / escm_reader.py): the embedding table behind the padded multi-field sum-pool, the lazily
reduced loss and the DygraphModel.

  * the table is `embedding.weight` [sparse_feature_number, D], Uniform(-1, 1) with the padding row 0 zeroed, as
    nn.Embedding(padding_idx=0) leaves it.  Forward: rec_field_sumpool_fwd reads ids [B, F, L] and writes the [B, F*D]
    feature rows the first GEMM reads (no LoD, no [B, F, L, D] intermediate).  Backward: lookup i of the flattened ids takes
    row i // L of dX viewed as [B*F, D] (grad_div = L), so ids_group(padding_idx=0) -> segment_partials -> adam_rows_all is
    the reference's dygraph Adam on the dense table gradient: non-lazy, every row's moments decay each step, and row 0,
    whose gradient is always zero, never moves;
  * the head is rec_esm_head (ops.esm_head): predictions [B, 2G+2], cost [B, 3] and d(logits) in one pass, with
    dz0 = -dz1 exactly per task.  The loss mean(cost0) + counterfactual_w mean(cost1) + global_w mean(cost2) is only
    taken, with torch, when something reads it."""
import torch

from .mtl import ADAM_EPS, BETA1, BETA2, LazyLoss
from .net_base import auc_metrics, auc_update


class EsmLoss(LazyLoss):
    """The step's loss of cost [B, 3] (ctr, counterfactual cvr, ctcvr): reduced (torch) when it is read."""

    def __init__(self, cost, global_w, counterfactual_w):
        super().__init__(cost)
        self.global_w, self.counterfactual_w = float(global_w), float(counterfactual_w)

    def value(self):
        if self._v is None:
            m = self.cost.mean(0)
            self._v = (m[0] + self.counterfactual_w * m[1] + self.global_w * m[2]).reshape(1)
        return self._v


class FieldTable:
    """embedding.weight with Adam's moments: the pool forward and the table's step."""

    def __init__(self, num_rows, dim, num_field, max_len, device, kernels):
        self.k, self.device = kernels, torch.device(device)
        self.num_rows, self.dim, self.num_field, self.max_len = int(num_rows), int(dim), int(num_field), int(max_len)
        if min(self.num_rows, self.dim, self.num_field, self.max_len) < 1:
            raise ValueError("sparse_feature_number, sparse_feature_dim, num_field and max_len must be positive")
        self.weight = torch.empty(self.num_rows, self.dim, dtype=torch.float32, device=self.device).uniform_(-1.0, 1.0)
        self.weight[0].zero_()                                 # padding_idx = 0
        self.m, self.v = torch.zeros_like(self.weight), torch.zeros_like(self.weight)
        self.ws_group = self.k.Workspace(self.device)
        self.groups = self._pp = None

    def check_ids(self, ids):
        if ids.dim() != 3 or tuple(ids.shape[1:]) != (self.num_field, self.max_len) or ids.dtype != torch.int64:
            raise ValueError("expected ids int64 [B, %d, %d], got %s %s" % (self.num_field, self.max_len, ids.dtype,
                                                                          tuple(ids.shape)))

    def pool(self, ids, status, out=None):
        """-> [B, num_field * dim] features (written into `out`, a view with a row stride, when given)."""
        self.check_ids(ids)
        return self.k.field_sumpool_fwd(ids, self.weight, 0, out=out, status=status)[0]

    def step(self, ids, dX, step, lr, status):
        """Non-lazy Adam from dX [B, num_field * dim] (contiguous), the gradient of pool()'s output."""
        k, flat = self.k, ids.reshape(-1)
        if self.groups is None or self.groups.n != flat.numel():
            self.groups = k.IdGroups(flat.numel(), self.device)
        k.ids_group(flat, self.num_rows, 0, self.ws_group, None, status, self.groups)
        self._pp = k.segment_partials(self.groups, dX, self.dim, grad_div=self.max_len, out=self._pp)
        k.adam_rows_all(self.groups, dX, self.max_len, self.weight, self.m, self.v, step, lr, BETA1, BETA2, ADAM_EPS,
                        partials=self._pp)

    def dense_gradient(self, ids, dX):
        """The [num_rows, dim] gradient the reference's optimizer sees (torch; for inspection, not on the step's path)."""
        flat = ids.reshape(-1)
        keep = (flat > 0) & (flat < self.num_rows)
        rows = dX.reshape(-1, self.dim)[torch.arange(flat.numel(), device=flat.device)[keep] // self.max_len]
        return torch.zeros_like(self.weight).index_add_(0, flat[keep], rows)

    def moment_views(self):
        """The table's share of its layer's _optimizer_views."""
        return {"mtl.m.embedding.weight": self.m, "mtl.v.embedding.weight": self.v}


def out_list(pred, n_tasks):
    """net.py's return value from pred [B, 2G+2]: ctr_out, ctr_prop_one, cvr_out, cvr_prop_one, ctcvr_prop, ctcvr_prop_one
    (and imp_prop_one with three tasks) — column views."""
    G = int(n_tasks)
    out = [pred[:, 0:2], pred[:, 1:2], pred[:, 2:4], pred[:, 3:4], pred[:, 2 * G:2 * G + 2], pred[:, 2 * G + 1:2 * G + 2]]
    if G == 3:
        out.append(pred[:, 5:6])
    return out


class EsmDygraphModel:
    """esmm / escm2 dygraph_model.py — same method names; tensors are torch device tensors.  Subclasses give create_model
    and METRICS: [(name, prediction column of pred [B, 2G+2] with G = dy_model.n_tasks, label: 0 click / 1 buy)]."""
    METRICS = ()

    def create_feeds(self, batch_data, config, device="cuda"):
        """(ids [B, num_field, max_len], click [B], buy [B]) as reader.AliCCPReader yields them -> the same on `device`,
        int64 (the reference's 23 per-field tensors are the slices ids[:, f, :])."""
        ids, click, buy = (torch.as_tensor(b).to(device).to(torch.int64) for b in batch_data[:3])
        return ids.contiguous(), click.reshape(-1).contiguous(), buy.reshape(-1).contiguous()

    def create_metrics(self, device="cuda"):
        return auc_metrics(device, [n for n, _, _ in self.METRICS])

    def _auc(self, dy_model, metrics_list, pred, click, buy):
        G = dy_model.n_tasks
        for m, (_, col, which) in zip(metrics_list, self.METRICS):
            c = 2 * G + 1 if col == "ctcvr" else 2 * col + 1       # column 1 of the prediction
            auc_update(dy_model.k, m, pred[:, c], buy if which else click)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        ids, click, buy = self.create_feeds(batch_data, config, dy_model.device)
        loss, pred = dy_model.train_step(ids, click, buy, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        self._auc(dy_model, metrics_list, pred, click, buy)
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        ids, click, buy = self.create_feeds(batch_data, config, dy_model.device)
        self._auc(dy_model, metrics_list, dy_model.predict(ids), click, buy)
        return metrics_list, None
