"""rank/autofis on the engine — AutoFIS's gated, batch-normalised pair term fused into the lookup (csrc/autofis_ops.hip),
its DNN on the engine's GEMM and Linear -> BatchNorm -> ReLU kernels, Adam on everything and SimpleGrda on the gate.

Host mirror of the reference's models/rank/autofis/net.py (`AutoDeepFMLayer`), optimizer.py (`SimpleGrda`),
dygraph_model.py (`DygraphModel`), metrics.py (`LogLoss`) and of the lr decay of its own trainer.py:
    xw = w_embeddings(ids) [B,S];  xv = v_embeddings(ids) [B,S,D]                                      net.py:78-80
    h  = xv.flatten(1) through depth x (Linear, BatchNorm, ReLU), then Linear(width -> 1)             net.py:82-89
    L[b,p] = <xv[b,c_p], xv[b,r_p]> over the kept pairs;  fm = (bn2(L) * mask).sum(-1)                 net.py:91-98
    pred = sigmoid(xw.sum(1) + fm + h) [B];  loss = mean binary_cross_entropy     net.py:101, dygraph_model.py:46-48
Quirks of the reference that are mirrored (AutoFIS):
  * two stages.  Stage 0 keeps all S (S - 1) / 2 pairs and trains `mask` with SimpleGrda(lr 1, c = grad_c, mu = grad_mu)
    while Adam trains everything else; the trainer then writes comb_mask.npy = (mask != 0).  Stage 1 keeps the pairs with
    comb_mask == 1 (mask and bn2 shrink to them) and runs Adam on everything, mask included;
  * SimpleGrda's accumulator starts at U(-0.1, 0.1), not at zero, and takes `+ p` on its first step only;
  * both tables are plain nn.Embedding without a padding row (id 0 trains) and with a DENSE gradient, so Adam is the
    non-lazy form: every row of both tables moves every step;
  * the initialisers are Uniform +-sqrt(6 / sum(shape)) with shape [input_size] for w, [input_size, D] for v and [in, out]
    for the Linears; mask starts at U(0.599, 0.601);
  * nn.BatchNorm (momentum 0.9, eps 1e-5, biased variance); no dropout; use_bn is always True (create_model never
    passes it): use_bn=False raises NotImplementedError;
  * the lr decays by `gamma` before batch b whenever (b + 1) % (len(loader) // 5) == 0 and carries across epochs
    (trainer.py:108-116); with fewer than 5 batches the reference divides by zero — here the lr stays constant.
The tables are ONE line-aligned record buffer rec [N, round_up(D + 3, 32)] = v (D) | w | m1 | v1 | zeros; v's moments are
the packed mv buffer of the other slot nets.  mask sits LAST in the flat dense buffer: stage 0 runs Adam on the floats in
front of it and rec_grda_step on it.  The only torch arithmetic of a step is plumbing: the label's cast to float32 and the
log-loss metric's running sum.  There is no autograd tape and no CPU fallback.
"""
import itertools
import logging
import math

import numpy as np
import torch

from .deepfm import _FlatParams, auc_from_buckets
from .slot_net import NUM_THRESHOLDS, SlotDygraphModel, SlotLayerBase, _OnSide, _round_up, auc_metrics

logger = logging.getLogger("paddlerec_amd.autofis")

MASK, WEMB, VEMB = "mask", "w_embeddings.weight", "v_embeddings.weight"
LIN, BN, BN2 = "linear.%d", "bn.%d", "bn2"
BN_MOMENTUM, BN_EPS = 0.9, 1e-5
GRDA_LR = 1.0                                       # dygraph_model.py:66: SimpleGrda(mask_params, 1, grad_c, grad_mu)


def generate_pairs(num_inputs, comb_mask=None):
    """net.py:29-38 -> (cols, rows) of the pairs kept by comb_mask (None: all), in itertools.combinations order."""
    kept = [pr for i, pr in enumerate(itertools.combinations(range(num_inputs), 2))
            if comb_mask is None or int(comb_mask[i]) == 1]
    return [a for a, _ in kept], [b for _, b in kept]


class StepDecay:
    """The lr rule of autofis/trainer.py:106-116: decay_steps = len(loader) // 5; before batch `batch_id` runs the lr is
    multiplied by gamma when (batch_id + 1) % decay_steps == 0; the lr carries across epochs.  With fewer than 5 batches
    the reference divides by zero: the lr stays constant here (one log line says so)."""

    def __init__(self, lr, gamma, num_batches):
        self.lr, self.gamma, self.decay_steps = float(lr), float(gamma), int(num_batches) // 5
        if self.decay_steps == 0:
            logger.info("autofis: %d batches per epoch, fewer than 5: decay_steps = len(loader) // 5 is 0 (the reference "
                        "divides by zero here); the learning rate stays constant at %g", int(num_batches), self.lr)

    def before_batch(self, batch_id):
        if self.decay_steps and (batch_id + 1) % self.decay_steps == 0:
            self.lr *= self.gamma
        return self.lr


class AutoDeepFMLayer(SlotLayerBase):
    """autofis/net.py:41-101.  forward(ids [B,S]) -> pred [B] (eval mode: running statistics)."""

    def __init__(self, num_inputs, input_size, embedding_size, width, depth, pairs, stage, use_bn=True, comb_mask=None,
                 grad_c=0.0005, grad_mu=0.8, device="cuda", kernels=None):
        if not use_bn:
            raise NotImplementedError("AutoDeepFMLayer(use_bn=False): the reference's create_model never builds it")
        self._init_runtime(device, kernels)
        self.num_inputs = S = int(num_inputs)
        self.sparse_feature_number = N = int(input_size)
        self.sparse_feature_dim = D = int(embedding_size)
        self.width, self.depth, self.stage = int(width), int(depth), int(stage)
        self.grad_c, self.grad_mu = float(grad_c), float(grad_mu)
        self.lazy_mode = False                                               # dense gradients: every row moves
        if self.stage not in (0, 1):
            raise ValueError("stage must be 0 or 1, got %r" % (stage,))
        if self.depth < 1:
            raise ValueError("depth must be >= 1")
        n_all = S * (S - 1) // 2
        if self.stage == 0:
            if comb_mask is not None:
                raise ValueError("stage 0 keeps every pair: comb_mask belongs to stage 1")
            if int(pairs) != n_all:                                          # net.py:71-76: mask [1, pairs] against all pairs
                raise ValueError("pairs = %d, but %d inputs have %d pairs" % (int(pairs), S, n_all))
            self.comb_mask = None
        else:
            if comb_mask is None:
                raise ValueError("stage 1 needs comb_mask (stage 0 writes comb_mask.npy)")
            self.comb_mask = np.asarray(comb_mask).reshape(-1).astype(np.int64)
            if len(self.comb_mask) != n_all:
                raise ValueError("comb_mask has %d entries, %d inputs have %d pairs" % (len(self.comb_mask), S, n_all))
        cols, rows = generate_pairs(S, self.comb_mask)
        self.num_pairs = P = len(cols)
        if P == 0:
            raise ValueError("stage 0 kept no interaction: comb_mask is all zero")
        self.pairs = self.k.AutofisPairs(cols, rows, S, self.device)
        self.ld_x0, self.ld_l = _round_up(S * D, 4), _round_up(P, 4)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.rec = torch.zeros(N, _round_up(D + 3, 32), **f32)               # v | w | m1 | v1 | zeros
        self.v_embeddings, self.w_embeddings = self.rec[:, :D], self.rec[:, D:D + 1]
        uniform = lambda t, *shape: t.uniform_(-math.sqrt(6.0 / sum(shape)), math.sqrt(6.0 / sum(shape)))
        uniform(self.w_embeddings, N)                                        # net.py:56-57: xavier_init([input_size])
        uniform(self.v_embeddings, N, D)
        sizes = [S * D] + [self.width] * self.depth + [1]
        shapes = []
        for i in range(self.depth + 1):
            shapes += [(LIN % i + ".weight", (sizes[i], sizes[i + 1])), (LIN % i + ".bias", (sizes[i + 1],))]
        for i in range(self.depth):
            shapes += [(BN % i + ".weight", (self.width,)), (BN % i + ".bias", (self.width,))]
        shapes += [(BN2 + ".weight", (P,)), (BN2 + ".bias", (P,)), (MASK, (1, P))]      # mask LAST: GRDA's tail
        self.dense = _FlatParams(shapes, self.device)
        self.n_adam = self.dense.offsets[MASK]
        p = self.dense.p
        self.buffers = {}
        for i in range(self.depth + 1):
            uniform(p[LIN % i + ".weight"], sizes[i], sizes[i + 1])
        for name, n in [(BN % i, self.width) for i in range(self.depth)] + [(BN2, P)]:
            p[name + ".weight"].fill_(1.0)
            self.buffers[name + "._mean"] = torch.zeros(n, **f32)
            self.buffers[name + "._variance"] = torch.ones(n, **f32)
        p[MASK].uniform_(0.6 - 0.001, 0.6 + 0.001)
        self.grda_acc = self.grda_iterations = self.grda_l1 = None
        if self.stage == 0:                                                  # optimizer.py:27-35
            self.grda_acc = torch.empty(P, **f32).uniform_(-0.1, 0.1)
            self.grda_iterations, self.grda_l1 = 0, 0.0
        self.ws_bn = self.k.Workspace(self.device)
        self.ws_fis = self.k.Workspace(self.device)

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def state_dict(self):
        sd = {WEMB: self.w_embeddings, VEMB: self.v_embeddings}
        sd.update(self.dense.p)
        sd.update(self.buffers)
        return sd

    def parameters(self):
        return [self.w_embeddings, self.v_embeddings] + list(self.dense.p.values())

    # -- the optimizer state beyond Adam's: SimpleGrda's accumulator and counters ------------------
    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            D = self.sparse_feature_dim
            st = self._packed_moments(self.rec.shape[0], D)
            st.update(m1=self.rec[:, D + 1:D + 2], v1=self.rec[:, D + 2:D + 3])
            self.sparse_state = st

    def extra_optimizer_state(self):
        if self.stage != 0:
            return {}
        return {"grda.acc": self.grda_acc.detach().cpu().numpy().copy(),
                "grda.iterations": int(self.grda_iterations), "grda.l1_accumulation": float(self.grda_l1)}

    def set_extra_optimizer_state(self, st):
        if self.stage == 0 and "grda.acc" in st:
            self.grda_acc.copy_(torch.as_tensor(st["grda.acc"]).to(self.device).reshape(-1))
            self.grda_iterations, self.grda_l1 = int(st["grda.iterations"]), float(st["grda.l1_accumulation"])

    def _grda_step(self):
        """optimizer.py:39-60 with lr 1; iterations and l1_accumulation stay host numbers, the reference's expression."""
        c, mu, lr, it = self.grad_c, self.grad_mu, GRDA_LR, self.grda_iterations
        self.grda_l1 += c * math.pow(lr, (0.5 + mu)) * math.pow(it + 1., mu) \
            - c * math.pow(lr, (0.5 + mu)) * math.pow(it + 0., mu)
        self.k.grda_step(self.dense.p[MASK].view(-1), self.grda_acc, self.dense.g[MASK].view(-1), lr, self.grda_l1,
                         max(1 - it, 0))
        self.grda_iterations = it + 1

    def comb_mask_of_mask(self):
        """(mask != 0).astype(int) — what the reference's trainer saves after stage 0 (trainer.py:219-222)."""
        return (self.dense.p[MASK].detach().reshape(-1).cpu().numpy() != 0).astype(int)

    # -- forward ------------------------------------------------------------------------------------
    def _ids(self, inputs):
        ids = self._concat_ids(inputs)
        if ids.dim() != 2 or ids.shape[1] != self.num_inputs:
            raise ValueError("autofis takes ids [B, %d], got %s" % (self.num_inputs, tuple(ids.shape)))
        return ids.contiguous()

    def _logit(self, ids, training):
        """-> (logit [B,1], saved)."""
        k, p, bf = self.k, self.dense.p, self.buffers
        B, S = ids.shape
        D, P, n = self.sparse_feature_dim, self.num_pairs, self.depth
        out = (self._buf("_x0", (B, self.ld_x0))[:, :S * D], self._buf("_L", (B, self.ld_l))[:, :P] if training else None)
        X0, s, L, mean, invstd, _ = k.autofis_fwd(ids, self.v_embeddings, self.w_embeddings, self.pairs, p[BN2 + ".weight"],
                                                  p[BN2 + ".bias"], p[MASK].view(-1), bf[BN2 + "._mean"],
                                                  bf[BN2 + "._variance"], self.ws_fis, training, BN_MOMENTUM, BN_EPS,
                                                  status=self.status, out=out)
        W, b, _, _ = self._linears(LIN, n + 1)
        x, cache = X0, []
        for i in range(n):
            z = k.gemm(x, W[i], self.ws, epilogue="bias", bias=b[i])
            y, mu, istd = k.batchnorm_relu_fwd(z, p[BN % i + ".weight"], p[BN % i + ".bias"], bf[BN % i + "._mean"],
                                               bf[BN % i + "._variance"], self.ws_bn, training, BN_MOMENTUM, BN_EPS)
            cache.append((x, z, y, mu, istd))
            x = y
        # l + fm + h (net.py:101): the pair kernel's s rides the last GEMM's epilogue
        logit = k.gemm(x, W[n], self.ws, epilogue="add", aux1=s.view(B, 1), bias=b[n])
        return logit, dict(X0=X0, L=L, mean=mean, invstd=invstd, cache=cache, x=x)

    def forward(self, inputs):
        logit, _ = self._logit(self._ids(inputs), False)
        return torch.sigmoid(logit).reshape(-1)                                      # net.py:101

    __call__ = forward

    def eval_loss(self, inputs, label):
        """Eval-mode (pred [B,1], mean binary cross entropy [1])."""
        logit, _ = self._logit(self._ids(inputs), False)
        pred, _, loss = self.k.bce_with_logits(logit, label.to(torch.float32).reshape(-1, 1).contiguous(), self.ws)
        return pred, loss

    def log_loss_update(self, logit, label, metric):
        """metrics.py:22-30: metric = (running sum of the batch means of F.log_loss (epsilon 1e-4), batch count), on the
        device; read back only when printed."""
        z = self._buf("_zeros", (logit.shape[0], 1), zero=True)
        _, _, ll = self.k.sigmoid_logloss(logit, z, z, label.reshape(-1, 1).to(torch.int64).contiguous(), self.ws,
                                          eps=1e-4, want_dz=False)
        metric[0].add_(ll.reshape(-1))
        metric[1].add_(1)

    # -- one full training step: train_forward + backward + optimizer.step ----------------------
    def train_step(self, inputs, label, lr=1e-3, metrics=None):
        """dygraph_model.py:82-95 + trainer.py:120-128.  label [B] or [B,1] int64.  metrics: None or
        [auc buckets, log-loss metric].  Returns (loss [1] device tensor = mean binary cross entropy, pred [B,1])."""
        k, p, g = self.k, self.dense.p, self.dense.g
        ids = self._ids(inputs)
        B, S = ids.shape
        D, n = self.sparse_feature_dim, self.depth
        t, cur, side, groups = self._begin_step(B * S)
        with _OnSide(side, cur):                                   # the merge keys depend on the ids only
            k.ids_group(ids, self.sparse_feature_number, None, self.ws_group, None, self.status, groups)
        logit, sv = self._logit(ids, True)
        label = label.reshape(-1, 1)
        # sigmoid + F.binary_cross_entropy = BCE with logits wherever sigmoid(logit) is not exactly 0 or 1 in float32
        pred, dz, loss = k.bce_with_logits(logit, label.to(torch.float32).contiguous(), self.ws)
        if metrics:
            k.auc_histogram(pred, label.to(torch.int64).contiguous(), metrics[0][0], metrics[0][1], NUM_THRESHOLDS)
            if len(metrics) > 1:
                self.log_loss_update(logit, label, metrics[1])
        W, _, dW, db = self._linears(LIN, n + 1)
        k.gemm(sv["x"], dz, self.ws, trans_a=True, out=dW[n], b_colsum=db[n])
        dx = k.gemm(dz, W[n], self.ws, trans_b=True)
        dx0_buf = self._buf("_dx0", (B, self.ld_x0))
        for i in reversed(range(n)):
            x, z, y, mu, istd = sv["cache"][i]
            dz_i, _, _ = k.batchnorm_relu_bwd(z, y, dx, p[BN % i + ".weight"], mu, istd, self.ws_bn,
                                              dgamma=g[BN % i + ".weight"], dbeta=g[BN % i + ".bias"])
            dx = k.linear_backward(x, dz_i, W[i], self.ws, dW[i], db[i], out=dx0_buf[:, :S * D] if i == 0 else None)
        # the pair term's gradient lands on top of the DNN's layer-0 dX; d s / d (l + fm) = dz
        k.autofis_bwd(dz, sv["L"], sv["X0"], self.pairs, sv["mean"], sv["invstd"], p[BN2 + ".weight"], p[BN2 + ".bias"],
                      p[MASK].view(-1), dx, self.ws_fis, out=(g[MASK].view(-1), g[BN2 + ".weight"], g[BN2 + ".bias"]))
        st = self.sparse_state
        with _OnSide(side, cur):                                   # non-lazy Adam: both tables, every row
            lay = dict(grad_group=S, grad_group_stride=self.ld_x0)  # lookup (b, s) = dx0[b, s*D : (s+1)*D]
            self._pp = k.segment_partials(groups, dx0_buf, D, out=getattr(self, "_pp", None), **lay)
            self._pp1 = k.segment_partials(groups, dz, 1, grad_div=S, out=getattr(self, "_pp1", None))
            k.adam_rows_all(groups, dx0_buf, 1, self.v_embeddings, st["m"], st["v"], t, lr, partials=self._pp, **lay)
            k.adam_rows_all(groups, dz, S, self.w_embeddings, st["m1"], st["v1"], t, lr, partials=self._pp1)
        if self.stage == 0:
            self._finish_step(t, lr, cur, side, n_adam=self.n_adam)
            self._grda_step()
        else:
            self._finish_step(t, lr, cur, side)
        self._last = dict(row_grad=dx, dz=dz)
        return loss, pred


class DygraphModel(SlotDygraphModel):
    """autofis/dygraph_model.py:25-110."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        stage = int(g("stage", 0))
        comb_mask = None
        if stage == 1:                                                   # net.py:70: np.load('comb_mask.npy')
            comb_mask = np.load(g("runner.comb_mask_path") or "comb_mask.npy")
        return AutoDeepFMLayer(g("hyper_parameters.num_inputs"), g("hyper_parameters.input_size"),
                               g("hyper_parameters.embedding_size"), g("hyper_parameters.width"),
                               g("hyper_parameters.depth"), g("hyper_parameters.pairs"), stage, comb_mask=comb_mask,
                               grad_c=g("hyper_parameters.grad_c", 0.0005), grad_mu=g("hyper_parameters.grad_mu", 0.8),
                               device=device, kernels=kernels)

    def create_feeds(self, batch_data, config, device="cuda"):
        """-> (label [B,1] i64, ids [B,S]).  batch_data: the reference's (x [B,S], y [B]) pair (criteo_reader.py:31-32)
        or the (label [B,1], ids [B,S]) device tensors of paddlerec_amd.reader.AutofisReader."""
        a, b = batch_data
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        if a.dim() == 2 and a.shape[1] > 1:
            a, b = b, a
        return a.to(torch.int64).reshape(-1, 1).to(device), b.to(torch.int64).to(device)

    def create_metrics(self, device="cuda"):
        """dygraph_model.py:74-79: ["auc", "log_loss"]; the log loss is (sum of batch means [1] f32, batches [1] i64)."""
        stats, _ = auc_metrics(device)
        ll = (torch.zeros(1, dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.int64, device=device))
        return stats + [ll], ["auc", "log_loss"]

    @staticmethod
    def metric_value(name, m):
        if name == "log_loss":                                           # metrics.py:40-44
            n = int(m[1].item())
            return float(m[0].item()) / n if n else 0.0
        return auc_from_buckets(m[0], m[1])

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        label, ids = self.create_feeds(batch_data, config, dy_model.device)
        lr = getattr(dy_model, "lr", None)                               # the trainer's step decay (StepDecay)
        if lr is None:
            lr = config.get("hyper_parameters.optimizer.learning_rate", 0.001)
        loss, _ = dy_model.train_step(ids, label, lr, metrics_list)
        return loss, metrics_list, {"loss": loss}                        # dygraph_model.py:94

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        label, ids = self.create_feeds(batch_data, config, dy_model.device)
        logit, _ = dy_model._logit(dy_model._ids(ids), False)
        if metrics_list:
            pred = torch.sigmoid(logit)
            dy_model.k.auc_histogram(pred.contiguous(), label.contiguous(), metrics_list[0][0], metrics_list[0][1],
                                     NUM_THRESHOLDS)
            if len(metrics_list) > 1:
                dy_model.log_loss_update(logit, label, metrics_list[1])
        return metrics_list, None
