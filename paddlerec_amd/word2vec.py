"""Host-side mirror of the reference's word2vec plugin (models/recall/word2vec/net.py:21-110 Word2VecLayer,
Word2VecInferLayer; dygraph_model.py; infer.py:62-69,129-146) on the recengine HIP kernels: skip-gram with negative
sampling — three tables, lookups, dots and row updates, no MLP.

  * rec_w2v_sgns_fwd_bwd: the input row, the 1 + neg target rows and biases, the logits, sigmoid then BCE on probabilities,
    g = d loss / d logit [B, 1 + neg] and d_in = sum_j g_j emb_w[target_j] [B, D] in one launch, the loss folded behind it;
  * rec_ids_group over target_ids, then rec_w2v_target_update: embedding_w / embedding_b rows step by SGD from g and the
    input table as it was BEFORE its own step — the [B, 1 + neg, D] gradient of the target rows is never written;
  * the input table's step is the engine's existing path: rec_ids_group over in_ids, the segment partials and
    rec_sparse_sgd_rows over d_in.  The order on the stream is fwd_bwd, target_update, input-row SGD;
  * infer: rec_w2v_analogy_topk normalises, scores and selects without the [B, V] matrix; the first-of-four-that-is-no-
    input rule and acc are counted on the host.
Names are the reference's: embedding.weight, embedding_w.weight, embedding_b.weight [V, 1]."""
import numpy as np
import torch

from .net_base import LayerBase

QUIRKS = ("the loss is binary_cross_entropy(sigmoid(true), 1) + binary_cross_entropy(sigmoid(neg), 0), each with its default "
          "MEAN reduction (dygraph_model.py:60-66): the true term is averaged over B and the negative term over B * neg — a "
          "mean of means, not a mean over B (1 + neg) — and the trailing paddle.mean of a scalar changes nothing; it is two "
          "stages, a sigmoid and then a BCE on probabilities, not BCE-with-logits: the log is clamped at -100 and the "
          "backward divides by max((1 - x) x, 1e-12), so a saturated float32 sigmoid gives a loss term of 100 and a gradient "
          "of exactly 0; there is no padding id, id 0 is an ordinary word; embedding_w and embedding_b start at zero, "
          "embedding at Uniform(+-0.5 / emb_dim); plain SGD on all three tables, no metric in the train loop; the reader's "
          "window is ONE draw — np.random.seed(12345); np.random.randint(1, window_size + 1) at construction "
          "(word2vec_reader.py:60-61), 3 for window_size 5 — used for every word; random.seed(12345) runs before EVERY "
          "sample's negatives (word2vec_reader.py:113-116), so every sample of every batch gets the same neg_num ids: the "
          "negative rows are neg_num hot rows with B occurrences each; infer re-normalises every vocabulary row by "
          "max(|row|, 1e-12) but not the query b - a + c, takes the top 4 and compares the first of them that is not one of "
          "the three input words with the label (none left: a miss); the infer reader stops at the first line that holds a "
          "':'; only embedding.weight matters to infer; the learning-rate decay keys are read by the static model only")


class Word2VecLayer(LayerBase):
    """net.py:21-81.  train_step(in_ids [B], target_ids [B, 1 + neg], lr) -> (loss [1], true_logits [B], neg_logits [B, neg])."""

    def __init__(self, sparse_feature_number, emb_dim, neg_num, emb_name="emb", emb_w_name="emb_w", emb_b_name="emb_b",
                 device="cuda", kernels=None):
        from ._lib import REC_W2V_MAX_DIM, REC_W2V_MAX_NEG
        self._init_runtime(device, kernels, group_status=True)   # the groupings' own word (the forward has flagged already)
        self.sparse_feature_number, self.emb_dim, self.neg_num = int(sparse_feature_number), int(emb_dim), int(neg_num)
        self.emb_name, self.emb_w_name, self.emb_b_name = emb_name, emb_w_name, emb_b_name
        if self.sparse_feature_number < 1 or not 1 <= self.emb_dim <= REC_W2V_MAX_DIM:
            raise ValueError("word2vec: sparse_feature_number must be positive and sparse_feature_dim in 1..%d" % REC_W2V_MAX_DIM)
        if not 1 <= self.neg_num <= REC_W2V_MAX_NEG:
            raise ValueError("word2vec: neg_num must be in 1..%d, got %d" % (REC_W2V_MAX_NEG, self.neg_num))
        V, D = self.sparse_feature_number, self.emb_dim
        f32 = dict(dtype=torch.float32, device=self.device)
        init_width = 0.5 / D                                                   # net.py:32
        self.emb = torch.empty(V, D, **f32).uniform_(-init_width, init_width)
        self.emb_w = torch.zeros(V, D, **f32)                                  # net.py:48, :56: Constant(0.0)
        self.emb_b = torch.zeros(V, 1, **f32)
        self._pp = None
        self.record_gradients = False            # True: every step also leaves the merged target-row gradients

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        return {"embedding.weight": self.emb, "embedding_w.weight": self.emb_w, "embedding_b.weight": self.emb_b}

    # ---------------------------------------------------------------- forward / training
    def _check(self, in_ids, target_ids):
        if in_ids.dim() != 1 or in_ids.dtype != torch.int64:
            raise ValueError("expected in_ids int64 [B], got %s %s" % (in_ids.dtype, tuple(in_ids.shape)))
        if tuple(target_ids.shape) != (in_ids.shape[0], 1 + self.neg_num) or target_ids.dtype != torch.int64:
            raise ValueError("expected target_ids int64 [B, %d], got %s %s" % (1 + self.neg_num, target_ids.dtype,
                                                                                tuple(target_ids.shape)))

    def forward(self, inputs):
        """net.py:57-81 with the reference's three inputs [input_word [B, 1], true_word [B, 1], neg_word [B, neg]]
        -> (true_logits [B, 1], neg_logits [B, neg]).  Nothing is stepped."""
        in_ids = inputs[0].reshape(-1).contiguous()
        target_ids = torch.cat([inputs[1].reshape(-1, 1), inputs[2].reshape(-1, self.neg_num)], 1).contiguous()
        self._check(in_ids, target_ids)
        t, n = self.k.w2v_sgns_fwd_bwd(in_ids, target_ids, self.emb, self.emb_w, self.emb_b, 1.0, self.status)[:2]
        return t.view(-1, 1), n

    __call__ = forward

    def train_step(self, in_ids, target_ids, lr=1.0, check_ids=False):
        """forward + create_loss + backward + SGD (dygraph_model.py:53-76).  check_ids: read the status word back before
        any table is stepped and raise on an id outside the table (a host sync; the trainer reads it at its log lines
        instead, where a flagged pair has contributed nothing: g = 0)."""
        k, V, D = self.k, self.sparse_feature_number, self.emb_dim
        self._check(in_ids, target_ids)
        B = in_ids.shape[0]
        true_logits, neg_logits, g, d_in, loss, _ = k.w2v_sgns_fwd_bwd(in_ids, target_ids, self.emb, self.emb_w, self.emb_b, 1.0,
                                                                      self.status)
        if check_ids:
            k.raise_on_status(self.status, "word2vec")
        self.step_count += 1
        n = target_ids.numel()
        groups_t = self._grouped("target", target_ids.reshape(-1), V, None, self._group_status)
        dw = db = None
        if self.record_gradients:
            dw = torch.zeros(n, D, dtype=torch.float32, device=self.device)
            db = torch.zeros(n, dtype=torch.float32, device=self.device)
        k.w2v_target_update(groups_t, g, in_ids, self.emb, self.emb_w, self.emb_b, lr, dw, db)     # reads the OLD emb
        groups_in = self._grouped("in", in_ids, V, None, self._group_status)
        self._pp = k.segment_partials(groups_in, d_in, D, out=self._pp)
        k.sparse_sgd_rows(groups_in, d_in, self.emb, lr, partials=self._pp)
        self._last = dict(in_ids=in_ids, d_in=d_in, dw=dw, db=db, g=g)
        return loss, true_logits, neg_logits

    def last_gradients(self):
        """The dense gradients of the newest train_step as {state_dict key: tensor}, rebuilt with torch from the step's row
        gradients (for inspection, not on the step's path).  Needs record_gradients = True before the step."""
        last = self._last
        if last is None or last["dw"] is None:
            raise RuntimeError("set record_gradients = True before the train_step whose gradients are wanted")
        sp, uniq, offs = self._id_groups["target"].host()
        rows = torch.as_tensor(np.asarray(uniq), dtype=torch.int64, device=self.device)
        U = rows.numel()
        ok = (last["in_ids"] >= 0) & (last["in_ids"] < self.sparse_feature_number)
        return {"embedding.weight": torch.zeros_like(self.emb).index_add_(0, last["in_ids"][ok], last["d_in"][ok]),
                "embedding_w.weight": torch.zeros_like(self.emb_w).index_add_(0, rows, last["dw"][:U]),
                "embedding_b.weight": torch.zeros_like(self.emb_b).index_add_(0, rows, last["db"][:U].view(-1, 1))}


class Word2VecInferLayer(LayerBase):
    """net.py:84-110.  forward(analogy_a, analogy_b, analogy_c [B] or [B, 1], k=4) -> (values [B, k], pred_idx [B, k]); the
    reference's all_label argument is the whole vocabulary in order and is not needed."""

    def __init__(self, sparse_feature_number, emb_dim, emb_name="emb", device="cuda", kernels=None, table=None):
        self._init_runtime(device, kernels)
        self.sparse_feature_number, self.emb_dim, self.emb_name = int(sparse_feature_number), int(emb_dim), emb_name
        if table is not None:
            self.emb = table                                   # share a trained layer's table
        else:
            init_width = 0.5 / self.emb_dim
            self.emb = torch.empty(self.sparse_feature_number, self.emb_dim, dtype=torch.float32,
                                   device=self.device).uniform_(-init_width, init_width)

    def state_dict(self):
        return {"embedding.weight": self.emb}

    def set_dict(self, sd):
        mine = self.state_dict()                               # infer.py loads a training checkpoint: the other keys are not ours
        super().set_dict({key: v for key, v in sd.items() if key in mine})

    def forward(self, analogy_a, analogy_b, analogy_c, all_label=None, k=4):
        a, b, c = (t.reshape(-1).to(torch.int64).contiguous() for t in (analogy_a, analogy_b, analogy_c))
        return self.k.w2v_analogy_topk(a, b, c, self.emb, k, self.status)

    __call__ = forward


class W2VLoss:
    """The step's loss [1] on the device, read when asked (the trainer's log line)."""

    def __init__(self, loss):
        self.loss = loss

    def reshape(self, *shape):
        return self.loss.reshape(*shape)

    def item(self):
        return self.loss.item()

    __float__ = item


class DygraphModel:
    """word2vec/dygraph_model.py — same method names; tensors are torch device tensors — plus the body of infer.py's batch
    loop as infer_forward / infer_summary."""

    def __init__(self):
        self.hits = self.seen = 0
        self._infer = None

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        self.hits = self.seen = 0
        self._infer = None
        return Word2VecLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                             g("hyper_parameters.neg_num"), emb_name="emb", emb_w_name="emb_w", emb_b_name="emb_b",
                             device=device, kernels=kernels)

    def create_feeds(self, batch_data, config, device="cuda"):
        """(in_ids [B], target_ids [B, 1 + neg]) as reader.Word2vecReader yields them, or the reference's three
        (input_word, true_word, neg_word) -> (in_ids [B], target_ids [B, 1 + neg]) on `device`, int64."""
        neg_num = config.get("hyper_parameters.neg_num")
        ts = [torch.as_tensor(b).to(device).to(torch.int64) for b in batch_data[:3]]
        if len(ts) == 3:
            ts = [ts[0], torch.cat([ts[1].reshape(-1, 1), ts[2].reshape(-1, neg_num)], 1)]
        return ts[0].reshape(-1).contiguous(), ts[1].reshape(-1, 1 + neg_num).contiguous()

    def create_metrics(self, device="cuda"):
        return [], []                                       # dygraph_model.py:80-83: no metric

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        in_ids, target_ids = self.create_feeds(batch_data, config, dy_model.device)
        loss, _, _ = dy_model.train_step(in_ids, target_ids, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        loss = W2VLoss(loss)
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        """infer.py:129-146 for one batch of reader.Word2vecInferReader: (a, b, c, label [B, 1], inputs_word [B, 3])."""
        if self._infer is None or self._infer.emb is not dy_model.emb:
            self._infer = Word2VecInferLayer(dy_model.sparse_feature_number, dy_model.emb_dim, device=dy_model.device,
                                             kernels=dy_model.k, table=dy_model.emb)
            self._infer.status = dy_model.status
        a, b, c, label = (torch.as_tensor(t).to(dy_model.device).to(torch.int64) for t in batch_data[:4])
        inputs_word = np.asarray(torch.as_tensor(batch_data[4]).cpu())
        _, pred_idx = self._infer.forward(a, b, c)
        self.count(pred_idx.cpu().numpy(), np.asarray(label.cpu()).reshape(-1), inputs_word)
        return metrics_list, None

    def count(self, pre, label, inputs_word):
        """infer.py:138-146: the first of the predictions that is not one of the sample's three input words is compared with
        the label."""
        for ii in range(len(label)):
            self.seen += 1
            for idx in pre[ii]:
                if int(idx) in inputs_word[ii]:
                    continue
                if int(idx) == int(label[ii]):
                    self.hits += 1
                break

    def infer_summary(self):
        """The epoch's acc = hits / seen (and a fresh count for the next epoch)."""
        acc = self.hits * 1.0 / max(self.seen, 1)
        self.hits = self.seen = 0
        return {"acc": acc}
