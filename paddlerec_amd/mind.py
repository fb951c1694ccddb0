"""Host-side mirror of the reference's MIND plugin (models/recall/mind/net.py:21-318 Mind_SampledSoftmaxLoss_Layer,
Mind_Capsual_Layer, MindLayer; dygraph_model.py; infer.py) on the recengine HIP kernels: the Multi-Interest Network with
Dynamic routing, a retrieval model — one item table, a capsule layer that routes the user's history into k_max interest
capsules, a label-aware attention over them and a sampled-softmax loss against n shared negatives.

  * history [B, T] -> rec_emb_gather(padding_idx 0) -> one GEMM with bilinear_mapping_matrix -> low [B*T, H];
    rec_mind_routing_fwd runs ALL routing rounds in one launch (low[b] read once, kept in LDS; the reference's [B, K, T, H]
    tile is never formed) -> W, Z, caps; relu_layer is one GEMM (bias + ReLU) over caps viewed as [B*K, H];
  * the label's row through the padding Embedding is the attention's query: rec_mind_label_attn_fwd -> user [B, H];
  * the true and the sampled rows come from ONE rec_emb_gather over labels | negatives WITHOUT a padding id
    (paddle.gather, net.py:75-76), their biases and log_q from two more over [N, 1] views; S = user x sample_w^T is a GEMM;
    rec_mind_ssm_head: true logit, accidental-hit mask, both log_q subtractions, log-sum-exp, the loss, d(S) in place,
    d(true logit) and the true column's two row scalings;
  * backward: d(user) = d_true true_w + dS x sample_w (GEMM, REC_EPI_ADD), d(sample_w) = dS^T x user (GEMM),
    rec_mind_label_attn_bwd, the ReLU mask, relu_layer's dW / db / dX (one pair), rec_mind_routing_bwd (W is a constant:
    the inner rounds and B sit behind stop_gradient), then dM and d(history rows) (one pair);
  * the table's FOUR gradient sources — history [B*T] and query [B] (padding id 0 takes none), true [B] and sampled [n]
    (id 0 is an ordinary row) — are rows of ONE buffer grouped ONCE and applied by ONE rec_adam_rows_all: Paddle's dygraph
    Adam without L2, non-lazy, duplicates across the sources summed.  The three dense parameters live in one flat buffer
    stepped by one rec_adam_dense.  embedding_bias and routing_logits are in state_dict and never stepped.
Names are the reference's: item_emb.weight, embedding_bias, capsual_layer.routing_logits,
capsual_layer.bilinear_mapping_matrix, capsual_layer.relu_layer.weight / .bias."""
import math

import numpy as np
import torch

from .mtl import ADAM_EPS, BETA1, BETA2
from .net_base import FlatStore, LayerBase

QUIRKS = ("the FINAL routing softmax runs over the k_max capsules (net.py:226, axis=1) where the iters - 1 inner rounds run "
          "over the positions: a padded position gets weight exactly 1/k_max on every capsule, not zero, and contributes "
          "whatever the mapped history holds there — zero for the reader's padding id 0 (the Embedding's padding row), "
          "anything for a non-zero id behind seq_len; B += B_delta updates padded positions too; only the last W x low "
          "product carries a gradient (low_capsule_new_nograd and B are behind stop_gradient), so routing_logits has none "
          "and, like embedding_bias, is trainable=False: both are saved and never stepped (embedding_bias stays zero); "
          "label_aware_attention multiplies [B, K, hidden_size] by the label's [B, embedding_dim, 1] and the loss multiplies "
          "the [B, hidden_size] user vector with item rows, so embedding_dim must equal hidden_size: anything else fails "
          "in the reference's matmul and is refused here; item_emb is read in two ways — through "
          "nn.Embedding(padding_idx=0) for the history and the attention's query (id 0: a zero row, no gradient) and "
          "through paddle.gather for the true and sampled rows (id 0: an ordinary row); the attention has no capsule mask "
          "and its scores go through pow(score, pow_p) before the softmax (a negative score under a fractional pow_p is "
          "NaN, as in Paddle); the accidental-hit mask (-1e30) goes in BEFORE log_q is subtracted; the log-uniform table "
          "is prob[i] = log((i+2)/(i+1)) / log(N+1) in float64 with prob[0] = 0, NOT normalised, cast to float32, and "
          "log_q = log(-(exp(-log1p(p) * 2n) - 1)) in float32: the expression cancels for small p and log_q[0] = -inf, so "
          "a label of 0 gives a non-finite loss in the reference and here alike (the readers never yield one); ONE draw "
          "of n distinct negatives is shared by the batch (multinomial without replacement over prob: id 0 is never "
          "drawn), made with torch from (seed, step) — Paddle's own random stream cannot be reproduced; Adam "
          "(beta 0.9 / 0.999, epsilon 1e-8, no L2) is non-lazy: every row of the table moves every step; the train "
          "reader calls random.seed(12345) before EVERY choice of the cut position, so a user's cut depends only on the "
          "history's length; infer.py starts its sample count at 1 (total = 1), so every retrieval metric is divided by "
          "samples + 1; the learning rate is hyper_parameters.optimizer.learning_rate (default 0.001)")


def _rounded_f32(fn, x):
    """fn(x) as the correctly rounded float32: evaluated in float64 and rounded once.  torch's float32 log1p / exp / log
    differ in the last bit between CPUs (their vector forms follow the instruction set), and the table must not."""
    return fn(x.double()).float()


def log_uniform_table(item_count, n_sample):
    """net.py:40-47, the reference's own operation sequence on the host (torch, CPU): prob in float64, cast to float32, then
    log(-(exp(-log1p(p) * 2 * n) - 1)) with EVERY intermediate a float32 — the cancellation for small p is the reference's
    and is kept; each of the three functions returns the correctly rounded float32 (_rounded_f32).
    -> (prob float32 [N], log_q float32 [N])."""
    prob = np.array([0.0] * item_count)
    for i in range(1, item_count):
        prob[i] = (np.log(i + 2) - np.log(i + 1)) / np.log(item_count + 1)
    new_prob = torch.from_numpy(prob.astype("float32"))
    log_q = _rounded_f32(torch.log, -(_rounded_f32(torch.exp, (-_rounded_f32(torch.log1p, new_prob) * 2 * n_sample)) - 1.0))
    return new_prob, log_q


class MindLoss:
    """The step's loss, the batch mean of loss_b [B] (dygraph_model.py:58-59): reduced (torch) when it is read."""

    def __init__(self, loss_b):
        self.loss_b, self._v = loss_b, None

    def value(self):
        if self._v is None:
            self._v = self.loss_b.mean().reshape(1)
        return self._v

    def reshape(self, *shape):
        return self.value().reshape(*shape)

    def item(self):
        return self.value().item()

    __float__ = item


class Mind_Capsual_Layer(LayerBase):
    """net.py:116-234.  forward(item_his_emb [B*T, input_units], seq_len [B]) -> (high_capsule [B*K, output_units] after
    relu_layer, W [B, K, T], seq_len); keep: a dict that receives what the backward needs."""

    def __init__(self, input_units, output_units, iters=3, maxlen=32, k_max=3, init_std=1.0, batch_size=None, device="cuda",
                 kernels=None):
        self._init_runtime(device, kernels)
        self.iters, self.input_units, self.output_units = int(iters), int(input_units), int(output_units)
        self.maxlen, self.init_std, self.k_max, self.batch_size = int(maxlen), float(init_std), int(k_max), batch_size
        from ._lib import REC_MIND_MAX_H, REC_MIND_MAX_ITERS, REC_MIND_MAX_K, REC_MIND_MAX_T
        for v, hi, n in ((self.maxlen, REC_MIND_MAX_T, "maxlen"), (self.k_max, REC_MIND_MAX_K, "k_max"),
                         (self.output_units, REC_MIND_MAX_H, "output_units"), (self.iters, REC_MIND_MAX_ITERS, "iters")):
            if not 1 <= v <= hi:
                raise ValueError("Mind_Capsual_Layer: %s must be in 1..%d, got %d" % (n, hi, v))
        E, H = self.input_units, self.output_units
        self.flat = FlatStore([("bilinear_mapping_matrix", (E, H)), ("relu_layer.weight", (H, H)), ("relu_layer.bias", (H,))],
                              self.device)
        self.params = self.flat.view["p"]
        self.routing_logits = torch.empty(1, self.k_max, self.maxlen, dtype=torch.float32, device=self.device)
        self.routing_logits.normal_(0.0, self.init_std)                       # trainable=False (net.py:142)
        self.params["bilinear_mapping_matrix"].normal_(0.0, self.init_std)
        lim = math.sqrt(6.0 / (H + H))                                         # nn.Linear: XavierUniform, zero bias [EXT]
        self.params["relu_layer.weight"].uniform_(-lim, lim)

    def forward(self, item_his_emb, seq_len, keep=None):
        k, p = self.k, self.params
        low = k.gemm(item_his_emb, p["bilinear_mapping_matrix"], self.ws)                    # net.py:191
        W, Z, caps = k.mind_routing_fwd(low, seq_len, self.routing_logits, self.iters)       # net.py:194-229
        caps = caps.view(-1, self.output_units)
        high = k.gemm(caps, p["relu_layer.weight"], self.ws, epilogue="bias_relu", bias=p["relu_layer.bias"])   # net.py:233
        if keep is not None:
            keep.update(emb=item_his_emb, W=W, Z=Z, caps=caps, caps2=high)
        return high, W, seq_len

    __call__ = forward

    def backward(self, d_high, sv, d_emb_out):
        """d_high [B*K, H] by the ReLU's output (overwritten with the mask applied) -> the dense gradients in the flat
        buffer and d(item_his_emb) written to d_emb_out [B*T, E]."""
        k, p, g = self.k, self.params, self.flat.view["g"]
        k.relu_mask_(d_high, sv["caps2"])
        d_caps = k.linear_backward(sv["caps"], d_high, p["relu_layer.weight"], self.ws, g["relu_layer.weight"],
                                   g["relu_layer.bias"])
        d_low = k.mind_routing_bwd(d_caps.view(-1, self.k_max, self.output_units), sv["Z"], sv["W"])
        k.linear_backward(sv["emb"], d_low, p["bilinear_mapping_matrix"], self.ws, g["bilinear_mapping_matrix"], None,
                          out=d_emb_out)
        return d_low


class MindLayer(LayerBase):
    """net.py:237-318.  forward(hist_item [B, T], seqlen [B]) -> (user_cap [B, K, H], cap_weights [B, K, T]) (eval mode);
    train_step(hist_item, seqlen, labels [B], lr, neg=None) -> (loss: a MindLoss, user_cap, cap_weights)."""

    def __init__(self, item_count, embedding_dim, hidden_size, neg_samples=100, maxlen=30, pow_p=1.0, capsual_iters=3,
                 capsual_max_k=3, capsual_init_std=1.0, batch_size=None, device="cuda", kernels=None, seed=12345):
        self._init_runtime(device, kernels, group_status=True)     # the grouping's own status word: see _table_step
        self.item_count, self.embedding_dim, self.hidden_size = int(item_count), int(embedding_dim), int(hidden_size)
        self.neg_samples, self.maxlen, self.pow_p, self.seed = int(neg_samples), int(maxlen), float(pow_p), int(seed)
        if self.item_count < 2 or self.embedding_dim < 1:
            raise ValueError("MIND: item_count must be at least 2 and embedding_dim positive")
        if self.embedding_dim != self.hidden_size:
            raise ValueError("MIND: embedding_dim (%d) must equal hidden_size (%d) — label_aware_attention multiplies the "
                             "[B, K, hidden_size] capsules by the label's [B, embedding_dim, 1] (net.py:287-290)"
                             % (self.embedding_dim, self.hidden_size))
        if not 1 <= self.neg_samples < self.item_count:
            raise ValueError("MIND: neg_samples must be in 1..item_count - 1 (distinct ids, never id 0)")
        N, E = self.item_count, self.embedding_dim
        self.emb = torch.empty(N, E, dtype=torch.float32, device=self.device)
        lim = math.sqrt(6.0 / (N + E))                       # XavierUniform(fan_in=item_count, fan_out=embedding_dim)
        self.emb.uniform_(-lim, lim)
        self.emb[0].zero_()                                  # nn.Embedding zeroes its padding row at construction [EXT]
        self.emb_m, self.emb_v = torch.zeros_like(self.emb), torch.zeros_like(self.emb)
        self.embedding_bias = torch.zeros(N, dtype=torch.float32, device=self.device)           # trainable=False
        self.capsual_layer = Mind_Capsual_Layer(E, self.hidden_size, maxlen=self.maxlen, iters=capsual_iters,
                                                k_max=capsual_max_k, init_std=capsual_init_std, batch_size=batch_size,
                                                device=device, kernels=kernels)
        self.prob, log_q = log_uniform_table(N, self.neg_samples)         # host, once (net.py:40-47)
        self.log_q_host = log_q
        self.log_q = log_q.to(self.device)
        self.ws = self.capsual_layer.ws                                   # one scratch buffer for both
        self._pp = None

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        c = self.capsual_layer
        return {"item_emb.weight": self.emb, "embedding_bias": self.embedding_bias,
                "capsual_layer.routing_logits": c.routing_logits,
                "capsual_layer.bilinear_mapping_matrix": c.params["bilinear_mapping_matrix"],
                "capsual_layer.relu_layer.weight": c.params["relu_layer.weight"],
                "capsual_layer.relu_layer.bias": c.params["relu_layer.bias"]}

    STEPPED = ("item_emb.weight", "capsual_layer.bilinear_mapping_matrix", "capsual_layer.relu_layer.weight",
               "capsual_layer.relu_layer.bias")

    def _optimizer_views(self):
        """Adam's moments of every stepped parameter (STEPPED), under the parameter's own name."""
        out = {}
        for s, t in (("m", self.emb_m), ("v", self.emb_v)):
            out["mtl.%s.item_emb.weight" % s] = t
            out.update(("mtl.%s.capsual_layer.%s" % (s, k), v) for k, v in self.capsual_layer.flat.view[s].items())
        return out

    # ---------------------------------------------------------------- negatives
    def sample_negatives(self, step):
        """The shared draw of training step `step` (1-based): neg_samples DISTINCT ids by multinomial without replacement
        over the unnormalised log-uniform prob (net.py:55-58); prob[0] = 0, so id 0 is never drawn.  A torch.Generator
        seeded from (seed, step): the draw can be rebuilt.  -> int64 [n] on the host."""
        g = torch.Generator()
        g.manual_seed((self.seed * 1000003 + int(step)) % (2 ** 63))
        return torch.multinomial(self.prob, self.neg_samples, replacement=False, generator=g)

    # ---------------------------------------------------------------- forward
    def _check(self, hist_item, seqlen):
        if hist_item.dim() != 2 or hist_item.shape[1] != self.maxlen or hist_item.dtype != torch.int64:
            raise ValueError("expected hist_item int64 [B, %d], got %s %s" % (self.maxlen, hist_item.dtype, tuple(hist_item.shape)))
        if tuple(seqlen.shape) != (hist_item.shape[0],) or seqlen.dtype != torch.int64:
            raise ValueError("expected seqlen int64 [B], got %s %s" % (seqlen.dtype, tuple(seqlen.shape)))

    def _capsules(self, hist_item, seqlen, keep=None):
        self._check(hist_item, seqlen)
        emb, _ = self.k.emb_gather(hist_item.reshape(-1), self.emb, 0, status=self.status)       # net.py:308
        return self.capsual_layer(emb, seqlen, keep)

    def forward(self, hist_item, seqlen, labels=None):
        """net.py:299-312 in eval mode: (user_cap [B, K, H], cap_weights [B, K, T])."""
        high, W, _ = self._capsules(hist_item, seqlen)
        return high.view(hist_item.shape[0], self.capsual_layer.k_max, self.hidden_size), W

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, hist_item, seqlen, labels, lr=0.001, neg=None):
        """net.py:299-318 + backward + Adam.  labels int64 [B]; neg: int64 [n] distinct ids (None: sample_negatives of this
        step).  -> (loss: a MindLoss, user_cap [B, K, H], cap_weights [B, K, T])."""
        k, ws, c = self.k, self.ws, self.capsual_layer
        self.step_count += 1
        B, T, K, H, E, n = hist_item.shape[0], self.maxlen, c.k_max, self.hidden_size, self.embedding_dim, self.neg_samples
        if tuple(labels.shape) != (B,) or labels.dtype != torch.int64:
            raise ValueError("labels must be int64 [B], got %s %s" % (labels.dtype, tuple(labels.shape)))
        if neg is None:
            neg = self.sample_negatives(self.step_count)
        neg = torch.as_tensor(neg).to(self.device).to(torch.int64).reshape(-1).contiguous()
        if neg.numel() != n:
            raise ValueError("neg must hold %d ids, got %d" % (n, neg.numel()))
        sv = {}
        high, W, _ = self._capsules(hist_item, seqlen, sv)
        target, _ = k.emb_gather(labels, self.emb, 0, status=self.status)                         # net.py:313
        user, attn = k.mind_label_attn_fwd(high, target, K, self.pow_p)                           # net.py:314
        # net.py:75-84: paddle.gather over labels | negatives, no padding id
        all_ids = torch.cat([labels, neg])
        all_w, _ = k.emb_gather(all_ids, self.emb, None, status=self.status)
        all_b, _ = k.emb_gather(all_ids, self.embedding_bias.view(-1, 1), None, status=self.status)
        all_q, _ = k.emb_gather(all_ids, self.log_q.view(-1, 1), None, status=self.status)
        true_w, sample_w = all_w[:B], all_w[B:]
        all_b, all_q = all_b.view(-1), all_q.view(-1)
        S = k.gemm(user, sample_w, ws, trans_b=True)                                              # net.py:91
        # ONE buffer for the table's four gradient sources: history | query | true | sampled
        G = torch.empty(B * T + 2 * B + n, E, dtype=torch.float32, device=self.device)
        o_q, o_t, o_s = B * T, B * T + B, B * T + 2 * B
        du0 = torch.empty(B, H, dtype=torch.float32, device=self.device)
        loss_b, d_true, dS = k.mind_ssm_head(user, true_w, all_b[:B], S, all_b[B:], labels, neg, all_q[:B], all_q[B:], 1.0 / B,
                                             d_true_w=G[o_t:o_s], d_user0=du0)
        d_user = k.gemm(dS, sample_w, ws, epilogue="add", aux1=du0)        # d_true true_w + dS x sample_w
        k.gemm(dS, user, ws, trans_a=True, out=G[o_s:])                    # d(sample_w) = dS^T x user
        d_high, _ = k.mind_label_attn_bwd(high, target, attn, d_user, self.pow_p, d_target=G[o_q:o_t])
        c.backward(d_high, sv, G[:o_q])
        f = c.flat.flat
        k.adam_dense(f["p"], f["m"], f["v"], f["g"], self.step_count, lr, BETA1, BETA2, ADAM_EPS)
        self._last = dict(G=G, hist=hist_item, labels=labels, neg=neg, attn=attn, user=user)
        self._table_step(hist_item, labels, neg, G, lr)
        return MindLoss(loss_b), high.view(B, K, H), W

    def _table_step(self, hist_item, labels, neg, G, lr):
        """Non-lazy Adam on every row of the table from the rows of G.  The history's and the query's lookups went through
        the padding Embedding: their id 0 takes no gradient, so it is handed to the grouping as -1, which the grouping
        drops (it also counts it as out of range, in a status word of its own that nothing reads; an id that really is
        outside the table has already been flagged in self.status by the gathers)."""
        k = self.k
        pad = lambda ids: torch.where(ids == 0, torch.full_like(ids, -1), ids)
        rows = torch.cat([pad(hist_item.reshape(-1)), pad(labels), labels, neg])
        groups = self._grouped("emb", rows, self.item_count, None, self._group_status)
        E = self.embedding_dim
        self._pp = k.segment_partials(groups, G, E, out=self._pp)
        k.adam_rows_all(groups, G, 1, self.emb, self.emb_m, self.emb_v, self.step_count, lr, BETA1, BETA2, ADAM_EPS,
                        partials=self._pp)

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor} for the stepped parameters; the table's dense
        [N, E] gradient is rebuilt with torch from the step's gradient rows (for inspection, not on the step's path)."""
        v = self.capsual_layer.flat.view["g"]
        out = {"capsual_layer." + kk: v[kk].clone() for kk in ("bilinear_mapping_matrix", "relu_layer.weight", "relu_layer.bias")}
        last = self._last
        hist, labels = last["hist"].reshape(-1), last["labels"]
        rows = torch.cat([hist, labels, labels, last["neg"]])
        keep = torch.cat([hist != 0, labels != 0, torch.ones(labels.numel() + last["neg"].numel(), dtype=torch.bool,
                                                             device=rows.device)])
        out["item_emb.weight"] = torch.zeros_like(self.emb).index_add_(0, rows[keep], last["G"][keep])
        return out


# ---------------------------------------------------------------------------------------------------- retrieval (infer.py)
def search_inner_product(k, ws, queries, table, top_n, chunk=65536):
    """Exact inner-product search (infer.py's faiss IndexFlatIP): queries [Q, E] against every row of table [N, E] as GEMMs
    over item chunks, torch.topk per chunk and a merge.  -> (scores [Q, top_n], ids [Q, top_n]) sorted by score."""
    N = table.shape[0]
    top_n = min(int(top_n), N)
    best_s = best_i = None
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        s = k.gemm(queries, table[lo:hi], ws, trans_b=True)
        cs, ci = torch.topk(s, min(top_n, hi - lo), dim=1)
        ci = ci + lo
        if best_s is not None:
            cs, ci = torch.cat([best_s, cs], 1), torch.cat([best_i, ci], 1)
            cs, order = torch.topk(cs, min(top_n, cs.shape[1]), dim=1)
            ci = torch.gather(ci, 1, order)
        best_s, best_i = cs, ci
    return best_s, best_i


class RetrievalMetrics:
    """infer.py:103-194: recall@N, ndcg@N and hitrate@N, with the reference's `total = 1` start."""

    def __init__(self, top_n=20):
        self.top_n = int(top_n)
        self.reset()

    def reset(self):
        self.total, self.total_recall, self.total_ndcg, self.total_hitrate = 1, 0.0, 0.0, 0

    def update(self, D, I, target_items, ni=None):
        """D, I: scores and ids [B * ni, top_n] of the B samples' ni user vectors each (the reference's 3-D branch, which
        MIND's [B, K, H] capsules always take, K = 1 included), or with ni None [B, top_n] of one vector per sample (its
        2-D branch); target_items [B, maxlen] (0 = padding)."""
        D, I, target_items = np.asarray(D), np.asarray(I), np.asarray(target_items)
        for i, iid_list in enumerate(target_items):
            recall, dcg = 0, 0.0
            if ni is None:                                                # infer.py:117-135
                cor = list(I[i])
            else:                                                         # infer.py:136-156: merge by score, dedup, drop id 0
                item_list = list(zip(np.reshape(I[i * ni:(i + 1) * ni], -1), np.reshape(D[i * ni:(i + 1) * ni], -1)))
                item_list.sort(key=lambda x: x[1], reverse=True)
                seen, cor = set(), []
                for iid, _ in item_list:
                    if iid not in seen and iid != 0:
                        seen.add(iid)
                        cor.append(iid)
                        if len(seen) >= self.top_n:
                            break
            iid_list = [x for x in iid_list if x != 0]
            true_item_set = set(iid_list)
            for no, iid in enumerate(cor):
                if iid in true_item_set:
                    recall += 1
                    dcg += 1.0 / math.log(no + 2, 2)
            idcg = sum(1.0 / math.log(no + 2, 2) for no in range(recall))
            self.total_recall += recall * 1.0 / len(iid_list)
            if recall > 0:
                self.total_ndcg += dcg / idcg
                self.total_hitrate += 1
        self.total += target_items.shape[0]

    def values(self):
        n = self.top_n
        return {"recall@%d" % n: self.total_recall / self.total, "ndcg@%d" % n: self.total_ndcg / self.total,
                "hitrate@%d" % n: self.total_hitrate * 1.0 / self.total}


class DygraphModel:
    """mind/dygraph_model.py — same method names; tensors are torch device tensors."""

    def __init__(self):
        self.retrieval = RetrievalMetrics()

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        self.retrieval = RetrievalMetrics(g("runner.top_n", 20))
        return MindLayer(g("hyper_parameters.item_count", None), g("hyper_parameters.embedding_dim", 64),
                         g("hyper_parameters.hidden_size", 64), g("hyper_parameters.neg_samples", 100),
                         g("hyper_parameters.maxlen", 30), g("hyper_parameters.pow_p", 1.0),
                         g("hyper_parameters.capsual.iters", 3), g("hyper_parameters.capsual.max_k", 4),
                         g("hyper_parameters.capsual.init_std", 1.0), device=device, kernels=kernels,
                         seed=g("runner.seed", 12345))

    def create_feeds_train(self, batch_data, device="cuda"):
        """(hist_item [B, T], target_item [B, 1], seq_len [B, 1]) as reader.MindReader yields them -> (hist_item [B, T],
        labels [B], seq_len [B]) on `device`, int64."""
        hist, target, seq = (torch.as_tensor(b).to(device).to(torch.int64) for b in batch_data[:3])
        return hist.contiguous(), target.reshape(-1).contiguous(), seq.reshape(-1).contiguous()

    def create_feeds_infer(self, batch_data, device="cuda"):
        """(hist_item [B, T], seq_len [B, 1], eval_items [B, 1, T]) -> (hist_item, seq_len [B], eval_items [B, T])."""
        hist, seq = (torch.as_tensor(b).to(device).to(torch.int64) for b in batch_data[:2])
        ev = torch.as_tensor(batch_data[2])
        return hist.contiguous(), seq.reshape(-1).contiguous(), ev.reshape(ev.shape[0], -1)

    def create_metrics(self, device="cuda"):
        return [], []                                       # dygraph_model.py:70-73: no metric in the train loop

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        hist, labels, seq = self.create_feeds_train(batch_data, dy_model.device)
        loss, _, _ = dy_model.train_step(hist, seq, labels, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        """dygraph_model.py:85-91 and the body of infer.py's batch loop: the K capsules of every sample are searched against
        the item table and the hits folded into self.retrieval."""
        hist, seq, ev = self.create_feeds_infer(batch_data, dy_model.device)
        dy_model.eval()
        user_cap, _ = dy_model.forward(hist, seq)
        B, K, H = user_cap.shape
        D, I = search_inner_product(dy_model.k, dy_model.ws, user_cap.reshape(B * K, H), dy_model.emb, self.retrieval.top_n)
        self.retrieval.update(D.cpu().numpy(), I.cpu().numpy(), ev.cpu().numpy(), K)
        return metrics_list, None

    def infer_summary(self):
        """The epoch's retrieval metrics (and a fresh count for the next epoch)."""
        vals = self.retrieval.values()
        self.retrieval.reset()
        return vals
