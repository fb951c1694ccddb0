"""Host-side mirror of the reference's TiSASRec plugin (models/recall/tisas/net.py:26-309 PointWiseFeedForward,
TimeAwareMultiHeadAttention, TiSASRecLayer; dygraph_model.py; infer.py) on the recengine HIP kernels: the time-interval-aware
self-attention sequential recommender, the third retrieval model of the tree.

  * log_seqs [B, L] -> rec_tisas_embed_fwd (item_emb * sqrt(D), dropout, the padding mask: one pass);
  * per block: rec_affine_layer_norm_fwd (the residual add and `seqs *= (log_seqs != 0)` of the block before are part of
    it and it hands back the masked sum, the block's keys), three GEMMs (REC_EPI_BIAS) for Q_w / K_w / V_w,
    rec_tisas_attn_fwd — the reference's time_matrix_K / time_matrix_V, two [B, L, L, D] float tensors gathered from tables
    of (time_span + 1) x D, dropped out element by element and split per head, are NEVER formed, forward or backward: the
    kernel reads tm [B, L, L] and the tables — then rec_affine_layer_norm_fwd over Q + attention, the two k = 1
    convolutions as GEMMs (bias + ReLU in the first one's epilogue: relu(dropout(x)) == dropout(relu(x)) bit for bit) with
    rec_dropout behind each;
  * rec_tisas_head: both dot products, the two masked BCE means with the selected count taken on the device (no host
    sync), d(log_feats) and the gradient rows of the pos / neg lookups;
  * backward: the same kernels' counterparts; rec_tisas_attn_bwd sums the position tables over the batch and the time
    tables over every (b, i, j) that hit a row in a fixed order, the second block adding to the first's;
  * item_emb's three gradient sources (sequence, pos, neg; padding id 0 takes none) are rows of ONE buffer grouped ONCE and
    applied by ONE rec_adam_rows_all; everything else lives in one flat buffer stepped by one rec_adam_dense — Paddle's
    dygraph Adam(beta1 0.9, beta2 0.98), non-lazy, which for a dense table is the same arithmetic.
The conv weights are kept as [C_in, C_out] images (what the GEMMs read); state_dict shows them as the reference's
[C_out, C_in, 1] through a transposed view, so a reference checkpoint loads.  The train step is eager."""
import math

import numpy as np
import torch

from .mtl import ADAM_EPS, BETA1
from .net_base import FlatStore, LayerBase

BETA2 = 0.98                                     # dygraph_model.py:58-63
LN_EPS = 1e-8
QUIRKS = ("seqs = item_emb(log_seqs) * sqrt(hidden_units), THEN dropout, THEN * (log_seqs != 0); item_emb has padding_idx 0 "
          "(id 0 reads zeros, row 0 takes no gradient); abs_pos_K / abs_pos_V are expanded to the batch BEFORE their dropout, "
          "so the position masks are per sample, and the time tables' dropout runs over [B, L, L, D]; the five input "
          "dropouts are drawn once per step and every block reuses the same dropped tensors; per block Q = LN(seqs) and the "
          "residual is the layer-normed Q, not seqs (seqs = Q + MHA(Q, seqs)); then seqs = LN(seqs), seqs = seqs + "
          "dropout(conv2(relu(dropout(conv1(seqs))))) with k = 1 convolutions, then seqs *= (log_seqs != 0); every "
          "LayerNorm is affine with epsilon 1e-8; heads are contiguous slices of hidden_units // num_heads features and "
          "all four relation tables split the same way; a score row of a padded query (log_seqs == 0) is REPLACED by "
          "-2**32 + 1 (paddle.where, not an add), then every j > i is replaced as well: a padded query row attends "
          "uniformly, 1/L, over all L keys, future ones included; the loss is mean(BCE(pos_logits[pos != 0], 1)) + "
          "mean(BCE(neg_logits[pos != 0], 0)) (an empty selection gives NaN); Adam(beta1 0.9, beta2 0.98, lr 0.001) is "
          "non-lazy, without clip or decay; dropout_rate is the constructor's default 0.2 — dygraph_model.py never passes "
          "one; infer uses only item_indices[0], row 0's candidates, for every row of the batch (the reference infers at "
          "batch 1) and NDCG@10 / HR@10 count the rank of candidate 0 of the batch's row 0; the train reader ignores the "
          "index it is asked for and draws the user and the negatives from np.random seeded 2021 in the constructor; "
          "cleanAndsort numbers users and items in set order and rescales every user's times by the user's own smallest "
          "gap; the train relation matrix is built from user_train[:-1]; the test-mode branch for more than 10 000 users "
          "calls np.random.sample with two arguments and cannot run in the reference: it is refused here with an error; "
          "num_users / num_items come from the YAML, not from the data")
SITES = ("emb", "pos_k", "pos_v", "time_k", "time_v")          # the step's input dropouts; then att<n>, ffn1_<n>, ffn2_<n>


class TiSASLoss:
    """The step's loss [1] as the head left it on the device (loss2 = loss, selected count)."""

    def __init__(self, loss2):
        self.loss2 = loss2

    def value(self):
        return self.loss2[:1]

    def reshape(self, *shape):
        return self.value().reshape(*shape)

    def item(self):
        return self.value().item()

    __float__ = item


class TiSASRecLayer(LayerBase):
    """net.py:167-309.  forward(log_seqs [B, L], time_matrices [B, L, L], item_indices=None, pos_seqs=None, neg_seqs=None)
    -> logits [B, I] with item_indices, else (pos_logits, neg_logits) [B, L];
    train_step(log_seqs, time_matrices, pos_seqs, neg_seqs, lr) -> (loss: a TiSASLoss, log_feats [B, L, D])."""

    def __init__(self, user_num, item_num, hidden_units, maxlen, time_span, num_blocks, num_heads, dropout_rate=0.2,
                 device="cuda", kernels=None, dropout_seed=12345):
        self._init_runtime(device, kernels, group_status=True)
        self.user_num, self.item_num = int(user_num), int(item_num)
        D, H = int(hidden_units), int(num_heads)
        self.hidden_units, self.maxlen, self.time_span = D, int(maxlen), int(time_span)
        self.num_blocks, self.num_heads = int(num_blocks), H
        self.dropout_rate, self.dropout_seed = float(dropout_rate or 0.0), int(dropout_seed)
        if H < 1 or D < 1 or D % H:
            raise ValueError("TiSASRec: hidden_units %d must be a positive multiple of num_heads %d (net.py:82,92: the heads are "
                             "equal contiguous slices)" % (D, H))
        from ._lib import REC_TISAS_MAX_HEAD, REC_TISAS_MAX_L, REC_TISAS_MAX_TILE, REC_TISAS_MAX_TIME_TILE
        hd, T = D // H, self.time_span + 1
        if not (1 <= self.maxlen <= REC_TISAS_MAX_L and hd <= REC_TISAS_MAX_HEAD and self.maxlen * (hd | 1) <= REC_TISAS_MAX_TILE
                and T * hd <= REC_TISAS_MAX_TIME_TILE):
            raise ValueError("TiSASRec: maxlen %d / head size %d / time_span %d beyond rec_tisas_attn_*'s limits (maxlen <= %d, "
                             "head <= %d, maxlen * (head | 1) <= %d, (time_span + 1) * head <= %d)"
                             % (self.maxlen, hd, self.time_span, REC_TISAS_MAX_L, REC_TISAS_MAX_HEAD, REC_TISAS_MAX_TILE,
                                REC_TISAS_MAX_TIME_TILE))
        if self.num_blocks < 1 or self.item_num < 1:
            raise ValueError("TiSASRec: num_blocks and item_num must be positive")
        N = self.item_num + 1
        f32 = dict(dtype=torch.float32, device=self.device)
        xavier = lambda t, fi, fo: t.uniform_(-math.sqrt(6.0 / (fi + fo)), math.sqrt(6.0 / (fi + fo)))
        self.emb = xavier(torch.empty(N, D, **f32), N, D)
        self.emb[0].zero_()                                  # nn.Embedding zeroes its padding row at construction [EXT]
        self.emb_m, self.emb_v = torch.zeros_like(self.emb), torch.zeros_like(self.emb)
        entries = [("abs_pos_K_emb.weight", (self.maxlen, D)), ("abs_pos_V_emb.weight", (self.maxlen, D)),
                   ("time_matrix_K_emb.weight", (T, D)), ("time_matrix_V_emb.weight", (T, D)),
                   ("last_layernorm.weight", (D,)), ("last_layernorm.bias", (D,))]
        for n in range(self.num_blocks):
            entries += [("attention_layernorms.%d.weight" % n, (D,)), ("attention_layernorms.%d.bias" % n, (D,))]
            for w in ("Q_w", "K_w", "V_w"):
                entries += [("attention_layers.%d.%s.weight" % (n, w), (D, D)), ("attention_layers.%d.%s.bias" % (n, w), (D,))]
            entries += [("forward_layernorms.%d.weight" % n, (D,)), ("forward_layernorms.%d.bias" % n, (D,))]
            for c in ("conv1", "conv2"):                     # kept as the [C_in, C_out] image; see _conv_names
                entries += [("forward_layers.%d.%s.weight" % (n, c), (D, D)), ("forward_layers.%d.%s.bias" % (n, c), (D,))]
        self.flat = FlatStore(entries, self.device)
        self._conv_names = {n for n, _ in entries if ".conv" in n and n.endswith(".weight")}
        self.params = self.flat.view["p"]
        for name, sh in entries:
            t = self.params[name]
            if "layernorm" in name:
                t.fill_(1.0 if name.endswith(".weight") else 0.0)
            elif name.endswith(".weight"):
                xavier(t, sh[0], sh[1])                      # XavierUniform; every bias starts at zero [EXT]
        self._pp = None
        self._scratch = {}
        self.streams_per_step = len(SITES) + 3 * self.num_blocks

    # ---------------------------------------------------------------- parameters
    def _shown(self, store):
        """{state_dict key: tensor} of one store ("p", "g", "m", "v"); a conv weight as the reference's [C_out, C_in, 1]."""
        out = {"item_emb.weight": {"p": self.emb, "m": self.emb_m, "v": self.emb_v}.get(store)}
        for name, t in self.flat.view[store].items():
            out[name] = t.t().unsqueeze(-1) if name in self._conv_names else t
        return out

    def state_dict(self):
        return self._shown("p")

    def _optimizer_views(self):
        """Adam's moments of every parameter, under the parameter's own name."""
        return {"mtl.%s.%s" % (s, k): v for s in ("m", "v") for k, v in self._shown(s).items()}

    # ---------------------------------------------------------------- dropout sites
    def dropout_streams(self, step):
        """{site: mask stream} of training step `step` (1-based): "emb", "pos_k", "pos_v", "time_k", "time_v" (drawn once,
        shared by the blocks) and per block n "att<n>", "ffn1_<n>", "ffn2_<n>"; {} when dropout_rate is 0.  Tests rebuild
        the masks from these with rec_dropout on ones ([B*L, D]; time_*: [B*L*L, D]; att<n>: [B*H*L, L])."""
        if self.dropout_rate <= 0.0:
            return {}
        base = step * self.streams_per_step
        out = {s: base + i for i, s in enumerate(SITES)}
        for n in range(self.num_blocks):
            for j, s in enumerate(("att%d", "ffn1_%d", "ffn2_%d")):
                out[s % n] = base + len(SITES) + 3 * n + j
        return out

    # ---------------------------------------------------------------- forward
    def _check(self, log_seqs, tm):
        if log_seqs.dim() != 2 or log_seqs.dtype != torch.int64 or log_seqs.shape[1] > self.maxlen:
            raise ValueError("expected log_seqs int64 [B, L <= %d], got %s %s" % (self.maxlen, log_seqs.dtype, tuple(log_seqs.shape)))
        B, L = log_seqs.shape
        if tuple(tm.shape) != (B, L, L) or tm.dtype != torch.int64:
            raise ValueError("expected time_matrices int64 [B, L, L], got %s %s" % (tm.dtype, tuple(tm.shape)))
        return B, L

    def _tables(self, L, store="p"):
        v = self.flat.view[store]
        return (v["abs_pos_K_emb.weight"][:L], v["abs_pos_V_emb.weight"][:L], v["time_matrix_K_emb.weight"],
                v["time_matrix_V_emb.weight"])

    def _seq2feats(self, log_seqs, tm, streams, keep=None):
        """net.py:244-289 -> log_feats [B*L, D].  streams: {} (no dropout) or dropout_streams(step)."""
        k, p, ws = self.k, self.params, self.ws
        B, L = self._check(log_seqs, tm)
        D, H, rate, seed = self.hidden_units, self.num_heads, self.dropout_rate, self.dropout_seed
        on = bool(streams)
        ids = log_seqs.contiguous().view(-1)
        tm = tm.contiguous()
        seqs = k.tisas_embed_fwd(ids, self.emb, math.sqrt(D), rate if on else 0.0, seed, streams.get("emb", 0), status=self.status)
        tables = self._tables(L)
        scale = 1.0 / math.sqrt(D // H)
        probs = (rate, rate, rate) if on else (0.0, 0.0, 0.0)
        lin = lambda x, n: k.gemm(x, p[n + ".weight"], ws, epilogue="bias", bias=p[n + ".bias"])
        blocks = []
        x, r, first = seqs, None, True                       # the next layer norm reads (x + r) * (log_seqs != 0)
        for n in range(self.num_blocks):
            a, f = "attention_layers.%d." % n, "forward_layers.%d." % n
            S = x if first else torch.empty_like(x)
            Q, mu_a, rs_a = k.affine_layer_norm_fwd(x, p["attention_layernorms.%d.weight" % n], p["attention_layernorms.%d.bias" % n],
                                                    LN_EPS, r=r, row_ids=None if first else ids, sum_out=None if first else S)
            q, kk, v = lin(Q, a + "Q_w"), lin(S, a + "K_w"), lin(S, a + "V_w")
            st = [streams.get(s, 0) for s in ("att%d" % n, "pos_k", "pos_v", "time_k", "time_v")]
            M, lse = k.tisas_attn_fwd(q, kk, v, tables, tm, log_seqs, H, scale, probs, seed, st, status=self.status)
            T2 = torch.empty_like(Q)
            U, mu_f, rs_f = k.affine_layer_norm_fwd(Q, p["forward_layernorms.%d.weight" % n], p["forward_layernorms.%d.bias" % n],
                                                    LN_EPS, r=M, sum_out=T2)
            h = k.gemm(U, p[f + "conv1.weight"], ws, epilogue="bias_relu", bias=p[f + "conv1.bias"])
            if on:
                k.dropout(h, rate, seed, streams["ffn1_%d" % n], step_stride=self.streams_per_step)
            ff = lin(h, f + "conv2")
            if on:
                k.dropout(ff, rate, seed, streams["ffn2_%d" % n], step_stride=self.streams_per_step)
            blocks.append(dict(Q=Q, S=S, mu_a=mu_a, rs_a=rs_a, first=first, q=q, k=kk, v=v, lse=lse, st=st, U=U, T2=T2, mu_f=mu_f,
                               rs_f=rs_f, h=h))
            x, r, first = ff, U, False
        T3 = torch.empty_like(x)
        feats, mu_l, rs_l = k.affine_layer_norm_fwd(x, p["last_layernorm.weight"], p["last_layernorm.bias"], LN_EPS, r=r,
                                                    row_ids=ids, sum_out=T3)
        if keep is not None:
            keep.update(B=B, L=L, ids=ids, tm=tm, log_seqs=log_seqs, tables=tables, scale=scale, probs=probs, blocks=blocks, T3=T3,
                        mu_l=mu_l, rs_l=rs_l, on=on, streams=streams)
        return feats, B, L

    def forward(self, log_seqs, time_matrices, item_indices=None, pos_seqs=None, neg_seqs=None):
        """net.py:291-309.  Train mode draws the masks the next train_step would."""
        k = self.k
        streams = self.dropout_streams(self.step_count + 1) if self.training else {}
        feats, B, L = self._seq2feats(log_seqs, time_matrices, streams)
        D = self.hidden_units
        if item_indices is not None:
            cand, _ = k.emb_gather(item_indices[0].contiguous().view(-1), self.emb, 0, status=self.status)
            return k.gemm(feats.view(B, L * D)[:, (L - 1) * D:], cand, self.ws, trans_b=True)      # [B, I]
        out = k.tisas_head(feats, pos_seqs.contiguous().view(-1), neg_seqs.contiguous().view(-1), self.emb, status=self.status)
        return out[5].view(B, L), out[6].view(B, L)

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, log_seqs, time_matrices, pos_seqs, neg_seqs, lr=0.001):
        """dygraph_model.py:74-83 train_forward + backward + Adam -> (loss: a TiSASLoss, log_feats [B, L, D])."""
        k, p, g, ws = self.k, self.params, self.flat.view["g"], self.ws
        self.step_count += 1
        streams = self.dropout_streams(self.step_count) if self.training else {}
        sv = {}
        feats, B, L = self._seq2feats(log_seqs, time_matrices, streams, keep=sv)
        D, H, rate, seed, n = self.hidden_units, self.num_heads, self.dropout_rate, self.dropout_seed, B * L
        for t, name in ((pos_seqs, "pos_seqs"), (neg_seqs, "neg_seqs")):
            if tuple(t.shape) != (B, L) or t.dtype != torch.int64:
                raise ValueError("%s must be int64 [B, L], got %s %s" % (name, t.dtype, tuple(t.shape)))
        pos, neg, ids = pos_seqs.contiguous().view(-1), neg_seqs.contiguous().view(-1), sv["ids"]
        # ONE buffer for the table's three gradient sources: sequence | pos | neg
        G = torch.empty(3 * n, D, dtype=torch.float32, device=self.device)
        loss2, dx = k.tisas_head(feats, pos, neg, self.emb, status=self.status, d_pos_rows=G[n:2 * n], d_neg_rows=G[2 * n:])[:2]
        ln_bwd = lambda t, mu, rs, name, dy, **kw: k.affine_layer_norm_bwd(t, mu, rs, p[name + ".weight"], dy, g[name + ".weight"],
                                                                          g[name + ".bias"], **kw)
        lin_bwd = lambda name, x, dy: k.linear_backward(x, dy, p[name + ".weight"], ws, g[name + ".weight"], g[name + ".bias"])
        dx = ln_bwd(sv["T3"], sv["mu_l"], sv["rs_l"], "last_layernorm", dx, row_ids=ids, out=dx)   # d(ff) = d(U) of the last block
        d_tables = self._tables(L, "g")
        for tname in ("abs_pos_K_emb.weight", "abs_pos_V_emb.weight"):
            g[tname][L:].zero_()                             # positions behind this batch's length take no gradient
        for nb in reversed(range(self.num_blocks)):
            b = sv["blocks"][nb]
            a, f = "attention_layers.%d." % nb, "forward_layers.%d." % nb
            df = dx
            if sv["on"]:
                df = k.dropout(dx, rate, seed, streams["ffn2_%d" % nb], out=torch.empty_like(dx), step_stride=self.streams_per_step)
            dh = lin_bwd(f + "conv2", b["h"], df)
            if sv["on"]:
                k.dropout(dh, rate, seed, streams["ffn1_%d" % nb], step_stride=self.streams_per_step)
            k.relu_mask_(dh, b["h"])
            dU = lin_bwd(f + "conv1", b["U"], dh)
            dT2 = ln_bwd(b["T2"], b["mu_f"], b["rs_f"], "forward_layernorms.%d" % nb, dU, dy2=dx, out=dU)   # d(Q) = d(attention)
            dq, dk, dv = k.tisas_attn_bwd(b["q"], b["k"], b["v"], sv["tables"], sv["tm"], sv["log_seqs"], H, sv["scale"], b["lse"],
                                          dT2, d_tables, sv["probs"], seed, b["st"], accumulate=nb != self.num_blocks - 1,
                                          scratch=self._scratch)
            dQ = lin_bwd(a + "Q_w", b["Q"], dq)
            dSk, dSv = lin_bwd(a + "K_w", b["S"], dk), lin_bwd(a + "V_w", b["S"], dv)
            dx = ln_bwd(b["S"], b["mu_a"], b["rs_a"], "attention_layernorms.%d" % nb, dQ, dy2=dT2, e1=dSk, e2=dSv,
                        row_ids=None if b["first"] else ids, out=dQ)
        k.tisas_embed_bwd(ids, dx, self.item_num + 1, math.sqrt(D), rate if sv["on"] else 0.0, seed, streams.get("emb", 0), out=G[:n])
        fl = self.flat.flat
        k.adam_dense(fl["p"], fl["m"], fl["v"], fl["g"], self.step_count, lr, BETA1, BETA2, ADAM_EPS)
        rows = torch.cat([ids, pos, neg])
        self._last = dict(G=G, rows=rows)
        # every lookup went through the padding Embedding: id 0 takes no gradient
        groups = self._grouped("emb", rows, self.item_num + 1, 0, self._group_status)
        self._pp = k.segment_partials(groups, G, D, out=self._pp)
        k.adam_rows_all(groups, G, 1, self.emb, self.emb_m, self.emb_v, self.step_count, lr, BETA1, BETA2, ADAM_EPS,
                        partials=self._pp)
        return TiSASLoss(loss2), feats.view(B, L, D)

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}; the table's dense gradient is rebuilt with
        torch from the step's gradient rows (for inspection, not on the step's path)."""
        out = {k: v.clone() for k, v in self._shown("g").items() if v is not None}
        rows, G = self._last["rows"], self._last["G"]
        keep = rows != 0
        out["item_emb.weight"] = torch.zeros_like(self.emb).index_add_(0, rows[keep], G[keep])
        return out


class DygraphModel:
    """tisas/dygraph_model.py — same method names; tensors are torch device tensors.  infer_summary(): infer.py's NDCG@10 and
    HR@10 of the batches seen since the last call."""

    def __init__(self):
        self._ndcg = self._hr = self._users = 0.0

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return TiSASRecLayer(g("hyper_parameters.num_users"), g("hyper_parameters.num_items"), g("hyper_parameters.hidden_units"),
                             g("hyper_parameters.maxlen"), g("hyper_parameters.time_span"), g("hyper_parameters.num_blocks"),
                             g("hyper_parameters.num_heads"), device=device, kernels=kernels,
                             dropout_seed=g("runner.seed", 12345))

    def create_feeds(self, batch_data, device="cuda"):
        return [torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).to(device).to(torch.int64).contiguous()
                for b in batch_data]

    def create_loss(self, prediction, mask):
        """dygraph_model.py:42-53 on (pos_logits, neg_logits) and the mask, with torch (train_forward takes the loss from
        rec_tisas_head instead)."""
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        pl, nl = prediction[0][mask], prediction[1][mask]
        return bce(pl, torch.ones_like(pl)) + bce(nl, torch.zeros_like(nl))

    def create_optimizer(self, dy_model, config):
        return None                                      # Adam is part of train_step (rec_adam_dense, rec_adam_rows_all)

    def create_metrics(self, device="cuda"):
        return [], []

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        seq, tm, pos, neg = self.create_feeds(batch_data, dy_model.device)
        loss, _ = dy_model.train_step(seq, tm, pos, neg, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        seq, tm, item_idx = self.create_feeds(batch_data, dy_model.device)
        was = dy_model.training
        dy_model.eval()
        logits = dy_model.forward(seq, tm, item_idx)
        dy_model.training = was
        # infer.py: the rank of candidate 0 in the batch's row 0
        rank = int((-logits[0]).argsort().argsort()[0].item())
        self._users += 1
        if rank < 10:
            self._ndcg += 1.0 / math.log2(rank + 2)
            self._hr += 1
        return metrics_list, {"user": seq, "prediction": logits}

    def infer_summary(self):
        n = max(self._users, 1.0)
        vals = {"NDCG@10": self._ndcg / n, "HR@10": self._hr / n}
        self._ndcg = self._hr = self._users = 0.0
        return vals
