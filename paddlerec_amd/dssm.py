"""Host-side mirror of the reference's DSSM plugin (models/match/dssm/net.py DSSMLayer; dygraph_model.py) on the recengine HIP
kernels: the two-tower semantic-matching net over bags of letter trigrams.

A tower input is a float vector of trigram_d = 2 900 entries of which a dozen are set.  The reference feeds it dense, so its
first Linear multiplies by a matrix that is more than 99.5 % zeros, and that layer is 87 % of a tower's multiply-adds.  A step
here is, on the sparse route (feeds in CSR):

  * rec_dssm_sparse_linear_fwd per tower: layer 0 as a sum of the weight rows a sample names; the document tower runs ONCE
    over the (1 + neg) B stacked rows, not 1 + neg times;
  * rec_gemm_f32 with its BIAS / BIAS_RELU epilogue per later Linear;
  * rec_dssm_head_step: the 1 + neg cosines, the softmax, -log of the positive's share, their mean over the first
    min(B, slice_end) rows and dq / dd (the last ReLU's mask folded in) in one launch plus a one-wave fold;
  * rec_gemm_f32_pair per later Linear on the way back; for layer 0 rec_colsum (the bias) and, per tower, rec_dssm_lod_rows,
    rec_ids_group (both skipped where the reader's batch carries row_of and the grouping: reader.dssm_group) and
    rec_dssm_sparse_linear_bwd: the weight gradient from the touched rows alone, every row written;
  * one rec_adam_dense over the flat buffer (Paddle's Adam is not lazy: every weight moves every step).
The general route takes the reference's dense [B, trigram_d] feeds and runs layer 0 on rec_gemm_f32 and its weight-gradient
form; REC_DSSM_SPARSE=0 sends CSR feeds there by densifying them with torch ahead of the step (tests and the benchmark)."""
import math
import os
import types

import numpy as np
import torch

from .net_base import FlatStore, LayerBase

TOWERS = ("query", "pos")
QUIRKS = ("forward reads self._query_layers[-2].bias, which exists only when the entry before the last of the Linear / ReLU "
          "list is a Linear: the mirror refuses the configurations the reference raises on; neg_num is read from the YAML and "
          "never used, the number of negatives is len(input_data) - 2; positives and negatives all run through the pos_linear "
          "tower; weights AND biases are drawn XavierNormal(fan_in, fan_out); hit_prob is prob[0:slice_end, 0:1], so the rows at "
          "or beyond slice_end run their towers but add nothing to the loss and get a zero gradient, and the mean is over "
          "min(B, slice_end) rows; cosine_similarity clamps w1 * w2 at eps^2 = 1e-16, so a tower output that ReLU zeroed "
          "entirely has cosine 0 and hands the other vector / 1e-8 back as its gradient; infer returns ones [slice_end, 1] as "
          "its second value")


def layer_kinds(fc_sizes, fc_acts):
    """The reference's list of sublayers of one tower, as "linear" / "relu" (net.py:30-48).  ValueError where the reference
    itself raises: fc_acts shorter than fc_sizes (IndexError there), or no Linear at [-2] (net.py:81)."""
    fc_sizes, fc_acts = list(fc_sizes), list(fc_acts)
    if not fc_sizes:
        raise ValueError("DSSM: fc_sizes is empty")
    if len(fc_acts) < len(fc_sizes):
        raise ValueError("DSSM: fc_acts (%d entries) is shorter than fc_sizes (%d): the reference indexes past its end"
                         % (len(fc_acts), len(fc_sizes)))
    kinds = []
    for i in range(len(fc_sizes)):
        kinds.append("linear")
        if fc_acts[i] == "relu":
            kinds.append("relu")
    if len(kinds) < 2 or kinds[-2] != "linear":
        raise ValueError("DSSM: the reference reads _query_layers[-2].bias (net.py:81) and the layer list %s has %s there"
                         % (kinds, "no entry" if len(kinds) < 2 else "a ReLU"))
    return kinds


def _is_csr(x):
    return isinstance(x, (tuple, list))


class DSSMLayer(LayerBase):
    """net.py:21-101.  forward(inputs, is_infer) -> (R_Q_D_p [B, 1], hit_prob [min(B, slice_end), 1]) or, for inference,
    (R_Q_D_p, ones [slice_end, 1]);  train_step(inputs, lr) -> loss [1].

    inputs, sparse route: [query, docs], each a CSR tuple (cols int64 [nnz], vals float32 [nnz], lod int64 [rows + 1]),
    optionally followed by row_of int32 [nnz], optionally followed by the entries grouped by column as reader.dssm_group
    makes them (sorted_pos, uniq_rows, seg_offset, n_uniq: rec_ids_group's outputs) — what a feed lacks is made on the device;
    docs holds the (1 + neg) B document rows field-major (the B positives first).
    inputs, general route: the reference's list [query, doc_pos, doc_neg_0, ...] of dense [B, trigram_d] tensors."""

    def __init__(self, trigram_d, neg_num, slice_end, hidden_layers, hidden_acts, device="cuda", kernels=None):
        layer_kinds(hidden_layers, hidden_acts)
        self._init_runtime(device, kernels, group_status=True)
        self.trigram_d, self.neg_num, self.slice_end = int(trigram_d), neg_num, int(slice_end)
        self.h = [self.trigram_d] + [int(x) for x in hidden_layers]
        self.relu = [a == "relu" for a in list(hidden_acts)[:len(hidden_layers)]]
        self.nl = len(self.h) - 1
        if min(self.h) < 1 or self.slice_end < 1:
            raise ValueError("DSSM: trigram_d, every fc size and slice_end must be positive")
        if self.h[1] > self.k.DSSM_MAX_WIDTH:
            raise ValueError("DSSM: fc_sizes[0] = %d above the sparse layer's %d" % (self.h[1], self.k.DSSM_MAX_WIDTH))
        entries = []
        for t in TOWERS:
            for i in range(self.nl):
                entries += [("%s_linear_%d.weight" % (t, i), (self.h[i], self.h[i + 1])),
                            ("%s_linear_%d.bias" % (t, i), (self.h[i + 1],))]
        self.store = FlatStore(entries, self.device)
        self.flat = self.store.flat
        self.sparse_default = os.environ.get("REC_DSSM_SPARSE", "1") != "0"
        self._head, self._row_of = {}, {}
        self._init()

    # ---------------------------------------------------------------- parameters
    def _init(self):
        """net.py:35-42: XavierNormal(fan_in, fan_out) — std sqrt(2 / (fan_in + fan_out)) — for the weight and the bias."""
        for name, t in self.store.view["p"].items():
            i = int(name.split("_")[2].split(".")[0])
            t.copy_(torch.randn(t.shape, device=self.device) * math.sqrt(2.0 / (self.h[i] + self.h[i + 1])))

    def state_dict(self):
        return self.store.view["p"]

    def moments(self):
        return self.store.view["m"], self.store.view["v"]

    def load_state_dict(self, sd):
        self.set_dict(sd)

    def _optimizer_views(self):
        return {"dssm.%s.%s" % (s, k): v for s in ("m", "v") for k, v in self.store.view[s].items()}

    # ---------------------------------------------------------------- feeds
    def _csr(self, x, name):
        if len(x) not in (3, 4, 8):
            raise ValueError("%s must be (cols, vals, lod), (cols, vals, lod, row_of) or those four and reader.dssm_group's four"
                             % name)
        cols, vals, lod = x[0].reshape(-1), x[1].reshape(-1), x[2].reshape(-1)
        if cols.dtype != torch.int64 or lod.dtype != torch.int64 or vals.dtype != torch.float32:
            raise ValueError("%s: cols and lod must be int64 and vals float32" % name)
        if lod.numel() < 1 or cols.numel() != vals.numel():
            raise ValueError("%s: cols and vals must have one entry each and lod rows + 1" % name)
        groups = None
        if len(x) == 8:
            groups = types.SimpleNamespace(n=cols.numel(), sorted_pos=x[4], uniq_rows=x[5], seg_offset=x[6], n_uniq=x[7])
        return cols.contiguous(), vals.contiguous(), lod.contiguous(), (x[3] if len(x) > 3 else None), groups

    def _densify(self, csr):
        """[rows, trigram_d] of a CSR feed with torch (REC_DSSM_SPARSE=0 only; an out-of-range column is an error there)."""
        cols, vals, lod = csr[:3]
        R = lod.numel() - 1
        rows = torch.repeat_interleave(torch.arange(R, device=lod.device), lod[1:] - lod[:-1])
        n = rows.numel()                                       # lod may have been cut to the positives (inference)
        return torch.zeros(R, self.trigram_d, dtype=torch.float32, device=self.device).index_put_((rows, cols[:n]), vals[:n],
                                                                                                  accumulate=True)

    def _inputs(self, inputs, is_infer):
        """-> (sparse, query, docs, B, docs_per_sample): _csr's records or dense matrices; inference keeps the positives."""
        if len(inputs) < 2:
            raise ValueError("DSSM: inputs must hold the query and the positive document")
        if _is_csr(inputs[0]):
            if len(inputs) != 2:
                raise ValueError("DSSM: CSR feeds are [query, docs]")
            q, d = self._csr(inputs[0], "query"), self._csr(inputs[1], "docs")
            B, R = q[2].numel() - 1, d[2].numel() - 1
            if B < 1 or R % B or R < B:
                raise ValueError("DSSM: docs holds %d rows, not a positive multiple of the %d queries" % (R, B))
            if is_infer and R > B:
                d = (d[0], d[1], d[2][:B + 1].contiguous(), None, None)
            n = 1 if is_infer else R // B
            if not self.sparse_default:
                return False, self._densify(q), self._densify(d), B, n
            return True, q, d, B, n
        xs = [x.reshape(-1, self.trigram_d).to(torch.float32) for x in (inputs[:2] if is_infer else inputs)]
        B = xs[0].shape[0]
        if B < 1 or any(x.shape[0] != B for x in xs):
            raise ValueError("DSSM: every input must be [B, trigram_d] with one B")
        return False, xs[0].contiguous(), (xs[1].contiguous() if len(xs) == 2 else torch.cat(xs[1:], 0)), B, len(xs) - 1

    # ---------------------------------------------------------------- towers
    def _tower_fwd(self, tower, sparse, x):
        """-> acts: acts[i] = the output of layer i (after its ReLU where it has one)."""
        k, p = self.k, self.store.view["p"]
        acts = []
        for i in range(self.nl):
            W, b = p["%s_linear_%d.weight" % (tower, i)], p["%s_linear_%d.bias" % (tower, i)]
            if i == 0 and sparse:
                y = k.dssm_sparse_linear_fwd(x[0], x[1], x[2], W, b, relu=self.relu[0], status=self.status)
            else:
                y = k.gemm(x if i == 0 else acts[-1], W, self.ws, epilogue="bias_relu" if self.relu[i] else "bias", bias=b)
            acts.append(y)
        return acts

    def _tower_bwd(self, tower, sparse, x, acts, d):
        """d: the gradient of the tower's output, already masked by the last ReLU."""
        k, p, g = self.k, self.store.view["p"], self.store.view["g"]
        for i in range(self.nl - 1, 0, -1):
            d = k.linear_backward(acts[i - 1], d, p["%s_linear_%d.weight" % (tower, i)], self.ws,
                                  g["%s_linear_%d.weight" % (tower, i)], g["%s_linear_%d.bias" % (tower, i)],
                                  relu_src=acts[i - 1] if self.relu[i - 1] else None)
        gW, gb = g["%s_linear_0.weight" % tower], g["%s_linear_0.bias" % tower]
        if not sparse:
            k.gemm(x, d, self.ws, trans_a=True, out=gW, b_colsum=gb)
            return
        cols, vals, lod, row_of, groups = x
        nnz = cols.numel()
        if row_of is None:
            row_of = self._row_of.get(tower)
            if row_of is None or row_of.numel() < nnz:
                row_of = self._row_of[tower] = torch.empty(max(nnz, 1), dtype=torch.int32, device=self.device)
            k.dssm_lod_rows(lod, nnz, out=row_of)
        k.colsum(d, self.ws, out=gb)
        if groups is None:
            groups = self._grouped(tower, cols, self.trigram_d, None, self._group_status) if nnz else self.k.IdGroups(0, self.device)
        k.dssm_sparse_linear_bwd(vals, row_of, groups, d, gW)

    # ---------------------------------------------------------------- forward
    def forward(self, inputs, is_infer=False):
        """net.py:70-101."""
        sparse, q, d, B, n = self._inputs(inputs, is_infer)
        qa, da = self._tower_fwd("query", sparse, q), self._tower_fwd("pos", sparse, d)
        if is_infer:
            cos = self.k.dssm_cos(qa[-1], da[-1])
            return cos.view(-1, 1), torch.ones(self.slice_end, 1, dtype=torch.float32, device=self.device)
        head = self.k.dssm_head_step(qa[-1], da[-1], self.slice_end, relu_mask=self.relu[-1])
        return head["cos"][:, :1], head["hit_prob"][:min(B, self.slice_end)].view(-1, 1)

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, inputs, lr=0.001):
        """dygraph_model.py:76-84 and the trainer's backward / Adam step -> loss [1]."""
        k, fl = self.k, self.flat
        sparse, q, d, B, n = self._inputs(inputs, False)
        if n > k.DSSM_MAX_DOCS:
            raise ValueError("DSSM: %d documents per query above the head kernel's %d" % (n, k.DSSM_MAX_DOCS))
        self.step_count += 1
        qa, da = self._tower_fwd("query", sparse, q), self._tower_fwd("pos", sparse, d)
        key = (B, n)
        head = self._head[key] = k.dssm_head_step(qa[-1], da[-1], self.slice_end, relu_mask=self.relu[-1],
                                                  out=self._head.get(key))
        if len(self._head) > 4:
            self._head.pop(next(iter(self._head)))
        self._tower_bwd("query", sparse, q, qa, head["dq"])
        self._tower_bwd("pos", sparse, d, da, head["dd"])
        k.adam_dense(fl["p"], fl["m"], fl["v"], fl["g"], self.step_count, lr=lr)
        self._last = dict(head=head, B=B, docs=n, sparse=sparse)
        return head["loss"]

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}."""
        return {n: v.clone() for n, v in self.store.view["g"].items()}

    def last_outputs(self):
        """cos [B, 1 + neg] and hit_prob [min(B, slice_end), 1] of the newest train_step."""
        L = self._last
        return L["head"]["cos"], L["head"]["hit_prob"][:min(L["B"], self.slice_end)].view(-1, 1)


class DygraphModel:
    """dssm/dygraph_model.py — same method names; tensors are torch device tensors.  infer_summary(): the mean query_doc_sim
    over the lines seen since the last call (`sims` keeps every line's, in file order, until then)."""

    def __init__(self):
        self.sims = []

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return DSSMLayer(g("hyper_parameters.trigram_d"), g("hyper_parameters.neg_num"), g("hyper_parameters.slice_end"),
                         g("hyper_parameters.fc_sizes"), g("hyper_parameters.fc_acts"), device=device, kernels=kernels)

    @staticmethod
    def _to(x, device, dtype):
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x))
        return x.to(device).to(dtype)

    def _feeds(self, batch_data, trigram_d, device, fields):
        if _is_csr(batch_data[0]):                             # reader.DssmReader's CSR batch: [query, docs]
            dt = (torch.int64, torch.float32, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32)
            return [tuple(self._to(t, device, dt[i]) for i, t in enumerate(x)) for x in batch_data[:2]]
        return [self._to(b, device, torch.float32).reshape(-1, trigram_d) for b in (batch_data if fields is None
                                                                                    else batch_data[:fields])]

    def create_feeds_train(self, batch_data, trigram_d, device="cuda"):
        """dygraph_model.py:36-46: [query, doc_pos, doc_negs...] as float32 [B, trigram_d]; a CSR batch passes through."""
        return self._feeds(batch_data, trigram_d, device, None)

    def create_feeds_infer(self, batch_data, trigram_d, device="cuda"):
        """dygraph_model.py:48-53: the first two fields."""
        return self._feeds(batch_data, trigram_d, device, 2)

    def create_loss(self, hit_prob):
        """dygraph_model.py:56-59 with torch (train_forward takes the loss from the step's kernels)."""
        return (-torch.sum(torch.log(hit_prob), dim=-1)).mean()

    def create_optimizer(self, dy_model, config):
        return None                                          # Adam is part of train_step

    def create_metrics(self, device="cuda"):
        return [], []

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        inputs = self.create_feeds_train(batch_data, config.get("hyper_parameters.trigram_d"), dy_model.device)
        loss = dy_model.train_step(inputs, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        inputs = self.create_feeds_infer(batch_data, config.get("hyper_parameters.trigram_d"), dy_model.device)
        sim, _ = dy_model.forward(inputs, True)
        self.sims.append(sim.reshape(-1))
        return metrics_list, {"query_doc_sim": sim}

    def infer_summary(self):
        if not self.sims:
            return {"query_doc_sim": 0.0}
        sims, self.sims = torch.cat(self.sims), []
        return {"query_doc_sim": float(sims.double().mean().item())}
