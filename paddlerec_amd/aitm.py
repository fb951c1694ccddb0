"""Host-side mirror of the reference's AITM plugin (models/multitask/aitm/net.py:19-115 Tower, Attention, AITM;
dygraph_model.py) on the recengine HIP kernels: one embedding table per field, two towers (click, conversion), the adaptive
information transfer (AIT) block from the click tower to the conversion task, two sigmoid heads.

  * tables: the F tables of very different sizes are ONE buffer [sum(vocab), D] with field_begin [F + 1];
    rec_field_gather_fwd checks an id against its OWN field's size (an id past its table but inside the buffer is flagged,
    reads nothing and gives a zero row) and writes the [B, F*D] feature rows the first GEMM reads, and the global rows
    (-1 for a refused id) the backward groups: ids_group(rows) -> segment_partials -> adam_rows_all(l2) is the reference's
    dygraph Adam with weight_decay on the dense gradient of every table.  state_dict shows embedding_dict.{i}.weight as
    [vocab_i, D] row ranges of the buffer;
  * the towers' first Linears both read the features: they are the column ranges of ONE packed image [F*D, 2 dims[0]], so
    the forward is one GEMM (bias + ReLU) and the backward one dW and one dX GEMM (esmm.py); later layers are per tower.
    The conversion tower's last layer and info_layer write straight into the two token rows of ONE buffer [B, 2, 32]
    (token 0 the conversion tower, token 1 info) through a row stride: net.py:104-110's unsqueeze + concat without a copy;
  * Q, K, V are ONE [2B, 32] x [32, 96] GEMM (no bias), then rec_ait_fwd and rec_aitm_head: both heads' dots, sigmoids, the
    two BCE terms, the hinge and d(logits) in one launch.  Backward: the heads' dW / db / d(act) (GEMMs with one column),
    rec_ait_bwd, one rec_gemm_f32_pair over the packed QKV image, the towers (Dropout with the same mask streams, then the
    ReLU mask), one pair for the packed first layer;
  * Adam (beta 0.9 / 0.999, epsilon 1e-8, non-lazy) with the coupled L2 term g + 1e-6 w on EVERY parameter: l2_decay_grad
    over the flat gradient and one rec_adam_dense for the dense parameters, adam_rows_all(l2=1e-6) for the tables.
Names are the reference's: embedding_dict.{i}.weight, click_tower.layer.{0,3,6}, conversion_tower.layer.{0,3,6},
attention_layer.{q,k,v}_layer.weight, info_layer.0, click_layer.0, conversion_layer.0."""
import math

import torch

from .mtl import ADAM_EPS, BETA1, BETA2, STORES, LazyLoss
from .net_base import FlatStore, LayerBase, auc_metrics

NUM_THRESHOLDS = 100000                  # dygraph_model.py:71-73: paddle.metric.Auc("ROC", num_thresholds=100000)
CONSTRAINT_WEIGHT, WEIGHT_DECAY, INFO_DIM = 0.6, 1e-6, 32
SITES = ("l0", "click1", "click2", "conv1", "conv2", "info")   # the Dropout sites, in mask-stream order

QUIRKS = ("info_layer's output width is hard-coded to 32 (net.py:83) while the attention is built for dims[-1], so dims[-1] "
          "must be 32: anything else fails in the reference's concat and is refused here; feature_names = sorted(...) "
          "(net.py:71) is computed and never used: table i belongs to the i-th entry of hyper_parameters.feature_vocabulary "
          "in CONFIG order, which is the CSV's column order, and there is no padding id (id 0 is a trained row); the "
          "attention scores are each token's own <Q_t, K_t> / sqrt(d) (net.py:57), not a cross-token product, and its "
          "three Linears have no bias; the loss is mean BCE(pCTR, click) + mean BCE(pCVR, buy) + 0.6 * SUM over the batch "
          "of max(pCVR - pCTR, 0): constraint_weight 0.6 is a Python default (dygraph_model.py:46), not a YAML key, and the "
          "hinge is a batch sum beside two means; binary_cross_entropy clamps the log at -100 and floors p (1 - p) at 1e-12 "
          "in its gradient [EXT]; the hinge passes its gradient where pCVR > pCTR strictly, a tie carries none (Paddle's "
          "maximum splits a tie's gradient [EXT]; exact ties do not occur in float32 training and are kept out of the "
          "fixtures); Adam(weight_decay=1e-6) is the coupled L2 term g + 1e-6 w [EXT] on every parameter, biases and all "
          "table rows included, non-lazy: every row of every table moves every step; the reader reads only file_list[0] and "
          "skips its header line; both AUCs use 100000 thresholds; Dropout is off in eval mode and uses the engine's "
          "counter-based masks in train mode; Linear and Embedding weights are XavierUniform with zero bias, Paddle's "
          "defaults [EXT] (drawn with torch, not Paddle's random stream); the learning rate is "
          "hyper_parameters.optimizer.learning_rate (default 1e-4)")


class AitmLoss(LazyLoss):
    """The step's loss of cost [B, 3] (BCE click, BCE buy, hinge): mean + mean + constraint_weight * SUM, reduced (torch) when
    it is read."""

    def __init__(self, cost, constraint_weight):
        super().__init__(cost)
        self.constraint_weight = float(constraint_weight)

    def value(self):
        if self._v is None:
            c = self.cost
            self._v = (c[:, 0].mean() + c[:, 1].mean() + self.constraint_weight * c[:, 2].sum()).reshape(1)
        return self._v


def _xavier(t):
    lim = math.sqrt(6.0 / (t.shape[0] + t.shape[1]))
    t.uniform_(-lim, lim)


class AITMLayer(LayerBase):
    """aitm/net.py:63-115.  forward(ids [B, F] int64) -> (pCTR [B], pCVR [B]); train_step(ids, click [B], buy [B], lr) ->
    (loss, pred [B, 2] = pCTR | pCVR).  feature_vocabulary: [[name, size], ...] in the order of the ids' columns."""

    def __init__(self, feature_vocabulary, embedding_size, tower_dims=(128, 64, 32), drop_prob=(0.1, 0.3, 0.3),
                 constraint_weight=CONSTRAINT_WEIGHT, device="cuda", kernels=None, dropout_seed=12345):
        self._init_runtime(device, kernels)
        pairs = list(feature_vocabulary.items()) if isinstance(feature_vocabulary, dict) else [tuple(p) for p in feature_vocabulary]
        self.feature_names = [str(n) for n, _ in pairs]       # config order; net.py:71's sorted copy is never used
        self.vocab = [int(s) for _, s in pairs]
        self.dims, self.drop_prob = [int(h) for h in tower_dims], [float(p) for p in drop_prob]
        D = self.embedding_size = int(embedding_size)
        if not self.vocab or min(self.vocab) < 1 or D < 1:
            raise ValueError("AITM: feature_vocabulary must hold positive sizes and embedding_size must be positive")
        if len(self.dims) != 3 or len(self.drop_prob) != 3 or min(self.dims) < 1:
            raise ValueError("AITM: dims and drop_prob must hold three entries (net.py:26-34 builds three layers)")
        if any(not 0.0 <= p < 1.0 for p in self.drop_prob):
            raise ValueError("AITM: drop_prob must be in [0, 1)")
        if self.dims[-1] != INFO_DIM:
            raise ValueError("AITM: dims[-1] must be 32, got %d — info_layer is Linear(dims[-1], 32) (net.py:83) and its output "
                             "is concatenated with the conversion tower's" % self.dims[-1])
        self.constraint_weight, self.dropout_seed = float(constraint_weight), int(dropout_seed)
        F, d = len(self.vocab), INFO_DIM
        self.num_fields, self.K = F, F * D
        begin = [0]
        for n in self.vocab:
            begin.append(begin[-1] + n)
        self.num_rows = begin[-1]
        self.field_begin_host = begin
        self.field_begin = torch.tensor(begin, dtype=torch.int64, device=self.device)
        self.emb = torch.empty(self.num_rows, D, dtype=torch.float32, device=self.device)
        self.emb_m, self.emb_v = torch.zeros_like(self.emb), torch.zeros_like(self.emb)
        h0, h1, _ = self.dims
        entries = [("W0", (self.K, 2 * h0)), ("b0", (2 * h0,))]
        for t in ("click_tower", "conversion_tower"):
            entries += [(t + ".layer.3.weight", (h0, h1)), (t + ".layer.3.bias", (h1,)),
                        (t + ".layer.6.weight", (h1, d)), (t + ".layer.6.bias", (d,))]
        entries += [("Wqkv", (d, 3 * d)), ("info_layer.0.weight", (d, d)), ("info_layer.0.bias", (d,)),
                    ("click_layer.0.weight", (d, 1)), ("click_layer.0.bias", (1,)),
                    ("conversion_layer.0.weight", (d, 1)), ("conversion_layer.0.bias", (1,))]
        self.flat = FlatStore(entries, self.device)
        self._views = {s: {} for s in STORES}
        for s in STORES:
            v, o = self.flat.view[s], self._views[s]
            for i, t in enumerate(("click_tower", "conversion_tower")):
                o[t + ".layer.0.weight"], o[t + ".layer.0.bias"] = v["W0"][:, i * h0:(i + 1) * h0], v["b0"][i * h0:(i + 1) * h0]
                for j in (3, 6):
                    for x in ("weight", "bias"):
                        o["%s.layer.%d.%s" % (t, j, x)] = v["%s.layer.%d.%s" % (t, j, x)]
            for i, n in enumerate("qkv"):
                o["attention_layer.%s_layer.weight" % n] = v["Wqkv"][:, i * d:(i + 1) * d]
            for name, _ in entries[-6:]:
                o[name] = v[name]
        self.params = self._views["p"]
        for i in range(F):                                     # Paddle's defaults: XavierUniform, zero bias
            _xavier(self.emb[begin[i]:begin[i + 1]])
        for name, w in self.params.items():
            if name.endswith(".weight"):
                _xavier(w)
        self._pp = None

    # ---------------------------------------------------------------- parameters
    def _table_views(self, t):
        b = self.field_begin_host
        return {"embedding_dict.%d.weight" % i: t[b[i]:b[i + 1]] for i in range(self.num_fields)}

    def state_dict(self):
        sd = self._table_views(self.emb)
        sd.update(self.params)
        return sd

    def _optimizer_views(self):
        """Adam's moments of every parameter, under the parameter's own name."""
        out = {}
        for s, t in (("m", self.emb_m), ("v", self.emb_v)):
            for k, v in dict(self._table_views(t), **self._views[s]).items():
                out["mtl.%s.%s" % (s, k)] = v
        return out

    # ---------------------------------------------------------------- dropout sites
    def dropout_streams(self, step):
        """{site: (mask stream, rate)} of training step `step` (1-based) for the sites whose rate is positive — "l0" (both
        towers' first layers: ONE pass over the packed image's [B, 2 dims[0]] output, click columns first), "click1",
        "click2", "conv1", "conv2" (each [B, dims[j]]) and "info" ([B, 32]); tests rebuild the masks from these with
        rec_dropout on ones."""
        base, out = step * len(SITES), {}
        rates = dict(l0=self.drop_prob[0], click1=self.drop_prob[1], click2=self.drop_prob[2], conv1=self.drop_prob[1],
                     conv2=self.drop_prob[2], info=self.drop_prob[2])
        for i, site in enumerate(SITES):
            if rates[site] > 0.0:
                out[site] = (base + i, rates[site])
        return out

    def _drop(self, x, streams, site):
        if site in streams:
            s, p = streams[site]
            self.k.dropout(x, p, self.dropout_seed, s, step_stride=len(SITES))

    # ---------------------------------------------------------------- forward
    def _check_ids(self, ids):
        if ids.dim() != 2 or ids.shape[1] != self.num_fields or ids.dtype != torch.int64:
            raise ValueError("expected ids int64 [B, %d], got %s %s" % (self.num_fields, ids.dtype, tuple(ids.shape)))

    def _run(self, ids, streams, keep=None):
        """-> (tower_click [B, 32], ait [B, 32]).  streams: {} (no dropout) or dropout_streams(step); keep: a dict that
        receives what the backward needs."""
        k, ws, p, v = self.k, self.ws, self.params, self.flat.view["p"]
        self._check_ids(ids)
        B, d = ids.shape[0], INFO_DIM
        h0 = self.dims[0]
        x, rows, _ = k.field_gather_fwd(ids, self.emb, self.field_begin, status=self.status)
        Y = k.gemm(x, v["W0"], ws, epilogue="bias_relu", bias=v["b0"])
        self._drop(Y, streams, "l0")
        # tok [B, 2 * 32] IS the AIT input [B, 2, 32]: token 0 the conversion tower, token 1 info, written through a row stride
        tok = torch.empty(B, 2 * d, dtype=torch.float32, device=self.device)
        tc = torch.empty(B, d, dtype=torch.float32, device=self.device)
        tv, info = tok[:, 0:d], tok[:, d:2 * d]
        mids = {}
        for i, (t, site, dst) in enumerate((("click_tower", "click", tc), ("conversion_tower", "conv", tv))):
            a1 = k.gemm(Y[:, i * h0:(i + 1) * h0], p[t + ".layer.3.weight"], ws, epilogue="bias_relu", bias=p[t + ".layer.3.bias"])
            self._drop(a1, streams, site + "1")
            k.gemm(a1, p[t + ".layer.6.weight"], ws, epilogue="bias_relu", bias=p[t + ".layer.6.bias"], out=dst)
            self._drop(dst, streams, site + "2")
            mids[t] = a1
        k.gemm(tc, p["info_layer.0.weight"], ws, epilogue="bias_relu", bias=p["info_layer.0.bias"], out=info)
        self._drop(info, streams, "info")
        X2 = tok.view(2 * B, d)
        QKV = k.gemm(X2, v["Wqkv"], ws)
        ait, prob = k.ait_fwd(QKV, 2)
        if keep is not None:
            keep.update(x=x, rows=rows, Y=Y, tc=tc, X2=X2, mids=mids, QKV=QKV, ait=ait, prob=prob, B=B)
        return tc, ait

    def predict(self, ids):
        """-> pred [B, 2] = pCTR | pCVR, Dropout off (eval mode)."""
        tc, ait = self._run(ids, {})
        p = self.params
        none = torch.zeros(ids.shape[0], dtype=torch.int64, device=self.device)
        return self.k.aitm_head(tc, ait, p["click_layer.0.weight"], p["click_layer.0.bias"], p["conversion_layer.0.weight"],
                                p["conversion_layer.0.bias"], none, none, self.constraint_weight, 1.0, want_grad=False)[0]

    def forward(self, ids):
        """net.py forward: ids [B, F] (the reference's list of F tensors [B], side by side) -> (click [B], conversion [B])."""
        pred = self.predict(ids)
        return pred[:, 0], pred[:, 1]

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, ids, click, buy, lr=1e-4):
        """dygraph_model.py train_forward + backward + Adam(weight_decay).  -> (loss: an AitmLoss, pred [B, 2])."""
        k, ws, p, g = self.k, self.ws, self.params, self._views["g"]
        self.step_count += 1
        streams = self.dropout_streams(self.step_count) if self.training else {}
        sv = {}
        tc, ait = self._run(ids, streams, keep=sv)
        B, d, h0 = sv["B"], INFO_DIM, self.dims[0]
        if tuple(click.shape) != (B,) or tuple(buy.shape) != (B,):
            raise ValueError("click and buy must be int64 [B], got %s and %s" % (tuple(click.shape), tuple(buy.shape)))
        pred, cost, dz = k.aitm_head(tc, ait, p["click_layer.0.weight"], p["click_layer.0.bias"], p["conversion_layer.0.weight"],
                                     p["conversion_layer.0.bias"], click, buy, self.constraint_weight, 1.0 / B)
        dz0, dz1 = dz[:, 0:1], dz[:, 1:2]
        # the two Linear(32, 1) heads: dW = act^T dz, db = sum dz, d(act) = dz w^T; tower_click sits behind a ReLU
        k.gemm(tc, dz0, ws, trans_a=True, out=g["click_layer.0.weight"], b_colsum=g["click_layer.0.bias"])
        k.gemm(ait, dz1, ws, trans_a=True, out=g["conversion_layer.0.weight"], b_colsum=g["conversion_layer.0.bias"])
        d_tc = k.gemm(dz0, p["click_layer.0.weight"], ws, trans_b=True, epilogue="relu_mask", aux0=tc)
        d_ait = k.gemm(dz1, p["conversion_layer.0.weight"], ws, trans_b=True)
        # AIT, then the packed Q | K | V image: dW and dX in one call; both tokens sit behind a ReLU
        dQKV = k.ait_bwd(sv["QKV"], sv["prob"], d_ait, 2)
        v = self.flat.view
        d_tok = k.linear_backward(sv["X2"], dQKV, v["p"]["Wqkv"], ws, v["g"]["Wqkv"], None, relu_src=sv["X2"]).view(B, 2 * d)
        d_tv, d_info = d_tok[:, 0:d], d_tok[:, d:2 * d]
        self._drop(d_info, streams, "info")
        d_tc2 = k.linear_backward(tc, d_info, p["info_layer.0.weight"], ws, g["info_layer.0.weight"], g["info_layer.0.bias"],
                                  relu_src=tc)
        k.bst_add(d_tc, d_tc2)                                   # tower_click feeds the click head and info_layer
        GY = torch.empty(B, 2 * h0, dtype=torch.float32, device=self.device)
        for i, (t, site, dt) in enumerate((("click_tower", "click", d_tc), ("conversion_tower", "conv", d_tv))):
            a0, a1 = sv["Y"][:, i * h0:(i + 1) * h0], sv["mids"][t]
            self._drop(dt, streams, site + "2")
            d1 = k.linear_backward(a1, dt, p[t + ".layer.6.weight"], ws, g[t + ".layer.6.weight"], g[t + ".layer.6.bias"],
                                   relu_src=a1)
            self._drop(d1, streams, site + "1")
            k.linear_backward(a0, d1, p[t + ".layer.3.weight"], ws, g[t + ".layer.3.weight"], g[t + ".layer.3.bias"],
                              relu_src=a0, out=GY[:, i * h0:(i + 1) * h0])
        self._drop(GY, streams, "l0")
        dX = k.linear_backward(sv["x"], GY, v["p"]["W0"], ws, v["g"]["W0"], v["g"]["b0"])
        self._last = dict(dz=dz, dX=dX, rows=sv["rows"], table=self.emb.clone() if self.keep_table_for_gradients else None)
        f = self.flat.flat
        k.l2_decay_grad(f["g"], f["p"], WEIGHT_DECAY)
        k.adam_dense(f["p"], f["m"], f["v"], f["g"], self.step_count, lr, BETA1, BETA2, ADAM_EPS)
        self._table_step(sv["rows"], dX, lr)
        return AitmLoss(cost, self.constraint_weight), pred

    keep_table_for_gradients = False      # True: train_step keeps a copy of the tables for last_gradients() (tests)

    def _table_step(self, rows, dX, lr):
        """Non-lazy Adam with L2 on every row of every table from dX [B, F*D]: lookup i takes row i of dX viewed as
        [B*F, D]; a lookup the gather refused has row -1, which the grouping drops."""
        k = self.k
        # the grouping flags a -1 row as out of range once more: the same bit the gather has already set in self.status
        groups = self._grouped("emb", rows, self.num_rows, None, self.status)
        D = self.embedding_size
        self._pp = k.segment_partials(groups, dX, D, out=self._pp)
        k.adam_rows_all(groups, dX, 1, self.emb, self.emb_m, self.emb_v, self.step_count, lr, BETA1, BETA2, ADAM_EPS,
                        partials=self._pp, l2=WEIGHT_DECAY)

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}, WITH the L2 term g + 1e-6 w: what the
        reference's optimizer applies (Adam(weight_decay) adds it before the moments).  The dense parameters' come from the
        flat buffer after l2_decay_grad; the tables' dense gradient is rebuilt with torch (for inspection, not on the step's
        path) and needs keep_table_for_gradients = True before the step, since the step overwrites the rows it decays."""
        out = {kk: self._views["g"][kk].clone() for kk in self.params}
        last = self._last
        if last["table"] is None:
            raise ValueError("set keep_table_for_gradients = True before train_step to read the tables' gradients")
        rows = last["rows"]
        keep = rows >= 0
        gt = torch.zeros_like(self.emb).index_add_(0, rows[keep], last["dX"].reshape(-1, self.embedding_size)[keep])
        gt = gt + WEIGHT_DECAY * last["table"]
        out.update(self._table_views(gt))
        return out


class DygraphModel:
    """aitm/dygraph_model.py — same method names; tensors are torch device tensors."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return AITMLayer(g("hyper_parameters.feature_vocabulary"), g("hyper_parameters.embedding_size"),
                         g("hyper_parameters.dims"), g("hyper_parameters.drop_prob"), device=device, kernels=kernels,
                         dropout_seed=g("runner.seed", 12345))

    def create_feeds(self, batch_data, config, device="cuda"):
        """(ids [B, F], click [B], buy [B]) as reader.AitmReader yields them -> the same on `device`, int64 (the reference's F
        per-field tensors are the columns ids[:, f])."""
        ids, click, buy = (torch.as_tensor(b).to(device).to(torch.int64) for b in batch_data[:3])
        return ids.contiguous(), click.reshape(-1).contiguous(), buy.reshape(-1).contiguous()

    def create_metrics(self, device="cuda"):
        return auc_metrics(device, ("click_auc", "purchase_auc"), NUM_THRESHOLDS)

    def _auc(self, dy_model, metrics_list, pred, click, buy):
        for col, (m, label) in enumerate(zip(metrics_list, (click, buy))):
            dy_model.k.auc_histogram_wide(pred[:, col], label, m[0], m[1], NUM_THRESHOLDS)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        ids, click, buy = self.create_feeds(batch_data, config, dy_model.device)
        loss, pred = dy_model.train_step(ids, click, buy, config.get("hyper_parameters.optimizer.learning_rate", 0.0001))
        self._auc(dy_model, metrics_list, pred, click, buy)
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        ids, click, buy = self.create_feeds(batch_data, config, dy_model.device)
        self._auc(dy_model, metrics_list, dy_model.predict(ids), click, buy)
        return metrics_list, None
