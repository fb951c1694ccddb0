"""Host-side mirror of the reference's DIEN plugin (models/rank/dien/net.py:21-280 DIENLayer, dygraph_model.py) on the
recengine HIP kernels.

Kept as the reference writes it, oddities included:
  * eight independent tables (hist / target / target-seq / neg x item / cat), all with padding_idx 0: id 0 reads as a zero
    row and row 0 never gets a gradient (unlike DIN, where id 0 is a live row); item_b_attr has no padding row;
  * the interest extractor is a 2-layer GRU over ALL T positions (no lengths: padded positions are processed); only its
    layer-1 outputs are used, and only by the auxiliary loss;
  * the attention MLP is used but never trained: add_sublayer('linear_%d') is called again for the top MLP under the same
    names (net.py:123,144), so the attention Linears are not parameters — no gradient, not in state_dict (set_attention
    sets them) — while gradients flow THROUGH them to the rows (DIN's App. B-9 again);
  * x_att = w * hist is not pooled; the attention "GRU" is a plain GRUCell (not AUGRU) stepped over all T positions from a
    zero state, and only its last state is used, whatever the sample's length;
  * the auxiliary loss has no length mask and no minus sign, and its negative term is log(sigmoid(n)), not 1 - sigmoid;
    the clip on the positive term has no bounds (the identity);
  * cost = BCEWithLogits(mean) + aux; SGD with PiecewiseDecay([410000], [base_lr, 0.2]) (dygraph_model.py:66-75).
The GRU recurrences are one launch per layer and direction (rec_gru_seq_fwd / _bwd); their input projections, weight
gradients and dX are rec_gemm_f32 calls over all B*T rows.  The GRU state_dict keys (gru_net.weight_ih_l0, ...,
gru_cell_attention.weight_ih, ...) follow Paddle's documentation of nn.GRU / nn.GRUCell and are unverified against a
Paddle install; set_dict also takes gru_net.{l}.cell.*.  The train step is eager (no plan recorder, no graph capture).
"""
import math

import torch

from .din import _xavier_uniform_
from .net_base import FlatStore, LayerBase, auc_metrics, auc_update

TABLES = (("hist_item_emb_attr", 0), ("hist_cat_emb_attr", 1), ("target_item_emb_attr", 0), ("target_cat_emb_attr", 1),
          ("target_item_seq_emb_attr", 0), ("target_cat_seq_emb_attr", 1), ("neg_item_seq_emb_attr", 0),
          ("neg_cat_seq_emb_attr", 1))
GRU_KEYS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
QUIRKS = ("padding_idx 0 on all eight tables (row 0 is never trained); the attention MLP is used but not trained and not "
          "in state_dict; the GRUs and the aux loss run over padded positions; aux has no minus sign and uses sigmoid(n); "
          "plain GRUCell instead of AUGRU, last state whatever the length")


class DIENLayer(LayerBase):
    """dien/net.py:21-280.  forward(...) -> (logit [B,1], aux_loss [1])."""

    def __init__(self, item_emb_size, cat_emb_size, act, is_sparse, use_DataLoader, item_count, cat_count, device="cuda",
                 kernels=None):
        if item_emb_size != cat_emb_size:
            raise ValueError("DIEN: item_emb_size (%d) must equal cat_emb_size (%d): the reference's attention GRU starts "
                             "from a state of item_emb_size * 2 columns (net.py:258)" % (item_emb_size, cat_emb_size))
        self._init_runtime(device, kernels)
        self.item_emb_size, self.cat_emb_size = item_emb_size, cat_emb_size
        self.item_count, self.cat_count = item_count, cat_count
        f32 = dict(dtype=torch.float32, device=self.device)
        E = self.E = item_emb_size + cat_emb_size
        if E % 4 or E > getattr(self.k, "GRU_MAX_HIDDEN", 256):
            raise ValueError("DIEN: item_emb_size + cat_emb_size = %d must be a multiple of 4, at most 256" % E)
        self.params = {}
        for name, kind in TABLES:
            rows, dim = (item_count, item_emb_size) if kind == 0 else (cat_count, cat_emb_size)
            w = _xavier_uniform_(torch.empty(rows, dim, **f32), rows, dim)
            w[0].zero_()                                                                   # padding_idx=0
            self.params[name + ".weight"] = w
        self.params["item_b_attr.weight"] = torch.zeros(item_count, 1, **f32)              # net.py:102-107
        sizes = [4 * E, 80, 40, 1]                                                         # net.py:110-128
        self.attention_w = [_xavier_uniform_(torch.empty(sizes[i], sizes[i + 1], **f32), sizes[i], sizes[i + 1])
                            for i in range(3)]
        self.attention_b = [torch.zeros(sizes[i + 1], **f32) for i in range(3)]
        # the dense parameters (top MLP, the three GRU cells) are views of ONE flat buffer, their gradients of another
        top = [2 * E, 80, 40, 1]                                                           # net.py:131-149
        shapes = []
        for i in range(3):
            shapes += [("linear_%d.weight" % i, (top[i], top[i + 1])), ("linear_%d.bias" % i, (top[i + 1],))]
        self.gru_names = []
        for pat in ("gru_net.%s_l0", "gru_net.%s_l1", "gru_cell_attention.%s"):            # net.py:153-159
            names = [pat % key for key in GRU_KEYS]
            self.gru_names.append(names)
            shapes += [(names[0], (3 * E, E)), (names[1], (3 * E, E)), (names[2], (3 * E,)), (names[3], (3 * E,))]
        self.flat = FlatStore(shapes, self.device, stores=("p", "g"))     # SGD: no moments; W_hh is read as float4
        self._gb = self.flat.view["g"]
        for name, sh in shapes:
            self.params[name] = self.flat.view["p"][name]
            if name.startswith("linear_") and name.endswith(".weight"):
                _xavier_uniform_(self.params[name], sh[0], sh[1])
            elif name.startswith("gru"):
                self.params[name].uniform_(-1.0 / math.sqrt(E), 1.0 / math.sqrt(E))       # Uniform(+-1/sqrt(H))

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        return dict(self.params)

    def set_dict(self, sd):
        mine = {}
        for key, v in sd.items():
            parts = key.split(".")
            if len(parts) == 4 and parts[0] == "gru_net" and parts[2] == "cell":           # gru_net.{l}.cell.weight_ih
                key = "gru_net.%s_l%s" % (parts[3], parts[1])
            mine[key] = v
        super().set_dict(mine)

    def set_attention(self, weights, biases):
        for dst, src in zip(self.attention_w + self.attention_b, list(weights) + list(biases)):
            dst.copy_(torch.as_tensor(src).to(self.device).reshape(dst.shape))

    def _gru(self, i):
        return [self.params[n] for n in self.gru_names[i]]

    # ---------------------------------------------------------------- forward
    def _rows(self, item_ids, cat_ids, item_table, cat_table):
        """[.., E] = [item row | cat row] of the two tables (padding_idx 0)."""
        p, Ei, E = self.params, self.item_emb_size, self.E
        out = torch.empty(*item_ids.shape, E, dtype=torch.float32, device=self.device)
        flat = out.view(-1, E)
        self.k.emb_gather(item_ids.reshape(-1).contiguous(), p[item_table + ".weight"], 0, self.status, out=flat,
                          out_group=1, out_group_stride=E)
        self.k.emb_gather(cat_ids.reshape(-1).contiguous(), p[cat_table + ".weight"], 0, self.status, out=flat[:, Ei:],
                          out_group=1, out_group_stride=E)
        return out

    def forward(self, hist_item_seq, hist_cat_seq, target_item, target_cat, label, mask, target_item_seq, target_cat_seq,
                neg_hist_item_seq, neg_hist_cat_seq, _keep=None):
        p, E, k, ws = self.params, self.E, self.k, self.ws
        B, T = hist_item_seq.shape
        train = _keep is not None
        hist = self._rows(hist_item_seq, hist_cat_seq, "hist_item_emb_attr", "hist_cat_emb_attr")       # net.py:168-179
        q = self._rows(target_item_seq, target_cat_seq, "target_item_seq_emb_attr", "target_cat_seq_emb_attr")
        ti, tc = target_item.reshape(-1).contiguous(), target_cat.reshape(-1).contiguous()
        emb = torch.empty(B, 2 * E, dtype=torch.float32, device=self.device)                            # net.py:275
        k.emb_gather(ti, p["target_item_emb_attr.weight"], 0, self.status, out=emb[:, E:], out_group=1,
                     out_group_stride=2 * E)
        k.emb_gather(tc, p["target_cat_emb_attr.weight"], 0, self.status, out=emb[:, E + self.item_emb_size:],
                     out_group=1, out_group_stride=2 * E)
        item_b, _ = k.emb_gather(ti, p["item_b_attr.weight"], None, self.status)                        # net.py:176
        # interest extractor (net.py:190): two GRU layers, only layer 1's outputs are used
        h0, sv0 = k.gru_layer_fwd(hist, *self._gru(0), ws, want_saved=train)
        h1, sv1 = k.gru_layer_fwd(h0, *self._gru(1), ws, want_saved=train)
        ni, nc = neg_hist_item_seq.contiguous(), neg_hist_cat_seq.contiguous()
        aux, _ = k.dien_aux_fwd(h1, hist, ni, nc, p["neg_item_seq_emb_attr.weight"], p["neg_cat_seq_emb_attr.weight"], ws,
                                padding_idx=0, status=self.status)                                      # net.py:219-254
        mask2 = mask.reshape(B, T).to(torch.float32).contiguous()
        w, x_att, att_saved = k.dien_attention_seq(hist, q, mask2, self.attention_w, self.attention_b, ws)   # 192-209
        ha, sva = k.gru_layer_fwd(x_att, *self._gru(2), ws, want_saved=train)                           # net.py:256-273
        emb[:, :E].copy_(ha[:, T - 1])          # the last state, whatever the sample's length (a strided device copy)
        x1 = k.gemm(emb, p["linear_0.weight"], ws, epilogue="bias_sigmoid", bias=p["linear_0.bias"])
        x2 = k.gemm(x1, p["linear_1.weight"], ws, epilogue="bias_sigmoid", bias=p["linear_1.bias"])
        logit = k.gemm(x2, p["linear_2.weight"], ws, epilogue="add", bias=p["linear_2.bias"], aux1=item_b)   # net.py:279
        if train:
            _keep.update(hist=hist, q=q, ti=ti, tc=tc, emb=emb, h0=h0, h1=h1, sv0=sv0, sv1=sv1, sva=sva, ni=ni, nc=nc,
                         w=w, x_att=x_att, att_saved=att_saved, x1=x1, x2=x2)
        return logit, aux

    __call__ = forward

    # ---------------------------------------------------------------- training
    @staticmethod
    def learning_rate(step, base_lr):
        """paddle.optimizer.lr.PiecewiseDecay(boundaries=[410000], values=[base_lr, 0.2]) (dygraph_model.py:67-74)."""
        return base_lr if step < 410000 else 0.2

    def _sgd_rows(self, ids, grad_view, table, lr, row_stride_floats, padding_idx):
        grp = self._grouped(ids.numel(), ids.reshape(-1), table.shape[0], padding_idx, self.status)   # one per id count
        pp = self.k.segment_partials(grp, grad_view, table.shape[1], grad_group=1, grad_group_stride=row_stride_floats)
        self.k.sparse_sgd_rows(grp, grad_view, table, lr, grad_group=1, grad_group_stride=row_stride_floats, partials=pp)

    def train_step(self, hist_item_seq, hist_cat_seq, target_item, target_cat, label, mask, target_item_seq,
                   target_cat_seq, neg_hist_item_seq, neg_hist_cat_seq, base_lr=0.85):
        """dygraph_model.py:86-103 train_forward + backward + SGD.  -> (cost [1], pred [B,1], aux [1])."""
        p, E, Ei, k, ws, g = self.params, self.E, self.item_emb_size, self.k, self.ws, self._gb
        B, T = hist_item_seq.shape
        lr = self.learning_rate(self.step_count, base_lr)
        self.step_count += 1
        sv = {}
        logit, aux = self.forward(hist_item_seq, hist_cat_seq, target_item, target_cat, label, mask, target_item_seq,
                                  target_cat_seq, neg_hist_item_seq, neg_hist_cat_seq, _keep=sv)
        pred, dz, loss = k.bce_with_logits(logit, label.reshape(B, 1).to(torch.float32).contiguous(), ws)
        cost = loss + aux                                                                  # dygraph_model.py:96

        def lin_bwd(name, x, dy, act=None):
            kw = dict(epilogue="dsigmoid", aux0=act) if act is not None else {}
            return k.linear_backward(x, dy, p[name + ".weight"], ws, g[name + ".weight"], g[name + ".bias"], **kw)

        d2 = lin_bwd("linear_2", sv["x2"], dz, act=sv["x2"])
        d1 = lin_bwd("linear_1", sv["x1"], d2, act=sv["x1"])
        de = lin_bwd("linear_0", sv["emb"], d1)                        # [B, 2E] = [d h_T | d target_concat]
        # attention GRU: only its last state has a gradient
        na, n1, n0 = self.gru_names[2], self.gru_names[1], self.gru_names[0]
        grads = lambda names: [g[n] for n in names]
        dx_att = k.gru_layer_bwd(sv["x_att"], sv["sva"], p[na[0]], p[na[1]], ws, *grads(na),
                                 dh_T=de[:, :E].contiguous())
        # d_hist collects four contributions: the weighting and the attention features here, then aux, then GRU layer 0
        d_hist = torch.empty(B, T, E, dtype=torch.float32, device=self.device)
        d_q = k.dien_attention_seq_bwd(sv["hist"], sv["q"], sv["w"], sv["att_saved"], self.attention_w, dx_att, d_hist, ws,
                                       accumulate=False)
        d_h1, d_neg = k.dien_aux_bwd(sv["h1"], sv["hist"], sv["ni"], sv["nc"], p["neg_item_seq_emb_attr.weight"],
                                     p["neg_cat_seq_emb_attr.weight"], d_hist, accumulate=True, d_aux=1.0, padding_idx=0,
                                     status=self.status)
        d_h0 = k.gru_layer_bwd(sv["h0"], sv["sv1"], p[n1[0]], p[n1[1]], ws, *grads(n1), dH_out=d_h1)
        d_hist = k.gru_layer_bwd(sv["hist"], sv["sv0"], p[n0[0]], p[n0[1]], ws, *grads(n0), dH_out=d_h0, dX_add=d_hist)
        self._last = dict(d_hist=d_hist, d_q=d_q, d_neg=d_neg, de=de, dz=dz)
        # ---- SGD: every table once (merged rows, padding row dropped); the dense parameters in one launch
        jobs = [(hist_item_seq, d_hist, "hist_item_emb_attr", E, 0), (hist_cat_seq, d_hist[:, :, Ei:], "hist_cat_emb_attr", E, 0),
                (target_item_seq, d_q, "target_item_seq_emb_attr", E, 0),
                (target_cat_seq, d_q[:, :, Ei:], "target_cat_seq_emb_attr", E, 0),
                (sv["ni"], d_neg, "neg_item_seq_emb_attr", E, 0), (sv["nc"], d_neg[:, :, Ei:], "neg_cat_seq_emb_attr", E, 0),
                (sv["ti"], de[:, E:], "target_item_emb_attr", 2 * E, 0),
                (sv["tc"], de[:, E + Ei:], "target_cat_emb_attr", 2 * E, 0),
                (sv["ti"], dz, "item_b_attr", 1, None)]
        for ids, gv, name, rs, pad in jobs:
            self._sgd_rows(ids.contiguous(), gv, p[name + ".weight"], lr, rs, pad)
        k.sgd_dense(self.flat.flat["p"], self.flat.flat["g"], lr)
        return cost, pred, aux


class DygraphModel:
    """dien/dygraph_model.py:21-117 — same method names; tensors are torch device tensors."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return DIENLayer(g("hyper_parameters.item_emb_size", 64), g("hyper_parameters.cat_emb_size", 64),
                         g("hyper_parameters.act", "sigmoid"), g("hyper_parameters.is_sparse", False),
                         g("hyper_parameters.use_DataLoader", False), g("hyper_parameters.item_count", 63001),
                         g("hyper_parameters.cat_count", 801), device=device, kernels=kernels)

    def create_feeds(self, batch, config, device="cuda"):
        t = [torch.as_tensor(x).to(device) for x in batch]
        label = t[4].to(torch.float32).reshape(-1, 1)                                  # dygraph_model.py:51
        return t[0], t[1], t[2], t[3], label, t[5], t[6], t[7], t[8], t[9]

    def create_metrics(self, device="cuda"):
        return auc_metrics(device)

    def _auc(self, dy_model, metrics_list, pred, label):
        if metrics_list:
            auc_update(dy_model.k, metrics_list[0], pred, label)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        feeds = self.create_feeds(batch_data, config, dy_model.device)
        base_lr = config.get("hyper_parameters.optimizer.learning_rate_base_lr")
        cost, pred, _ = dy_model.train_step(*feeds, base_lr=base_lr)
        self._auc(dy_model, metrics_list, pred, feeds[4])
        return cost, metrics_list, {"loss": cost}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        feeds = self.create_feeds(batch_data, config, dy_model.device)
        logit, _ = dy_model.forward(*feeds)
        pred = torch.sigmoid(logit)
        self._auc(dy_model, metrics_list, pred, feeds[4])
        return metrics_list, None
