"""Host-side mirror of the reference's ENSFM plugin (models/recall/ensfm/net.py:24-98 ENSFMLayer; dygraph_model.py; infer.py)
on the recengine HIP kernels: Efficient Non-Sampling Factorization Machines, the recall net that trains on ALL user-item pairs.

The reference forms dot = einsum('ac,bc->abc', p_emb, q_emb), a [B, I+1, C] tensor, on every training step although the loss
never reads `pre` (net.py:87-88), and three [B, P, C] tensors for the positives (net.py:92-97).  Here a step is

  * rec_ensfm_tower_fwd twice -> p_emb [B, C] and q_emb [I+1, C] (C = mf_dim + 2);
  * rec_ensfm_gram twice -> the two C x C Gram matrices of the loss's whole-data term;
  * rec_ensfm_pos_user: forward and backward of the positives per user (g [B, P], the only (b, j)-shaped array; dP);
  * rec_ids_group of the positive lists by item + rec_ensfm_pos_item -> dQ for all I + 1 rows;
  * rec_ensfm_loss -> the loss and dH_i;
  * rec_ensfm_tower_bwd twice -> the gradient rows of every lookup, dH_s (shared by both towers), d bias;
  * Adagrad: rec_adagrad_rows through a grouping of each tower's ids (the item side's grouping is made once: the item
    attributes never change) with rec_segment_partials for the hot rows, one rec_adagrad_dense over H_i | H_s | bias.
--infer writes pre [B, I+1] with rec_ensfm_score.  The train step is eager."""
import numpy as np
import torch

from .net_base import FlatStore, LayerBase

ACC_INIT, ADAGRAD_EPS = 1e-8, 1e-6               # dygraph_model.py:56-59: initial_accumulator_value; Paddle's epsilon [EXT]
QUIRKS = ("the reader appends item 0's features as row I of item_attribute (movielens_reader.py:66-68), so the padding row of "
          "q_emb is a copy of item 0: masked out of pos_r, but counted in q^T q (item 0 enters the Gram term twice) and present as "
          "column I of pre, which infer.py deletes; create_optimizer builds Adagrad(lr, initial_accumulator_value=1e-8) whatever "
          "optimizer.class says, over every parameter; H_s is shared by the user and item cross terms; the tables are sized "
          "from the YAML (num_users, num_items, num_items + 1 rows; item_bias has num_items), not from the data; the loss sums "
          "over every (b, j), padded pairs contributing 0; HR@k divides the hits by min(k, test positives)")


class ENSFMLayer(LayerBase):
    """net.py:24-98.  forward(input_u [B, Fu], item_attribute [I+1, Fi], input_ur=None, item_bind_M=None) -> (pre,) or
    (pre, pos_r, q_emb, p_emb, H_i_emb);  train_step(input_u, item_attribute, input_ur, item_bind_M, lr, negative_weight)
    -> loss [1]."""

    def __init__(self, user_field_M, item_field_M, embedding_size, device="cuda", kernels=None):
        from ._lib import REC_ENSFM_MAX_DIM
        self._init_runtime(device, kernels, group_status=True)
        self.user_field_M, self.item_field_M, D = int(user_field_M), int(item_field_M), int(embedding_size)
        self.embedding_size = D
        if not 1 <= D <= REC_ENSFM_MAX_DIM:
            raise ValueError("ENSFM: embedding_size %d outside 1..%d (REC_ENSFM_MAX_DIM)" % (D, REC_ENSFM_MAX_DIM))
        if self.user_field_M < 1 or self.item_field_M < 1:
            raise ValueError("ENSFM: user_field_M and item_field_M must be positive")
        f32 = dict(dtype=torch.float32, device=self.device)
        tn = lambda *sh: torch.nn.init.trunc_normal_(torch.empty(*sh, **f32), std=0.01, a=-0.02, b=0.02)
        self.tables = {"user_feature_emb.weight": tn(self.user_field_M, D),
                       "all_item_feature_emb.weight": tn(self.item_field_M + 1, D),
                       "user_bias.weight": tn(self.user_field_M, 1), "item_bias.weight": tn(self.item_field_M, 1)}
        self.acc = {n: torch.full_like(t, ACC_INIT) for n, t in self.tables.items()}
        self.flat = FlatStore([("H_i", (D, 1)), ("H_s", (D, 1)), ("bias", (1,))], self.device,
                              fill={"m": ACC_INIT})                                         # store "m": the accumulator
        self.params = self.flat.view["p"]
        self.params["H_i"].fill_(0.01)
        self.params["H_s"].fill_(0.01)
        self._scratch = {}
        self._item_groups = None                     # (key, item_attribute, its two groupings): made once, the tensor never changes
        self.item_groupings_made = 0
        self._pp = {}

    # ---------------------------------------------------------------- parameters
    def _shown(self, store):
        src = {"p": self.tables, "m": self.acc}.get(store, {})
        out = dict(src)
        out.update(self.flat.view[store])
        return out

    def state_dict(self):
        return self._shown("p")

    def _optimizer_views(self):
        """Adagrad's accumulator of every parameter, under the parameter's own name."""
        return {"ensfm.acc.%s" % k: v for k, v in self._shown("m").items()}

    # ---------------------------------------------------------------- forward
    def _check(self, input_u, item_attribute, input_ur=None, item_bind_M=None):
        for t, name in ((input_u, "input_u"), (item_attribute, "item_attribute")):
            if t.dim() != 2 or t.dtype != torch.int64:
                raise ValueError("%s must be int64 [n, F], got %s %s" % (name, t.dtype, tuple(t.shape)))
        I = item_attribute.shape[0] - 1
        if I < 1:
            raise ValueError("item_attribute must hold at least one item and the padding row")
        if item_bind_M is not None and int(item_bind_M) != I:
            raise ValueError("item_bind_M %d is not item_attribute's row count - 1 = %d" % (int(item_bind_M), I))
        if input_ur is not None and (input_ur.dim() != 2 or input_ur.dtype != torch.int64 or input_ur.shape[0] != input_u.shape[0]):
            raise ValueError("input_ur must be int64 [B, P], got %s %s" % (input_ur.dtype, tuple(input_ur.shape)))
        return I

    def _towers(self, input_u, item_attribute):
        k, t, p = self.k, self.tables, self.params
        p_emb = k.ensfm_tower_fwd(input_u.contiguous(), t["user_feature_emb.weight"], t["user_bias.weight"], p["H_s"], p["bias"],
                                  item_layout=False, status=self.status)
        q_emb = k.ensfm_tower_fwd(item_attribute.contiguous(), t["all_item_feature_emb.weight"], t["item_bias.weight"], p["H_s"],
                                  None, item_layout=True, status=self.status)
        return p_emb, q_emb

    def forward(self, input_u, item_attribute, input_ur=None, item_bind_M=None, negative_weight=0.5):
        """net.py:63-98.  pos_r does not depend on negative_weight."""
        k = self.k
        self._check(input_u, item_attribute, input_ur, item_bind_M)
        p_emb, q_emb = self._towers(input_u, item_attribute)
        pre = k.ensfm_score(p_emb, q_emb, self.params["H_i"])
        if input_ur is None:
            return (pre,)
        G_q = k.ensfm_gram(q_emb, self._scratch)
        pos_r = k.ensfm_pos_user(input_ur.contiguous(), p_emb, q_emb, self.params["H_i"], G_q, negative_weight, status=self.status,
                                 want_pos_r=True)[4]
        H_i_emb = torch.cat([self.params["H_i"], torch.ones(2, 1, dtype=torch.float32, device=self.device)], 0)
        return pre, pos_r, q_emb, p_emb, H_i_emb

    __call__ = forward

    # ---------------------------------------------------------------- training
    def _item_side_groups(self, item_attribute):
        """The groupings of the item attributes by table row, for all_item_feature_emb and for item_bias (one row shorter: an
        id it does not hold is dropped there).  item_attribute goes to the device once and never changes, so they are made
        once: the cache is keyed on the tensor's storage (data_ptr, shape, strides, version counter), not on the Python
        object — the reader hands every batch a fresh view of the same storage.  item_groupings_made counts the misses."""
        k = self.k
        key = (item_attribute.data_ptr(), tuple(item_attribute.shape), item_attribute.stride(), item_attribute._version,
               item_attribute.device)
        hit = self._item_groups
        if hit is None or hit[0] != key:
            flat = item_attribute.contiguous().view(-1)
            gv, _ = k.ids_group(flat, self.item_field_M + 1, None, self.ws_group, None, self._group_status)
            gb, _ = k.ids_group(flat, self.item_field_M, None, self.ws_group, None, self.k.new_status(self.device))
            # the tensor is kept: its storage cannot be freed and handed to another tensor while the key is live
            hit = self._item_groups = (key, item_attribute, gv, gb)
            self.item_groupings_made += 1
        return hit[2], hit[3]

    def _adagrad_rows(self, name, groups, grad, div, lr):
        k = self.k
        P = self.tables[name]
        self._pp[name] = k.segment_partials(groups, grad, P.shape[1], grad_div=div, out=self._pp.get(name))
        k.adagrad_rows(groups, grad, div, P, self.acc[name], lr, ADAGRAD_EPS, partials=self._pp[name])

    def train_step(self, input_u, item_attribute, input_ur, item_bind_M=None, lr=0.05, negative_weight=0.5):
        """dygraph_model.py:40-51,71-78: forward, loss, backward and the Adagrad step -> loss [1]."""
        k, t, p, g = self.k, self.tables, self.params, self.flat.view["g"]
        I = self._check(input_u, item_attribute, input_ur, item_bind_M)
        self.step_count += 1
        w, sc = float(negative_weight), self._scratch
        u, attr, ur = input_u.contiguous(), item_attribute.contiguous(), input_ur.contiguous()
        B, Fu = u.shape
        Fi = attr.shape[1]
        p_emb, q_emb = self._towers(u, attr)
        G_p, G_q = k.ensfm_gram(p_emb, sc), k.ensfm_gram(q_emb, sc)
        gpos, dP, loss_part, dHi_part, _ = k.ensfm_pos_user(ur, p_emb, q_emb, p["H_i"], G_q, w, status=self.status)
        # padding_idx = I: the padded positions of the lists leave the grouping (net.py:93)
        groups_ur = self._grouped("ur", ur.view(-1), I + 1, I, self._group_status)
        dQ = k.ensfm_pos_item(groups_ur, gpos, p_emb, q_emb, p["H_i"], G_p, w)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        k.ensfm_loss(G_p, G_q, p["H_i"], loss_part, dHi_part, w, B, loss=loss, dH_i=g["H_i"].view(-1))
        # H_s is shared by both cross terms (net.py:72-73): the user side writes dH_s, the item side adds to it
        rows_u, dsc_u = k.ensfm_tower_bwd(u, t["user_feature_emb.weight"], p["H_s"], dP, g["H_s"].view(-1), g["bias"],
                                          item_layout=False, scratch=sc)
        rows_v, dsc_v = k.ensfm_tower_bwd(attr, t["all_item_feature_emb.weight"], p["H_s"], dQ, g["H_s"].view(-1), None,
                                          item_layout=True, accumulate=True, scratch=sc)
        # Adagrad over every parameter (dygraph_model.py:54-60), after every gradient has been formed
        fl = self.flat.flat
        k.adagrad_dense(fl["p"], fl["m"], fl["g"], lr, ADAGRAD_EPS)
        groups_u = self._grouped("u", u.view(-1), self.user_field_M, None, self._group_status)
        gv, gb = self._item_side_groups(item_attribute)
        self._adagrad_rows("user_feature_emb.weight", groups_u, rows_u, 1, lr)
        self._adagrad_rows("user_bias.weight", groups_u, dsc_u, Fu, lr)
        self._adagrad_rows("all_item_feature_emb.weight", gv, rows_v, 1, lr)
        self._adagrad_rows("item_bias.weight", gb, dsc_v, Fi, lr)
        self._last = dict(u=u, attr=attr, rows_u=rows_u, dsc_u=dsc_u, rows_v=rows_v, dsc_v=dsc_v, dP=dP, dQ=dQ, g=gpos,
                          p_emb=p_emb, q_emb=q_emb)
        return loss

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}; the tables' dense gradients are rebuilt with
        torch, on the host, from the step's gradient rows (for inspection, not on the step's path)."""
        L, D = self._last, self.embedding_size
        out = {k: v.clone() for k, v in self.flat.view["g"].items()}

        def dense(name, ids, rows, rep):
            T = self.tables[name]
            flat = ids.reshape(-1)
            src = rows if rep == 1 else rows[:ids.shape[0]].repeat_interleave(rep).view(-1, 1)
            keep = (flat >= 0) & (flat < T.shape[0])
            # on the host: the device's index_add_ sums duplicates with float atomics, in no fixed order
            dense_g = torch.zeros(T.shape, dtype=torch.float32).index_add_(0, flat[keep].cpu(), src.view(flat.numel(), -1)[keep].cpu())
            return dense_g.to(T.device)

        out["user_feature_emb.weight"] = dense("user_feature_emb.weight", L["u"], L["rows_u"], 1)
        out["user_bias.weight"] = dense("user_bias.weight", L["u"], L["dsc_u"], L["u"].shape[1])
        out["all_item_feature_emb.weight"] = dense("all_item_feature_emb.weight", L["attr"], L["rows_v"], 1)
        out["item_bias.weight"] = dense("item_bias.weight", L["attr"], L["dsc_v"], L["attr"].shape[1])
        return out


def hit_ratios(pre, train_mask, test_mask, ks=(5, 10, 20)):
    """infer.py:183-209 on the device.  pre [B, I+1] (column I, the padding item, is dropped); train_mask, test_mask bool
    [B, I]: the user's train positives are set to -inf, then for every k the hits among the top k divided by min(k, number of
    test positives).  Equal scores order by the lower item id.  -> float32 [len(ks), B]."""
    pre = pre[:, :-1].clone()
    pre[train_mask] = float("-inf")
    n_test = test_mask.sum(1)
    out = []
    for kk in ks:
        kth = torch.topk(pre, kk, dim=1).values[:, -1:]
        above = pre > kth
        tie = pre == kth
        room = kk - above.sum(1, keepdim=True)                 # places left for the tied scores: the lowest ids take them
        chosen = above | (tie & (torch.cumsum(tie, 1) <= room))
        hits = (chosen & test_mask).sum(1).to(torch.float32)
        out.append(hits / torch.clamp(n_test, max=kk).to(torch.float32))
    return torch.stack(out)


class DygraphModel:
    """ensfm/dygraph_model.py — same method names; tensors are torch device tensors.  infer_summary(): infer.py's HR@5, HR@10
    and HR@20 over the rows seen since the last call (the loader sets `dataset` for the user -> train / test sets)."""

    def __init__(self):
        self.dataset = None
        self._rows = []

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return ENSFMLayer(g("hyper_parameters.num_users"), g("hyper_parameters.num_items"), g("hyper_parameters.mf_dim"),
                          device=device, kernels=kernels)

    def create_feeds(self, batch_data, device="cuda"):
        """dygraph_model.py:31-37.  The item attributes and item_bind_M arrive once per sample and copy 0 is the feed.  A
        tensor that already is int64 on the device is passed through; item_bind_M (feed 3) is a host scalar and stays on the
        host — nothing on the device reads it (it is item_attribute's row count - 1)."""
        batch_data = list(batch_data)
        batch_data[1] = batch_data[1][0]
        if len(batch_data) >= 4:
            batch_data[3] = batch_data[3][0]
        dev = torch.device(device)
        out = []
        for i, b in enumerate(batch_data):
            if not torch.is_tensor(b):
                b = torch.as_tensor(np.asarray(b))
            if i == 3:
                out.append(b.to(torch.int64))
                continue
            same = b.device.type == dev.type and (dev.index is None or b.device.index == dev.index)
            out.append(b if same and b.dtype == torch.int64 else b.to(dev).to(torch.int64))
        return out

    def create_loss(self, prediction, config):
        """dygraph_model.py:40-51 with torch on forward()'s outputs (train_forward takes the loss from rec_ensfm_loss)."""
        pre, pos_r, q_emb, p_emb, H_i_emb = prediction
        w = config.get("hyper_parameters.negative_weight", 0.5)
        loss = w * ((q_emb.t() @ q_emb) * (p_emb.t() @ p_emb) * (H_i_emb @ H_i_emb.t())).sum()
        return loss + ((1.0 - w) * pos_r * pos_r - 2.0 * pos_r).sum()

    def create_optimizer(self, dy_model, config):
        return None                                          # Adagrad is part of train_step

    def create_metrics(self, device="cuda"):
        return [], []

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        u, attr, ur, bind = self.create_feeds(batch_data, dy_model.device)
        # `bind` is on the host: checking it against item_attribute's row count costs no device read
        loss = dy_model.train_step(u, attr, ur, int(bind.reshape(-1)[0]), config.get("hyper_parameters.optimizer.learning_rate", 0.05),
                                   config.get("hyper_parameters.negative_weight", 0.5))
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        """batch_data: (user features, item attributes) as the reference's loader yields them; EnsfmReader adds the bound user
        id of every row as a third, device-resident element, so the train / test item sets are gathered on the device.  Without
        it the ids are looked up on the host from the feature rows, as infer.py does."""
        feeds = self.create_feeds(batch_data, dy_model.device)
        u, attr = feeds[:2]
        pre = dy_model.forward(u, attr)[0]
        if self.dataset is not None:
            train_mask, test_mask = self.dataset.user_masks(u, dy_model.device, feeds[2] if len(feeds) == 3 else None)
            self._rows.append(hit_ratios(pre, train_mask, test_mask))
        return metrics_list, {"user": u, "prediction": pre}

    def infer_summary(self):
        if not self._rows:
            return {"HR@5": 0.0, "HR@10": 0.0, "HR@20": 0.0}
        m = torch.cat(self._rows, 1).mean(1).tolist()
        self._rows = []
        return {"HR@5": m[0], "HR@10": m[1], "HR@20": m[2]}
