"""Host-side mirror of the reference's DMR plugin (models/rank/dmr/net.py:22-554 DMRLayer, dygraph_model.py) on the
recengine HIP kernels: Deep Match to Rank, the third net of the DIN -> DIEN -> DMR line.

Kept as the reference writes it, oddities included (QUIRKS below).  What is computed differently, with the same result:
  * the user-to-item net builds a [B, T, T] tile and a softmax per row, then dm_fcn_1 + PReLU over all T rows, and reads
    rows T-1 and T-2 only (net.py:288-291); the other rows receive no gradient.  Here rec_dmr_prefix_pool_fwd computes
    exactly those two rows (the padded "future" entries included: a prefix without a valid position is uniform 1/T over
    all T entries) and dm_fcn_1 / its PReLU run on 2B rows instead of 50B;
  * the auxiliary loss never materialises the [B, cate_size] logits (rec_dmr_match_loss_*);
  * the tiled item_eb of the item-to-item query (net.py:311-319) is a lookup of the tiled ids, and its gradient is summed
    over T before the rows merge.
Every Linear and weight gradient is rec_gemm_f32; the features are rec_dien_att_feat_* with the two inputs swapped
([q, h, q - h, q * h]); BatchNorm, BCE, AUC and Adam are the existing entry points.  paddle.optimizer.Adam here is the
dygraph default, non-lazy: every row of every table moves each step (rec_adam_rows_all, also for the small dense tables —
the same arithmetic as the dense rule on the dense-equivalent gradient); the Linears, PReLUs and BatchNorm scale / shift
are views of one flat buffer stepped by one rec_adam_dense.  The only torch work on the step's path is allocation and id
plumbing (slices of the feed matrix made contiguous, the tiled / concatenated id lists of the shared tables).
The state_dict keys (PReLU `_weight`; BatchNorm `weight`, `bias`, `_mean`, `_variance`; Linear weights [in, out]) follow
Paddle's documentation and are unverified against a Paddle install.  The train step is eager (no graph capture).
"""
import math

import torch

from .net_base import FlatStore, LayerBase, auc_metrics, auc_update, scatter_rows

USER_FEAT = (("uid", "uid_embeddings_var"), ("cms_segid", "cms_segid_embeddings_var"),
             ("cms_group_id", "cms_group_id_embeddings_var"), ("final_gender_code", "final_gender_code_embeddings_var"),
             ("age_level", "age_level_embeddings_var"), ("pvalue_level", "pvalue_level_embeddings_var"),
             ("shopping_level", "shopping_level_embeddings_var"), ("occupation", "occupation_embeddings_var"),
             ("new_user_class_level", "new_user_class_level_embeddings_var"))
ITEM_FEAT = (("mid", "mid_embeddings_var"), ("cate_id", "cat_embeddings_var"), ("brand", "brand_embeddings_var"),
             ("campaign_id", "campaign_id_embeddings_var"), ("customer", "customer_embeddings_var"))
# the 17 scalar columns behind the five history blocks (net.py:405-425)
SCALARS = ("uid", "cms_segid", "cms_group_id", "final_gender_code", "age_level", "pvalue_level", "shopping_level",
           "occupation", "new_user_class_level", "mid", "cate_id", "campaign_id", "customer", "brand", "price_slot", "pid",
           "label")
BN_MOMENTUM, BN_EPS = 0.99, 1e-3
QUIRKS = ("a prefix with no valid position is pooled uniformly (1/T) over ALL T positions, future ones included; "
          "logits_layer is declared and in state_dict but never used and never stepped; dm_item_biases is a constant "
          "zero, not a parameter; the aux label is the LAST history cate while user_vector2 comes from position T-2; "
          "sum_t hist ignores the mask; PReLU is applied to the final logit; the i2i softmax of a fully masked row is "
          "uniform")


class DMRLayer(LayerBase):
    """dmr/net.py:22-554.  forward([sparse [B, 5T+17] i64, price [B,1] f32], is_infer) -> (y_hat [B,1], loss [1])."""

    def __init__(self, user_size, cms_segid_size, cms_group_id_size, final_gender_code_size, age_level_size,
                 pvalue_level_size, shopping_level_size, occupation_size, new_user_class_level_size, adgroup_id_size,
                 cate_size, campaign_id_size, customer_size, brand_size, btag_size, pid_size, main_embedding_size,
                 other_embedding_size, history_length=50, device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        E, O, T = main_embedding_size, other_embedding_size, history_length
        if E % 4 or not 0 < E <= 64:
            raise ValueError("DMR: main_embedding_size %d must be a multiple of 4, at most 64 (rec_dmr_match_loss_*)" % E)
        if T < 2:
            raise ValueError("DMR: history_length %d must be at least 2 (user_vector2 is position T-2)" % T)
        self.main_embedding_size, self.other_embedding_size, self.history_length = E, O, T
        self.cate_size = cate_size
        f32 = dict(dtype=torch.float32, device=self.device)
        sizes = dict(uid_embeddings_var=(user_size, E), mid_embeddings_var=(adgroup_id_size, E),
                     cat_embeddings_var=(cate_size, E), brand_embeddings_var=(brand_size, E),
                     btag_embeddings_var=(btag_size, O), dm_btag_embeddings_var=(btag_size, O),
                     campaign_id_embeddings_var=(campaign_id_size, E), customer_embeddings_var=(customer_size, E),
                     cms_segid_embeddings_var=(cms_segid_size, O), cms_group_id_embeddings_var=(cms_group_id_size, O),
                     final_gender_code_embeddings_var=(final_gender_code_size, O),
                     age_level_embeddings_var=(age_level_size, O), pvalue_level_embeddings_var=(pvalue_level_size, O),
                     shopping_level_embeddings_var=(shopping_level_size, O), occupation_embeddings_var=(occupation_size, O),
                     new_user_class_level_embeddings_var=(new_user_class_level_size, O), pid_embeddings_var=(pid_size, O),
                     position_embeddings_var=(T, O), dm_position_embeddings_var=(T, O), dm_item_vectors_var=(cate_size, E))
        self.tables = tuple(sizes)
        self.params, self._tm, self._tv = {}, {}, {}
        for name, (rows, dim) in sizes.items():                                   # nn.initializer.Uniform(): U(-1, 1)
            self.params[name + ".weight"] = torch.empty(rows, dim, **f32).uniform_(-1.0, 1.0)
            self._tm[name] = torch.zeros(rows, dim, **f32)
            self._tv[name] = torch.zeros(rows, dim, **f32)
        # tower input (net.py:373-377, 524-528): column ranges of `inp`
        self.cols, c = {}, 0
        for n, t in USER_FEAT + ITEM_FEAT:
            self.cols[n] = (c, sizes[t][1])
            c += sizes[t][1]
        for n, w in (("price", 1), ("pid", O), ("hist_sum", 2 * E), ("prod", 2 * E), ("rel_u2i", 1), ("rel_i2i", 1),
                     ("att", 2 * E)):
            self.cols[n] = (c, w)
            c += w
        L = self.inp_length = c
        assert L == 12 * E + 9 * O + 3
        lin = [("query_layer", 2 * O, 2 * E), ("att_layer1_layer", 8 * E, 80), ("att_layer2_layer", 80, 40),
               ("att_layer3_layer", 40, 1), ("dnn_layer1_layer", 2 * E, E), ("query_layer2", 2 * (E + O), 2 * E),
               ("att_layer1_layer2", 8 * E, 80), ("att_layer2_layer2", 80, 40), ("att_layer3_layer2", 40, 1),
               ("dnn0_layer", L, 512), ("dnn1_layer", 512, 256), ("dnn2_layer", 256, 128), ("dnn3_layer", 128, 1)]
        prelu = [("query_prelu", T), ("dnn_layer1_prelu", T), ("query_prelu2", T), ("dnn0_prelu", 512), ("dnn1_prelu", 256),
                 ("dnn2_prelu", 128), ("dnn3_prelu", 1)]
        shapes = []
        for n, i, o in lin:
            shapes += [(n + ".weight", (i, o)), (n + ".bias", (o,))]
        shapes += [(n + "._weight", (c,)) for n, c in prelu]
        shapes += [("inp_layer.weight", (L,)), ("inp_layer.bias", (L,))]
        self.flat = FlatStore(shapes, self.device)       # everything but the tables, with Adam's moments: one adam_dense
        self._gb, self._dense_m = self.flat.view["g"], self.flat.flat["m"]
        for name, sh in shapes:
            self.params[name] = self.flat.view["p"][name]
            if name.endswith("_layer.weight") or name.endswith("_layer2.weight") or name.startswith("query_layer"):
                if len(sh) == 2:                                                  # nn.Linear: XavierUniform
                    lim = math.sqrt(6.0 / (sh[0] + sh[1]))
                    self.params[name].uniform_(-lim, lim)
            if name.endswith("._weight"):
                self.params[name].fill_(0.1)                                      # PReLU(init=0.1)
        self.params["inp_layer.weight"].fill_(1.0)
        self.params["inp_layer._mean"] = torch.zeros(L, **f32)
        self.params["inp_layer._variance"] = torch.ones(L, **f32)
        lim = math.sqrt(6.0 / (E + cate_size))                                    # declared, never used (net.py:236)
        self.params["logits_layer.weight"] = torch.empty(E, cate_size, **f32).uniform_(-lim, lim)
        self.params["logits_layer.bias"] = torch.zeros(cate_size, **f32)
        self._ids = {}

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        return dict(self.params)

    def _optimizer_views(self):
        """The Adam moments of the flat dense buffer, gaps included, and of every table (checkpoint.py saves the step)."""
        st = {"dmr.dense.m": self.flat.flat["m"], "dmr.dense.v": self.flat.flat["v"]}
        for n in self.tables:
            st["dmr.%s.m" % n], st["dmr.%s.v" % n] = self._tm[n], self._tv[n]
        return st

    # ---------------------------------------------------------------- forward
    def _const_ids(self, B):
        """Per batch size: the position ids of the two position tables and arange(cate_size) (id plumbing, cached)."""
        hit = self._ids.get(B)
        if hit is None:
            T = self.history_length
            pos = torch.arange(T, dtype=torch.int64, device=self.device).repeat(B)
            hit = self._ids[B] = (pos, torch.arange(self.cate_size, dtype=torch.int64, device=self.device))
        return hit

    def _gather(self, ids, table, out, stride):
        self.k.emb_gather(ids, self.params[table + ".weight"], None, self.status, out=out, out_group=1,
                          out_group_stride=stride)

    def _att(self, q, hist2, names):
        p, k, ws = self.params, self.k, self.ws
        feat = k.dien_att_feat_fwd(q, hist2)                              # [q, h, q - h, q * h] (net.py:246-251)
        a1 = k.gemm(feat, p[names[0] + ".weight"], ws, epilogue="bias_sigmoid", bias=p[names[0] + ".bias"])
        a2 = k.gemm(a1, p[names[1] + ".weight"], ws, epilogue="bias_sigmoid", bias=p[names[1] + ".bias"])
        s = k.gemm(a2, p[names[2] + ".weight"], ws, epilogue="bias", bias=p[names[2] + ".bias"])
        return feat, a1, a2, s

    def forward(self, inputs_tensor, is_infer=0, _keep=None):
        sparse, price = inputs_tensor[0], inputs_tensor[1]
        p, k, ws = self.params, self.k, self.ws
        E, O, T, L = self.main_embedding_size, self.other_embedding_size, self.history_length, self.inp_length
        B = sparse.shape[0]
        if sparse.shape[1] != 5 * T + 17:
            raise ValueError("DMR: the sparse feed has %d columns, expected 5 * %d + 17" % (sparse.shape[1], T))
        train = _keep is not None
        f32 = dict(dtype=torch.float32, device=self.device)
        btag, cate_his, brand_his = (sparse[:, i * T:(i + 1) * T].contiguous() for i in range(3))
        mask = sparse[:, 3 * T:4 * T]                                     # strided views: the kernels take a row stride
        mm = sparse[:, 5 * T - 2:5 * T - 1]                               # match_mask[:, T-2]
        sc = dict(zip(SCALARS, sparse[:, 5 * T:].t().contiguous()))       # 17 contiguous [B] id columns
        pos_ids, _ = self._const_ids(B)
        inp = torch.empty(B, L, **f32)
        col = lambda n: inp[:, self.cols[n][0]:self.cols[n][0] + self.cols[n][1]]
        for n, t in USER_FEAT + ITEM_FEAT + (("pid", "pid_embeddings_var"),):
            self._gather(sc[n], t, col(n), L)
        col("price").copy_(price.reshape(B, 1))
        item_eb = inp[:, self.cols["cate_id"][0]:self.cols["cate_id"][0] + 2 * E]      # [cat | brand] (net.py:477)
        hist = torch.empty(B, T, 2 * E, **f32)
        h2 = hist.view(B * T, 2 * E)
        self._gather(cate_his.view(-1), "cat_embeddings_var", h2, 2 * E)
        self._gather(brand_his.view(-1), "brand_embeddings_var", h2[:, E:], 2 * E)
        ctx_dm = torch.empty(B * T, 2 * O, **f32)                         # [dm_position | dm_btag] (net.py:490-502)
        self._gather(pos_ids, "dm_position_embeddings_var", ctx_dm, 2 * O)
        self._gather(btag.view(-1), "dm_btag_embeddings_var", ctx_dm[:, O:], 2 * O)
        W2 = 2 * E + 2 * O
        q2in = torch.empty(B * T, W2, **f32)                              # [item_eb tiled | position | btag] (net.py:311-319)
        tile = lambda ids: ids.view(B, 1).expand(B, T).reshape(-1)
        self._gather(tile(sc["cate_id"]), "cat_embeddings_var", q2in, W2)
        self._gather(tile(sc["brand"]), "brand_embeddings_var", q2in[:, E:], W2)
        self._gather(pos_ids, "position_embeddings_var", q2in[:, 2 * E:], W2)
        self._gather(btag.view(-1), "btag_embeddings_var", q2in[:, 2 * E + O:], W2)
        # ---- user-to-item (deep_match, net.py:239-303): rows T-2 and T-1 only
        q1p = k.gemm(ctx_dm, p["query_layer.weight"], ws, epilogue="bias", bias=p["query_layer.bias"])
        q1 = k.prelu_fwd(q1p, p["query_prelu._weight"], period=T, base=0)
        n1 = ("att_layer1_layer", "att_layer2_layer", "att_layer3_layer")
        feat1, a11, a12, s1 = self._att(q1, h2, n1)
        rows1 = (T - 2, T - 1)
        pooled, w1 = k.dmr_prefix_pool_fwd(s1.view(B, T), mask, hist, rows1)
        pooled2 = pooled.view(2 * B, 2 * E)
        d1p = k.gemm(pooled2, p["dnn_layer1_layer.weight"], ws, epilogue="bias", bias=p["dnn_layer1_layer.bias"])
        uv = k.prelu_fwd(d1p, p["dnn_layer1_prelu._weight"], period=2, base=T - 2).view(B, 2, E)
        # ---- item-to-item (dmr_fcn_attention, net.py:305-357)
        q2p = k.gemm(q2in, p["query_layer2.weight"], ws, epilogue="bias", bias=p["query_layer2.bias"])
        q2 = k.prelu_fwd(q2p, p["query_prelu2._weight"], period=T, base=0)
        n2 = ("att_layer1_layer2", "att_layer2_layer2", "att_layer3_layer2")
        feat2, a21, a22, s2 = self._att(q2, h2, n2)
        _, w2 = k.dmr_prefix_pool_fwd(s2.view(B, T), mask, hist, (T - 1,), out=col("att"), rel=col("rel_i2i"))
        # ---- tail: sum_t hist, item_eb * sum, rel_u2i, user_vector2
        V = p["dm_item_vectors_var.weight"]
        U2 = k.dmr_tail_fwd(hist, item_eb, uv, mm, V, sc["cate_id"], col("hist_sum"), col("prod"), col("rel_u2i"),
                            self.status)
        aux = lse = None
        label_aux = cate_his[:, T - 1]
        if not is_infer:
            aux, lse, _ = k.dmr_match_loss_fwd(U2, V, None, label_aux, ws, self.status)       # x 0.1 by the caller
        # ---- tower (net.py:531-542)
        bn, sm, si = k.batchnorm_fwd(inp, p["inp_layer.weight"], p["inp_layer.bias"], p["inp_layer._mean"],
                                     p["inp_layer._variance"], ws, training=self.training and not is_infer,
                                     momentum=BN_MOMENTUM, eps=BN_EPS)
        x, tower = bn, []
        for i in range(4):
            z = k.gemm(x, p["dnn%d_layer.weight" % i], ws, epilogue="bias", bias=p["dnn%d_layer.bias" % i])
            tower.append((x, z))
            x = k.prelu_fwd(z, p["dnn%d_prelu._weight" % i])
        if train:
            _keep.update(sc=sc, btag=btag, cate_his=cate_his, brand_his=brand_his, mask=mask, mm=mm, pos_ids=pos_ids,
                         inp=inp, item_eb=item_eb, hist=hist, ctx_dm=ctx_dm, q2in=q2in, q1p=q1p, q1=q1, feat1=feat1, a11=a11,
                         a12=a12, rows1=rows1, pooled2=pooled2, w1=w1, d1p=d1p, uv=uv, q2p=q2p, q2=q2, feat2=feat2, a21=a21,
                         a22=a22, w2=w2, U2=U2, lse=lse, label_aux=label_aux, sm=sm, si=si, tower=tower, col=col)
        if is_infer:
            y_hat, _, _ = k.bce_with_logits(x, torch.zeros(B, 1, **f32), ws)
            return y_hat, torch.ones(1, **f32)
        return x, aux

    def __call__(self, inputs_tensor, is_infer=0):
        """net.py:393: (y_hat, loss).  Training mode also needs the gradients: use train_step."""
        if is_infer:
            return self.forward(inputs_tensor, 1)
        sparse = inputs_tensor[0]
        logit, aux = self.forward(inputs_tensor, 0)
        label = sparse[:, -1].to(torch.float32).reshape(-1, 1).contiguous()
        y_hat, _, ctr = self.k.bce_with_logits(logit, label, self.ws)
        return y_hat, ctr + 0.1 * aux

    # ---------------------------------------------------------------- training
    def _adam_rows(self, ids, grad_view, name, row_stride, step, lr):
        k, table = self.k, self.params[name + ".weight"]
        grp = self._grouped(ids.numel(), ids, table.shape[0], None, self.status)      # one IdGroups per id count
        lay = dict(grad_group=1, grad_group_stride=row_stride)
        pp = k.segment_partials(grp, grad_view, table.shape[1], **lay)
        k.adam_rows_all(grp, grad_view, 1, table, self._tm[name], self._tv[name], step, lr, partials=pp, **lay)

    def train_step(self, inputs_tensor, lr=0.008):
        """dygraph_model.py:85-95 train_forward + backward + Adam.  -> (loss [1], y_hat [B,1], aux [1] (x 0.1), ctr [1])."""
        p, k, ws, g = self.params, self.k, self.ws, self._gb
        E, O, T, L = self.main_embedding_size, self.other_embedding_size, self.history_length, self.inp_length
        sparse = inputs_tensor[0]
        B = sparse.shape[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.step_count += 1
        sv = {}
        logit, aux_raw = self.forward(inputs_tensor, 0, _keep=sv)
        label = sparse[:, -1].to(torch.float32).reshape(B, 1).contiguous()
        y_hat, dz, ctr = k.bce_with_logits(logit, label, ws)
        aux = aux_raw * 0.1                                               # net.py:511
        loss = ctr + aux
        col, sc, hist, mask, mm = sv["col"], sv["sc"], sv["hist"], sv["mask"], sv["mm"]
        V = p["dm_item_vectors_var.weight"]
        Cn = V.shape[0]

        def lin_bwd(name, x, dy, act=None):
            kw = dict(epilogue="dsigmoid", aux0=act) if act is not None else {}
            return k.linear_backward(x, dy, p[name + ".weight"], ws, g[name + ".weight"], g[name + ".bias"], **kw)

        # ---- tower and BatchNorm
        d = dz
        for i in (3, 2, 1, 0):
            x, z = sv["tower"][i]
            d, _ = k.prelu_bwd(z, d, p["dnn%d_prelu._weight" % i], ws, dalpha=g["dnn%d_prelu._weight" % i])
            d = lin_bwd("dnn%d_layer" % i, x, d)
        d_inp, _, _ = k.batchnorm_bwd(sv["inp"], d, p["inp_layer.weight"], sv["sm"], sv["si"], ws,
                                      dgamma=g["inp_layer.weight"], dbeta=g["inp_layer.bias"])
        dcol = lambda n: d_inp[:, self.cols[n][0]:self.cols[n][0] + self.cols[n][1]]
        # gradient rows of the two history tables: [B*T rows of d_hist | B rows of d_item_eb], [cat | brand] columns
        GH = torch.empty(B * T + B, 2 * E, **f32)
        GHh = GH[:B * T].view(B, T, 2 * E)
        GV = torch.empty(Cn + B, E, **f32)                                # dense dV | the rows of the cate_id lookup

        def att_bwd(ds, q, feat, a1, a2, names):
            dd = lin_bwd(names[2], a2, ds.view(B * T, 1), act=a2)
            dd = lin_bwd(names[1], a1, dd, act=a1)
            dfeat = lin_bwd(names[0], feat, dd)
            dq = torch.empty(B * T, 2 * E, **f32)
            f_hist = k.dien_att_feat_bwd(q, hist.view(B * T, 2 * E), dfeat, dq, accumulate=False)
            return dq, f_hist.view(B, T, 2 * E)                           # d query; the features' share of d_hist

        # ---- item-to-item
        ds2 = k.dmr_prefix_pool_bwd(mask, hist, (T - 1,), sv["w2"], dcol("att"), GHh, d_rel=dcol("rel_i2i"),
                                    accumulate=False)
        dq2, F2 = att_bwd(ds2, sv["q2"], sv["feat2"], sv["a21"], sv["a22"],
                          ("att_layer1_layer2", "att_layer2_layer2", "att_layer3_layer2"))
        dq2p, _ = k.prelu_bwd(sv["q2p"], dq2, p["query_prelu2._weight"], ws, period=T, base=0,
                              dalpha=g["query_prelu2._weight"])
        dq2in = lin_bwd("query_layer2", sv["q2in"], dq2p)                 # [B*T, 2E + 2O]
        # ---- user-to-item
        dU2 = k.dmr_match_loss_bwd(sv["U2"], V, None, sv["label_aux"], sv["lse"], 0.1, GV[:Cn], ws, accumulate=False)
        d_uv = k.dmr_tail_bwd_match(dU2, dcol("rel_u2i"), sv["uv"], mm, V, sc["cate_id"], GV[Cn:])
        dd1p, _ = k.prelu_bwd(sv["d1p"], d_uv.view(2 * B, E), p["dnn_layer1_prelu._weight"], ws, period=2, base=T - 2,
                              dalpha=g["dnn_layer1_prelu._weight"])
        dpool = lin_bwd("dnn_layer1_layer", sv["pooled2"], dd1p)         # [2B, 2E]
        ds1 = k.dmr_prefix_pool_bwd(mask, hist, sv["rows1"], sv["w1"], dpool.view(B, 4 * E), GHh, accumulate=True)
        dq1, F1 = att_bwd(ds1, sv["q1"], sv["feat1"], sv["a11"], sv["a12"],
                          ("att_layer1_layer", "att_layer2_layer", "att_layer3_layer"))
        dq1p, _ = k.prelu_bwd(sv["q1p"], dq1, p["query_prelu._weight"], ws, period=T, base=0,
                              dalpha=g["query_prelu._weight"])
        dctx = lin_bwd("query_layer", sv["ctx_dm"], dq1p)                 # [B*T, 2O]
        c0 = self.cols["cate_id"][0]
        k.dmr_tail_bwd_hist(F1, F2, dcol("hist_sum"), dcol("prod"), sv["item_eb"], col("hist_sum"),
                            d_inp[:, c0:c0 + 2 * E], dq2in, GHh, GH[B * T:])
        # ---- Adam, non-lazy (dygraph_model.py:70-74): every table once, shared tables with their rows merged
        t = self.step_count
        W2 = 2 * E + 2 * O
        _, all_classes = self._const_ids(B)
        jobs = [(sc[n], dcol(n), tab, L) for n, tab in USER_FEAT + ITEM_FEAT + (("pid", "pid_embeddings_var"),)
                if n not in ("cate_id", "brand")]
        jobs += [(torch.cat([sv["cate_his"].view(-1), sc["cate_id"]]), GH, "cat_embeddings_var", 2 * E),
                 (torch.cat([sv["brand_his"].view(-1), sc["brand"]]), GH[:, E:], "brand_embeddings_var", 2 * E),
                 (sv["btag"].view(-1), dq2in[:, 2 * E + O:], "btag_embeddings_var", W2),
                 (sv["pos_ids"], dq2in[:, 2 * E:], "position_embeddings_var", W2),
                 (sv["btag"].view(-1), dctx[:, O:], "dm_btag_embeddings_var", 2 * O),
                 (sv["pos_ids"], dctx, "dm_position_embeddings_var", 2 * O),
                 (torch.cat([all_classes, sc["cate_id"]]), GV, "dm_item_vectors_var", E)]
        self._last = dict(jobs=jobs, d_inp=d_inp, GH=GH, GV=GV, ds1=ds1, ds2=ds2, dz=dz)
        for ids, gv, name, rs in jobs:
            self._adam_rows(ids, gv, name, rs, t, lr)
        f = self.flat.flat
        k.adam_dense(f["p"], f["m"], f["v"], f["g"], t, lr)
        return loss, y_hat, aux, ctr

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}, tables dense (tests and debugging: host
        index_add over the recorded gradient rows)."""
        out = {k: v.clone() for k, v in self._gb.items()}
        for ids, gv, name, rs in self._last["jobs"]:
            out[name + ".weight"] = scatter_rows(self.params[name + ".weight"], ids, gv, rs)      # every table once
        return out


class DygraphModel:
    """dmr/dygraph_model.py:23-105 — same method names; tensors are torch device tensors."""

    def create_model(self, config, device="cuda", kernels=None):
        g = lambda key: config.get("hyper_parameters." + key)
        return DMRLayer(g("user_size"), g("cms_segid_size"), g("cms_group_id_size"), g("final_gender_code_size"),
                        g("age_level_size"), g("pvalue_level_size"), g("shopping_level_size"), g("occupation_size"),
                        g("new_user_class_level_size"), g("adgroup_id_size"), g("cate_size"), g("campaign_id_size"),
                        g("customer_size"), g("brand_size"), g("btag_size"), g("pid_size"), g("main_embedding_size"),
                        g("other_embedding_size"), device=device, kernels=kernels)

    def create_feeds(self, batch, config, device="cuda"):
        """dygraph_model.py:61-67: batch = (sparse [B, 267] i64, price [B,1] f32) from reader.AlimamaReader."""
        sparse, price = (torch.as_tensor(x).to(device) for x in batch[:2])
        return sparse[:, -1].reshape(-1, 1), [sparse, price.to(torch.float32).reshape(-1, 1)]

    def create_metrics(self, device="cuda"):
        return auc_metrics(device)

    def _auc(self, dy_model, metrics_list, pred, label):
        if metrics_list:
            auc_update(dy_model.k, metrics_list[0], pred, label)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        label, feeds = self.create_feeds(batch_data, config, dy_model.device)
        lr = config.get("hyper_parameters.optimizer.learning_rate", 0.001)
        loss, pred, _, _ = dy_model.train_step(feeds, lr=lr)
        self._auc(dy_model, metrics_list, pred, label)
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        label, feeds = self.create_feeds(batch_data, config, dy_model.device)
        pred, _ = dy_model.forward(feeds, 1)
        self._auc(dy_model, metrics_list, pred, label)
        return metrics_list, None
