"""Host-side mirror of the reference's BST plugin (models/rank/bst/net.py:22-457 BSTLayer / BST, dygraph_model.py) on the
recengine HIP kernels: Behavior Sequence Transformer, the fourth net of the DIN -> DIEN -> DMR -> BST line and the first
with a Transformer encoder block.

Kept as the reference writes it, oddities included (QUIRKS below).  What is computed differently, with the same result:
  * the three projections q_liner / k_liner / v_liner are ONE GEMM on a packed [d_model, 2 H d_key + H d_value] weight
    image; the three parameters (and their Adagrad accumulators) are column ranges of that image and stay separate in
    state_dict and in the optimizer state;
  * the attention never builds the [B, H, L, L] products (rec_mha_fwd / rec_mha_bwd read q, k, v as column ranges of the
    packed projection and write the combined-heads layout);
  * the two concats in front of the encoder and the one in front of the DNN are no copies: rec_bst_embed_fwd writes the
    six sequence lookups into X and the user row into row 0 of the tower input, and the last step of the encoder writes
    rows 1.. of it;
  * a residual add directly in front of a layer norm is one pass (rec_add_layer_norm_fwd); two dropouts back to back are
    one rec_dropout with two mask streams.
Every Linear and weight gradient is rec_gemm_f32 (REC_EPI_BIAS) with rec_leaky_relu_* behind it; the loss is
rec_sigmoid_logloss (epsilon 1e-4), AUC rec_auc_histogram, the optimizer rec_adagrad_rows on the merged touched rows of
the seven tables (a zero gradient is an exact no-op for Adagrad, so this equals the dense update) and one rec_adagrad_dense
over the flat buffer of everything else.  The only torch work on the step's path is allocation and id plumbing.  The train
step is eager (no graph capture)."""
import math

import torch

from . import ops
from .net_base import FlatStore, LayerBase, auc_metrics, auc_update, scatter_rows

TABLES = ("hist_item_emb_attr", "hist_cat_emb_attr", "hist_position_emb_attr", "target_item_emb_attr",
          "target_cat_emb_attr", "target_position_emb_attr", "userid_attr")
LN_EPS, LEAKY_SLOPE, LOG_EPS = 1e-5, 0.01, 1e-4
ADAGRAD_EPS, ADAGRAD_INIT, LR = 1e-6, 0.0, 1e-3           # PiecewiseDecay([10, 20, 50], [1e-3, ...]) is never stepped
QUIRKS = ("preprocess_cmd is read from the key hyper_parameters.postprocess_cmd (both are 'da' with the shipped YAMLs: no "
          "layer norm runs; 'n' only when the key is absent); attention is unscaled (no 1/sqrt(d_key)) and unmasked (padded "
          "positions, id 0, attend and are attended to); one Dropout(dropout_rate) serves every site and "
          "prepostprocess_dropout only gates by truthiness; relu_dropout, act, n_encoder_layers (one layer, always), "
          "is_sparse and use_DataLoader are unused; layer_norm is parameter-free (epsilon 1e-5, biased variance); the "
          "activations are LeakyReLU(0.01), not ReLU; the DNN runs per position and the logits are summed over the L + 1 "
          "positions; target_* tables are separate parameters and id 0 is a trained row; Adagrad(epsilon 1e-6, accumulator "
          "0) at the fixed rate 1e-3 (the scheduler is never stepped; the YAML's optimizer block is ignored); k_liner.bias "
          "has a structurally zero gradient (softmax shift invariance)")


class BSTLayer(LayerBase):
    """bst/net.py:22-75.  forward(userid, hist_item_seq, hist_cat_seq, position_seq, target_item, target_cat,
    target_position) -> predict [B,1]; train_step(feeds, label) -> (loss [1], predict [B,1])."""

    def __init__(self, user_count, item_emb_size, cat_emb_size, position_emb_size, act, is_sparse, use_DataLoader, item_count,
                 cat_count, position_count, n_encoder_layers, d_model, d_key, d_value, n_head, dropout_rate, postprocess_cmd,
                 preprocess_cmd, prepostprocess_dropout, d_inner_hid, relu_dropout, layer_sizes, device="cuda", kernels=None,
                 dropout_seed=12345):
        self._init_runtime(device, kernels)
        widths = (int(item_emb_size), int(cat_emb_size), int(position_emb_size))
        dm, dk, dv, H = int(d_model), int(d_key), int(d_value), int(n_head)
        if sum(widths) != dm:
            raise ValueError("BST: item + cat + position width %d must equal d_model %d (net.py:435-442)" % (sum(widths), dm))
        if H * dv != dm:
            raise ValueError("BST: n_head * d_value = %d must equal d_model %d (po_liner, net.py:247-249)" % (H * dv, dm))
        if dk % 4 or dv % 4 or not 0 < dk <= ops.MHA_MAX_D or not 0 < dv <= ops.MHA_MAX_D:
            raise ValueError("BST: d_key %d / d_value %d must be multiples of 4, at most %d (rec_mha_*)" % (dk, dv, ops.MHA_MAX_D))
        self.widths, self.d_model, self.d_key, self.d_value, self.n_head = widths, dm, dk, dv, H
        self.d_inner_hid, self.layer_sizes = int(d_inner_hid), [int(x) for x in layer_sizes]
        self.dropout_rate, self.dropout_seed = float(dropout_rate or 0.0), int(dropout_seed)
        self.prepostprocess_dropout = prepostprocess_dropout
        self.preprocess_cmd, self.postprocess_cmd = str(preprocess_cmd), str(postprocess_cmd)
        # stored and unused, as in the reference
        self.act, self.is_sparse, self.use_DataLoader, self.n_encoder_layers = act, is_sparse, use_DataLoader, n_encoder_layers
        self.relu_dropout = relu_dropout
        f32 = dict(dtype=torch.float32, device=self.device)
        counts = (item_count, cat_count, position_count, item_count, cat_count, position_count, user_count)
        self.params, self._acc = {}, {}
        for name, rows, w in zip(TABLES, counts, widths + widths + (dm,)):        # TruncatedNormal(0, 0.1 / sqrt(width))
            std = 0.1 / math.sqrt(float(w))
            t = torch.empty(int(rows), w, **f32)
            torch.nn.init.trunc_normal_(t, 0.0, std, -2 * std, 2 * std)
            self.params["bst.%s.weight" % name] = t
            self._acc["bst.%s.weight" % name] = torch.full_like(t, ADAGRAD_INIT)
        sizes = [dm] + self.layer_sizes + [1]
        self.num_dnn = len(sizes) - 1
        self.qkv_cols = (0, H * dk, 2 * H * dk, 2 * H * dk + H * dv)
        lin = [("bst.dnn_linear_%d" % i, sizes[i], sizes[i + 1], 0.1 / math.sqrt(sizes[i])) for i in range(self.num_dnn)]
        lin += [("bst.hid_l", dm, self.d_inner_hid, 0.1 / math.sqrt(self.d_inner_hid)),
                ("bst.hid2_l", self.d_inner_hid, dm, 0.1 / math.sqrt(dm)),
                ("bst._qkv", dm, self.qkv_cols[3], None),
                ("bst.po_liner", dm, dm, 0.1 / math.sqrt(dm))]
        shapes = []
        for n, i, o, _ in lin:
            shapes += [(n + ".weight", (i, o)), (n + ".bias", (o,))]
        shapes.append(("bias", (1,)))
        # everything but the tables: one flat buffer each for the values, the gradients and the accumulators ("a")
        self.flat = FlatStore(shapes, self.device, stores=("p", "g", "a"), fill={"a": ADAGRAD_INIT})
        self._gb = dict(self.flat.view["g"])
        self.params.update(self.flat.view["p"])
        self._acc.update(self.flat.view["a"])
        for n, i, o_, std in lin:
            if std is not None:
                self.params[n + ".weight"].normal_(0.0, std)
        # the three projections: column ranges of the packed image, separate entries everywhere else
        c = self.qkv_cols
        for j, (n, std) in enumerate((("q_liner", 0.1 / math.sqrt(dm)), ("k_liner", 0.1 / math.sqrt(dk)),
                                      ("v_liner", 0.1 / math.sqrt(dv)))):
            for store in (self.params, self._gb, self._acc):
                store["bst.%s.weight" % n] = store["bst._qkv.weight"][:, c[j]:c[j + 1]]
                store["bst.%s.bias" % n] = store["bst._qkv.bias"][c[j]:c[j + 1]]
            self.params["bst.%s.weight" % n].normal_(0.0, std)
        self._packed = {s: (store.pop("bst._qkv.weight"), store.pop("bst._qkv.bias"))
                        for s, store in (("p", self.params), ("g", self._gb), ("a", self._acc))}
        # the 'd' letters of the four pre / post-process calls, in forward order, own mask streams 0 .. npp-1 of a step;
        # the softmax weights own stream npp and the dropout behind hid2_l stream npp + 1
        self.num_pp_sites = (3 * self.preprocess_cmd + self.postprocess_cmd).count("d")
        self.streams_per_step = self.num_pp_sites + 2

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        return dict(self.params)

    def _optimizer_views(self):
        """The Adagrad accumulator of every parameter, under the parameter's own name."""
        return {"bst.acc." + n: a for n, a in self._acc.items()}

    # ---------------------------------------------------------------- dropout sites
    def dropout_streams(self, step):
        """{site: mask stream} of training step `step` (1-based) — "pp0".., "att", "ffn" — for the sites that are active
        (tests rebuild the masks from these with rec_dropout on ones)."""
        if self.dropout_rate <= 0.0:
            return {}
        base, out = step * self.streams_per_step, {}
        if self.prepostprocess_dropout:
            out.update({"pp%d" % i: base + i for i in range(self.num_pp_sites)})
        out["att"] = base + self.num_pp_sites
        out["ffn"] = base + self.num_pp_sites + 1
        return out

    # ---------------------------------------------------------------- pre / post-process (net.py:272-317)
    def _proc(self, x, prev, cmd, st, B, L, Z=None):
        """pre_post_process_layer (prev None) / pre_post_process_layer_ on x [B*L, d_model].  st: {"streams", "site"}.
        Z [B, L+1, d_model]: the result goes to rows 1.. of every sample.  -> (out, tape).  x is never overwritten when
        prev is None; with prev, x (a fresh GEMM output) receives the sum."""
        k, dm = self.k, self.d_model
        steps = []
        for c in cmd:
            if c == "n":
                steps.append(["n"])
            elif c == "d":
                s = st["streams"].get("pp%d" % st["site"])
                st["site"] += 1
                if s is None:
                    continue
                if steps and steps[-1][0] == "d" and len(steps[-1]) == 2:
                    steps[-1].append(s)                                   # back to back: one pass, two mask streams
                else:
                    steps.append(["d", s])
        Zv = Z.view(B, (L + 1) * dm)[:, dm:] if Z is not None else None   # [B, L*dm]: rows 1.. of every sample
        cur, pending, owned, tape = x, prev, False, []
        for i, step in enumerate(steps):
            last = i == len(steps) - 1
            if step[0] == "n":
                grouped = last and Z is not None
                cur, _, rstd = k.add_layer_norm_fwd(cur, pending, LN_EPS, out=Z if grouped else None,
                                                    out_group=L if grouped else 0)
                pending, owned = None, False
                tape.append(("n", cur, rstd, grouped))
            else:
                if pending is not None:
                    cur, pending, owned = k.bst_add(cur, pending), None, True
                sb = step[2] if len(step) == 3 else None
                if last and Z is not None:
                    k.dropout(cur.view(B, L * dm), self.dropout_rate, self.dropout_seed, step[1], sb, out=Zv,
                              step_stride=self.streams_per_step)
                    cur = Z
                else:
                    cur = k.dropout(cur, self.dropout_rate, self.dropout_seed, step[1], sb,
                                    out=None if owned else torch.empty_like(cur), step_stride=self.streams_per_step)
                    owned = True
                tape.append(("d", step[1], sb))
        if pending is not None:
            cur = k.bst_add(cur, pending)
        if Z is not None and cur is not Z:
            k.bst_add(cur.view(B, L * dm), None, out=Zv)
            cur = Z
        return cur, tape

    def _proc_bwd(self, g, tape, B, L, from_Z=False):
        """g: the gradient of _proc's result — [B*L, d_model], owned by the caller's chain (overwritten), or with from_Z the
        [B, L+1, d_model] gradient of the tower input.  -> the gradient of x + prev, [B*L, d_model] contiguous."""
        k, dm = self.k, self.d_model
        if from_Z:
            gv = g.view(B, (L + 1) * dm)[:, dm:]
            if tape and tape[-1][0] == "d":
                _, sa, sb = tape[-1]
                g = k.dropout(gv, self.dropout_rate, self.dropout_seed, sa, sb,
                              out=torch.empty(B, L * dm, dtype=torch.float32, device=g.device),
                              step_stride=self.streams_per_step).view(B * L, dm)
                tape = tape[:-1]
            else:
                g = k.bst_add(gv, None, out=torch.empty(B, L * dm, dtype=torch.float32, device=g.device)).view(B * L, dm)
        for step in reversed(tape):
            if step[0] == "d":
                g = k.dropout(g, self.dropout_rate, self.dropout_seed, step[1], step[2], step_stride=self.streams_per_step)
            else:
                g = k.add_layer_norm_bwd(step[1], step[2], g, out=g, y_group=L if step[3] else 0)
        return g

    # ---------------------------------------------------------------- forward
    def _qkv(self, m):
        c = self.qkv_cols
        return m[:, c[0]:c[1]], m[:, c[1]:c[2]], m[:, c[2]:c[3]]

    def _run(self, feeds, streams, keep=None):
        """-> (logit [B,1], B, L).  streams: {} (no dropout) or dropout_streams(step); keep: a dict that receives what the
        backward needs."""
        p, k, ws = self.params, self.k, self.ws
        ids = [feeds[1], feeds[2], feeds[3], feeds[4], feeds[5], feeds[6], feeds[0]]      # TABLES order
        if len(feeds) != 7 or ids[0].dim() != 2:
            raise ValueError("BST takes userid, hist_item_seq, hist_cat_seq, position_seq [B,T], target_item, target_cat, "
                             "target_position")
        B, T = ids[0].shape
        L, dm, H = T + 1, self.d_model, self.n_head
        f32 = dict(dtype=torch.float32, device=self.device)
        X, Z = torch.empty(B * L, dm, **f32), torch.empty(B, L + 1, dm, **f32)
        k.bst_embed_fwd(ids, [p["bst.%s.weight" % n] for n in TABLES], X, Z, self.status)
        st = dict(streams=streams, site=0)
        lin = lambda x, n: k.gemm(x, p[n + ".weight"], ws, epilogue="bias", bias=p[n + ".bias"])
        # encoder_layer (net.py:400-416)
        a_in, tape0 = self._proc(X, None, self.preprocess_cmd, st, B, L)
        qkv = k.gemm(a_in, self._packed["p"][0], ws, epilogue="bias", bias=self._packed["p"][1])
        q, kk, v = self._qkv(qkv)
        s_att = streams.get("att")
        p_att = self.dropout_rate if s_att is not None else 0.0
        ctx, lse = k.mha_fwd(q, kk, v, B, L, H, 1.0, p_att, self.dropout_seed, s_att or 0)
        att = lin(ctx, "bst.po_liner")
        A, tape1 = self._proc(att, X, self.postprocess_cmd, st, B, L)
        a1 = k.leaky_relu_fwd(lin(A, "bst.hid_l"), LEAKY_SLOPE)
        f = lin(a1, "bst.hid2_l")
        s_ffn = streams.get("ffn")
        if s_ffn is not None:
            k.dropout(f, self.dropout_rate, self.dropout_seed, s_ffn, step_stride=self.streams_per_step)
        # the second residual and the final pre-process (net.py:414-416, 450) are one chain of steps on f + A
        _, tape2 = self._proc(f, A, 2 * self.preprocess_cmd, st, B, L, Z=Z)
        x, acts = Z.view(B * (L + 1), dm), []
        for i in range(self.num_dnn):
            y = lin(x, "bst.dnn_linear_%d" % i)
            if i < self.num_dnn - 1:
                k.leaky_relu_fwd(y, LEAKY_SLOPE)
            acts.append((x, y))
            x = y
        logit = k.bst_possum_fwd(x, p["bias"], B)
        if keep is not None:
            keep.update(ids=ids, X=X, Z=Z, a_in=a_in, tape0=tape0, qkv=qkv, ctx=ctx, lse=lse, p_att=p_att, s_att=s_att or 0,
                        tape1=tape1, A=A, a1=a1, s_ffn=s_ffn, tape2=tape2, acts=acts)
        return logit, B, L

    def forward(self, userid, hist_item_seq, hist_cat_seq, position_seq, target_item, target_cat, target_position):
        """net.py:67-75 -> predict [B,1].  Train mode draws the masks the next train_step would."""
        feeds = [userid, hist_item_seq, hist_cat_seq, position_seq, target_item, target_cat, target_position]
        streams = self.dropout_streams(self.step_count + 1) if self.training else {}
        logit, B, _ = self._run(feeds, streams)
        pred, _, _ = self.k.sigmoid_logloss(logit, None, None, torch.zeros(B, 1, dtype=torch.int64, device=self.device),
                                            self.ws, eps=LOG_EPS, want_dz=False)
        return pred

    __call__ = forward

    # ---------------------------------------------------------------- training
    def _adagrad_rows(self, ids, grad, name, lr, row_stride=0):
        k, table = self.k, self.params[name]
        grp = self._grouped(ids.numel(), ids, table.shape[0], None, self.status)      # one IdGroups per id count
        lay = dict(grad_group=1, grad_group_stride=row_stride) if row_stride else {}
        pp = k.segment_partials(grp, grad, table.shape[1], **lay)
        k.adagrad_rows(grp, grad, 1, table, self._acc[name], lr, ADAGRAD_EPS, partials=pp, **lay)

    def train_step(self, feeds, label, lr=LR):
        """dygraph_model.py:103-115 train_forward + backward + Adagrad.  feeds: the seven id tensors of forward(); label
        [B,1] i64.  -> (loss [1], predict [B,1])."""
        p, k, ws, g = self.params, self.k, self.ws, self._gb
        self.step_count += 1
        streams = self.dropout_streams(self.step_count) if self.training else {}
        sv = {}
        logit, B, L = self._run(feeds, streams, keep=sv)
        T, dm, H = L - 1, self.d_model, self.n_head
        pred, dz, loss = k.sigmoid_logloss(logit, None, None, label.reshape(B, 1).to(torch.int64).contiguous(), ws, eps=LOG_EPS)
        lin_bwd = lambda n, x, dy: k.linear_backward(x, dy, p[n + ".weight"], ws, g[n + ".weight"], g[n + ".bias"])
        # the sum over the positions, the per-position DNN
        d = k.bst_possum_bwd(dz, L + 1, g["bias"])
        for i in reversed(range(self.num_dnn)):
            x, y = sv["acts"][i]
            if i < self.num_dnn - 1:
                k.leaky_relu_bwd(y, d, LEAKY_SLOPE)
            d = lin_bwd("bst.dnn_linear_%d" % i, x, d)
        dZ = d.view(B, L + 1, dm)
        # the encoder layer, backwards
        gE = self._proc_bwd(dZ, sv["tape2"], B, L, from_Z=True)            # d (f + A)
        gf = gE
        if sv["s_ffn"] is not None:
            gf = k.dropout(gE, self.dropout_rate, self.dropout_seed, sv["s_ffn"], out=torch.empty_like(gE),
                           step_stride=self.streams_per_step)
        da1 = lin_bwd("bst.hid2_l", sv["a1"], gf)
        k.leaky_relu_bwd(sv["a1"], da1, LEAKY_SLOPE)
        gA = k.bst_add(lin_bwd("bst.hid_l", sv["A"], da1), gE)
        g_att = self._proc_bwd(gA, sv["tape1"], B, L)                      # d (att + X)
        d_ctx = lin_bwd("bst.po_liner", sv["ctx"], g_att)
        dqkv = torch.empty_like(sv["qkv"])
        q, kk, v = self._qkv(sv["qkv"])
        k.mha_bwd(q, kk, v, B, L, H, sv["ctx"], sv["lse"], d_ctx, 1.0, sv["p_att"], self.dropout_seed, sv["s_att"],
                  grads=self._qkv(dqkv))
        g_ain = k.linear_backward(sv["a_in"], dqkv, self._packed["p"][0], ws, self._packed["g"][0], self._packed["g"][1])
        dX = k.bst_add(self._proc_bwd(g_ain, sv["tape0"], B, L), g_att)
        # Adagrad: the merged touched rows of the seven tables, then everything else in one pass
        rows = k.bst_embed_bwd(dX, B, T, self.widths)
        ids = sv["ids"]
        jobs = [(ids[i].contiguous().view(-1), rows[i], "bst.%s.weight" % TABLES[i], 0) for i in range(6)]
        jobs.append((ids[6].contiguous().view(-1), dZ[:, 0, :], "bst.userid_attr.weight", (L + 1) * dm))
        self._last = dict(jobs=jobs, dX=dX, dZ=dZ, dz=dz, dqkv=dqkv, d_ctx=d_ctx)
        for idv, gv, name, rs in jobs:
            self._adagrad_rows(idv, gv, name, lr, rs)
        f = self.flat.flat
        k.adagrad_dense(f["p"], f["a"], f["g"], lr, ADAGRAD_EPS)
        return loss, pred

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}, tables dense (tests and debugging: host
        index_add over the recorded gradient rows)."""
        out = {n: v.clone() for n, v in self._gb.items()}
        for idv, gv, name, rs in self._last["jobs"]:
            out[name] = scatter_rows(self.params[name], idv, gv, rs or self.params[name].shape[1])
        return out


class DygraphModel:
    """bst/dygraph_model.py:23-126 — same method names; tensors are torch device tensors."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        postprocess_cmd = g("hyper_parameters.postprocess_cmd", "da")
        preprocess_cmd = g("hyper_parameters.postprocess_cmd", "n")           # dygraph_model.py:46: the wrong key, kept
        return BSTLayer(g("hyper_parameters.user_count", 192403), g("hyper_parameters.item_emb_size", 64),
                        g("hyper_parameters.cat_emb_size", 64), g("hyper_parameters.position_emb_size", 64),
                        g("hyper_parameters.act", "sigmoid"), g("hyper_parameters.is_sparse", False),
                        g("hyper_parameters.use_DataLoader", False), g("hyper_parameters.item_count", 63001),
                        g("hyper_parameters.cat_count", 801), g("hyper_parameters.position_count", 5001),
                        g("hyper_parameters.n_encoder_layers", 1), g("hyper_parameters.d_model", 96),
                        g("hyper_parameters.d_key", None), g("hyper_parameters.d_value", None),
                        g("hyper_parameters.n_head", None), g("hyper_parameters.dropout_rate", 0.0), postprocess_cmd,
                        preprocess_cmd, g("hyper_parameters.prepostprocess_dropout", 0.0),
                        g("hyper_parameters.d_inner_hid", 512), g("hyper_parameters.relu_dropout", 0.0),
                        g("hyper_parameters.fc_sizes", None), device=device, kernels=kernels,
                        dropout_seed=g("runner.seed", 12345))

    def create_feeds(self, batch_data, config, device="cuda"):
        """dygraph_model.py:63-73: eight int64 arrays — label, userid, history, cate, position, target, target_cate,
        target_position (reader.AmazonBSTReader) -> (label [B,1], the seven feeds of forward())."""
        t = [torch.as_tensor(b).to(device).to(torch.int64) for b in batch_data]
        t = [x.reshape(x.shape[0], -1) for x in t]
        return t[0], t[1:8]

    def create_metrics(self, device="cuda"):
        return auc_metrics(device)

    def _auc(self, dy_model, metrics_list, pred, label):
        if metrics_list:
            auc_update(dy_model.k, metrics_list[0], pred, label)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        label, feeds = self.create_feeds(batch_data, config, dy_model.device)
        loss, pred = dy_model.train_step(feeds, label, LR)                # the YAML's learning rate is not read
        self._auc(dy_model, metrics_list, pred, label)
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        label, feeds = self.create_feeds(batch_data, config, dy_model.device)
        was = dy_model.training
        dy_model.eval()
        pred = dy_model.forward(*feeds)
        dy_model.training = was
        self._auc(dy_model, metrics_list, pred, label)
        return metrics_list, None
