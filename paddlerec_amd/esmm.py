"""Host-side mirror of the reference's ESMM plugin (models/multitask/esmm/net.py:21-111 ESMMLayer, dygraph_model.py) on the
recengine HIP kernels: two MLP towers (ctr, cvr) over the padded multi-field embedding sum-pool, pCTCVR = pCTR * pCVR.

  * features: rec_field_sumpool_fwd (esm.py) — ids [B, F, L] -> [B, F*D];
  * the towers' first Linears both read the features: they are the column ranges of ONE packed image [F*D, h_ctr + h_cvr],
    so the forward is one GEMM (bias + ReLU) and the backward one dW and one dX GEMM; later layers are per tower
    (ops.gemm / ops.linear_backward).  A tower without hidden layers has its two logits in the image, without the ReLU;
  * the head is rec_esm_head in the ESMM mode (no clip, no counterfactual term, weights 0 and 1).  It returns
    dz0 = -dz1 exactly, so below a tower's last Linear d a = d z1 (W[:, 1] - W[:, 0]), as in mtl.py;
  * Adam (beta 0.9 / 0.999, epsilon 1e-8, non-lazy) is one rec_adam_dense over the flat buffer of both towers and
    adam_rows_all on the table.
Names are the reference's: embedding.weight and linear_0 .. linear_{n_ctr + n_cvr + 1} (net.py:56, 75)."""
import math

import torch

from .esm import EsmDygraphModel, EsmLoss, FieldTable, out_list
from .mtl import ADAM_EPS, BETA1, BETA2, STORES
from .net_base import FlatStore, LayerBase

QUIRKS = ("no clip on the softmax outputs (ESCM2 clips, ESMM does not); log_loss has epsilon 1e-4; the loss is the batch mean "
          "of log_loss(pCTR, click) + log_loss(pCTR * pCVR, buy): the cvr tower is trained through the product only; "
          "act_i is registered twice under one name (net.py:60, 80), which holds no parameter; Linear weights are "
          "Normal(0, 1 / sqrt(in)) with zero bias (drawn with torch, not Paddle's random stream), the table Uniform(-1, 1) "
          "with row 0 zero; Adam (beta 0.9 / 0.999, epsilon 1e-8, non-lazy: every table row moves) at "
          "hyper_parameters.optimizer.learning_rate")


class ESMMLayer(LayerBase):
    """esmm/net.py:21-111.  forward(ids [B, num_field, max_len] int64) -> net.py's six outputs; train_step(ids, click [B],
    buy [B], lr) -> (loss, pred [B, 6] = ctr_out | cvr_out | ctcvr_prop)."""
    n_tasks = 2

    def __init__(self, sparse_feature_number, sparse_feature_dim, num_field, ctr_layer_sizes, cvr_layer_sizes, max_len=3,
                 device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        self.emb = FieldTable(sparse_feature_number, sparse_feature_dim, num_field, max_len, self.device, self.k)
        K = int(num_field) * int(sparse_feature_dim)
        hidden = [[int(h) for h in (ctr_layer_sizes or [])], [int(h) for h in (cvr_layer_sizes or [])]]
        if any(h < 1 for hs in hidden for h in hs):
            raise ValueError("ESMM: ctr_fc_sizes and cvr_fc_sizes must hold positive widths")
        self.ctr_layer_sizes, self.cvr_layer_sizes = hidden
        # tower t: widths K -> sizes[t][0] -> ... -> 2; its Linear j is linear_{first[t] + j}
        self.sizes = [hs + [2] for hs in hidden]
        self.first = [0, len(hidden[0]) + 1]
        self.h0 = [s[0] for s in self.sizes]                  # column widths of the packed first layer
        entries = [("W0", (K, sum(self.h0))), ("b0", (sum(self.h0),))]
        for t in range(2):
            for j in range(1, len(self.sizes[t])):
                n = "linear_%d" % (self.first[t] + j)
                entries += [(n + ".weight", (self.sizes[t][j - 1], self.sizes[t][j])), (n + ".bias", (self.sizes[t][j],))]
        self.flat = FlatStore(entries, self.device)
        self._views = {s: {} for s in STORES}
        for s in STORES:
            v, c = self.flat.view[s], 0
            for t in range(2):
                n = "linear_%d" % self.first[t]
                self._views[s][n + ".weight"], self._views[s][n + ".bias"] = v["W0"][:, c:c + self.h0[t]], v["b0"][c:c + self.h0[t]]
                c += self.h0[t]
            for name, _ in entries[2:]:
                self._views[s][name] = v[name]
        n_lin = self.first[1] + len(self.sizes[1])
        self.names = ["linear_%d" % i for i in range(n_lin)]
        self.params = {}
        for n in self.names:                                   # net.py:53-55, 72-74: Normal(std = 1 / sqrt(in)), bias 0
            w = self.params[n + ".weight"] = self._views["p"][n + ".weight"]
            self.params[n + ".bias"] = self._views["p"][n + ".bias"]
            w.normal_(0.0, 1.0 / math.sqrt(w.shape[0]))
        self._minus_plus = torch.tensor([[-1.0], [1.0]], dtype=torch.float32, device=self.device)

    # ---------------------------------------------------------------- parameters
    def state_dict(self):
        sd = {"embedding.weight": self.emb.weight}
        sd.update(self.params)
        return sd

    def _optimizer_views(self):
        """Adam's moments of every parameter, under the parameter's own name."""
        out = self.emb.moment_views()
        out.update(("mtl.%s.%s" % (s, k), self._views[s][k]) for k in self.params for s in ("m", "v"))
        return out

    # ---------------------------------------------------------------- forward
    def _cols(self, t):
        c = sum(self.h0[:t])
        return c, c + self.h0[t]

    def _run(self, ids, keep=None):
        """-> z [B, 4], the towers' logits.  keep: a dict that receives what the backward needs."""
        k, ws, p = self.k, self.ws, self.params
        x = self.emb.pool(ids, self.status)
        B = x.shape[0]
        v = self.flat.view["p"]
        both_hidden = all(len(s) > 1 for s in self.sizes)
        Y = k.gemm(x, v["W0"], ws, epilogue="bias_relu" if both_hidden else "bias", bias=v["b0"])
        z = torch.empty(B, 4, dtype=torch.float32, device=self.device)
        acts = []
        for t in range(2):
            c0, c1 = self._cols(t)
            n = len(self.sizes[t])
            if n == 1:                                         # no hidden layer: the logits are the image's columns
                k.bst_add(Y[:, c0:c1], None, out=z[:, 2 * t:2 * t + 2])
                acts.append([])
                continue
            if not both_hidden:
                k.leaky_relu_fwd(Y[:, c0:c1], 0.0)
            a, chain = Y[:, c0:c1], [Y[:, c0:c1]]
            for j in range(1, n):
                name = "linear_%d" % (self.first[t] + j)
                last = j == n - 1
                a = k.gemm(a, p[name + ".weight"], ws, epilogue="bias" if last else "bias_relu", bias=p[name + ".bias"],
                           out=z[:, 2 * t:2 * t + 2] if last else None)
                if not last:
                    chain.append(a)
            acts.append(chain)                                 # chain[j - 1]: the (post-ReLU) input of Linear j
        if keep is not None:
            keep.update(x=x, Y=Y, acts=acts, B=B)
        return z

    def predict(self, ids):
        """-> pred [B, 6]: ctr_out | cvr_out | (1 - pCTCVR, pCTCVR)."""
        z = self._run(ids)
        none = torch.zeros(z.shape[0], dtype=torch.int64, device=self.device)
        return self.k.esm_head(z, none, none, "ESMM", 1.0, 0.0, 1.0, want_grad=False)[0]

    def forward(self, ids):
        return out_list(self.predict(ids), 2)

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, ids, click, buy, lr=1e-3):
        """dygraph_model.py train_forward + backward + Adam.  -> (loss: an EsmLoss, pred [B, 6])."""
        k, ws, p, g = self.k, self.ws, self.params, self._views["g"]
        self.step_count += 1
        sv = {}
        z = self._run(ids, keep=sv)
        B = sv["B"]
        if tuple(click.shape) != (B,) or tuple(buy.shape) != (B,):
            raise ValueError("click and buy must be int64 [B], got %s and %s" % (tuple(click.shape), tuple(buy.shape)))
        pred, cost, dz = k.esm_head(z, click, buy, "ESMM", 1.0, 0.0, 1.0 / B)
        GY = torch.empty(B, sum(self.h0), dtype=torch.float32, device=self.device)
        for t in range(2):
            c0, c1 = self._cols(t)
            n, chain = len(self.sizes[t]), sv["acts"][t]
            if n == 1:
                k.bst_add(dz[:, 2 * t:2 * t + 2], None, out=GY[:, c0:c1])
                continue
            # the last Linear [h, 2]: d z0 = -d z1 exactly (rec_esm_head), so d a = d z1 (W[:, 1] - W[:, 0]) (mtl.py has why)
            name, a = "linear_%d" % (self.first[t] + n - 1), chain[n - 2]
            k.gemm(a, dz[:, 2 * t:2 * t + 2], ws, trans_a=True, out=g[name + ".weight"], b_colsum=g[name + ".bias"])
            wd = k.gemm(p[name + ".weight"], self._minus_plus, ws)
            d = k.gemm(dz[:, 2 * t + 1:2 * t + 2], wd, ws, trans_b=True, epilogue="relu_mask", aux0=a,
                       out=GY[:, c0:c1] if n == 2 else None)
            for j in range(n - 2, 0, -1):
                name, a = "linear_%d" % (self.first[t] + j), chain[j - 1]
                d = k.linear_backward(a, d, p[name + ".weight"], ws, g[name + ".weight"], g[name + ".bias"], relu_src=a,
                                      out=GY[:, c0:c1] if j == 1 else None)
        v = self.flat.view
        dX = k.linear_backward(sv["x"], GY, v["p"]["W0"], ws, v["g"]["W0"], v["g"]["b0"])
        self._last = dict(dz=dz, dX=dX, ids=ids)
        f = self.flat.flat
        k.adam_dense(f["p"], f["m"], f["v"], f["g"], self.step_count, lr, BETA1, BETA2, ADAM_EPS)
        self.emb.step(ids, dX, self.step_count, lr, self.status)
        return EsmLoss(cost, 1.0, 0.0), pred

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}."""
        g = {kk: self._views["g"][kk].clone() for kk in self.params}
        g["embedding.weight"] = self.emb.dense_gradient(self._last["ids"], self._last["dX"])
        return g


class DygraphModel(EsmDygraphModel):
    """esmm/dygraph_model.py — same method names."""
    METRICS = (("auc_ctr", 0, 0), ("auc_ctcvr", "ctcvr", 1))

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return ESMMLayer(g("hyper_parameters.sparse_feature_number"), g("hyper_parameters.sparse_feature_dim"),
                         g("hyper_parameters.num_field"), g("hyper_parameters.ctr_fc_sizes"), g("hyper_parameters.cvr_fc_sizes"),
                         max_len=g("hyper_parameters.max_len", 3), device=device, kernels=kernels)
