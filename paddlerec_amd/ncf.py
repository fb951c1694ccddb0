"""Host-side mirror of the reference's NCF plugin (models/recall/ncf/net.py NCF_NeuMF_Layer, NCF_GMF_Layer, NCF_MLP_Layer;
dygraph_model.py; evaluate.py) on the recengine HIP kernels: neural collaborative filtering.

The dense side of the shipped net is 2 761 floats, so a step built from gathers, GEMMs and a head is a chain of launches that
each do microseconds of work.  A step here is

  * rec_ncf_step: forward, log loss and backward of the whole net in ONE launch (all weights in LDS) plus a small fold ->
    pred, the loss, the gradient row of every sample's two lookups and the dense gradients;  or, for a tower the LDS cannot
    hold (rec_ncf_fused_eligible) or with REC_NCF_FUSED=0, the general route: rec_ncf_gather_fwd, rec_gemm_f32 with its
    ReLU epilogue per Linear (the last one writes into the prediction input: no concat), rec_gemm_f32 for the head,
    rec_sigmoid_logloss, rec_mlp_head_bwd, rec_relu_mask_inplace, rec_gemm_f32_pair per Linear, rec_ncf_gather_bwd;
  * one rec_ids_group and one rec_adam_rows_all per side: a user's MF and MLP rows are ONE row of a packed [U, Cu] buffer
    (MF first), the items likewise; Adam is elementwise, so the bits equal four separate tables;
  * one rec_adam_dense over the flat dense buffer.
Paddle's dygraph Adam is not lazy: every row of every table moves every step."""
import math
import os

import numpy as np
import torch

from .net_base import LayerBase

MODES = ("NCF_NeuMF", "NCF_GMF", "NCF_MLP")
QUIRKS = ("prediction.in_features is written as layers[2] (NeuMF) or layers[3] (GMF, MLP) in net.py, which equals the true "
          "width only for numbers like the shipped ones; the mirror computes the true width and refuses a configuration for "
          "which the reference's own matmul would fail; GMF builds no MLP tables and MLP no MF tables; the L2Decay(coeff=0) "
          "attributes are no-ops; Adam moves every row of every table on every step (dense or SelectedRows gradient alike); "
          "evaluate.py drops the last log line (result[:-1]), an artefact of parsing a log that is not reproduced")


def prediction_width(mode, mf_dim, layers):
    """The true in_features of `prediction`; ValueError (naming both numbers) when the reference's expression (net.py:82,
    150, 214) is undefined or differs from it — the reference then fails in its matmul."""
    if mode not in MODES:
        raise ValueError("NCF: mode %r is not one of %s" % (mode, ", ".join(MODES)))
    layers = [int(x) for x in layers]
    if mode != "NCF_GMF" and len(layers) < 2:
        raise ValueError("NCF: fc_layers needs at least two entries for a tower, got %s" % (layers,))
    true = {"NCF_NeuMF": lambda: int(mf_dim) + layers[-1], "NCF_GMF": lambda: int(mf_dim), "NCF_MLP": lambda: layers[-1]}[mode]()
    idx = 2 if mode == "NCF_NeuMF" else 3
    if len(layers) <= idx:
        raise ValueError("NCF %s: the reference sizes prediction by fc_layers[%d], which %s does not have (the true width is %d)"
                         % (mode, idx, layers, true))
    if layers[idx] != true:
        raise ValueError("NCF %s: the reference sizes prediction by fc_layers[%d] = %d but its input is %d wide"
                         % (mode, idx, layers[idx], true))
    return true


class NCFLayer(LayerBase):
    """net.py:22-241.  forward(users, items) -> prediction [B, 1];  train_step(users, items, labels, lr) -> loss [1]."""

    def __init__(self, num_users, num_items, mf_dim, layers, mode="NCF_NeuMF", device="cuda", kernels=None):
        self._init_runtime(device, kernels, group_status=True)
        k = self.k
        self.mode, self.num_users, self.num_items = mode, int(num_users), int(num_items)
        self.layers = [int(x) for x in layers]
        self.pred_width = prediction_width(mode, mf_dim, self.layers)
        if self.num_users < 1 or self.num_items < 1:
            raise ValueError("NCF: num_users and num_items must be positive")
        self.mf = 0 if mode == "NCF_MLP" else int(mf_dim)
        self.widths = [] if mode == "NCF_GMF" else list(self.layers)
        if self.widths and (self.widths[0] % 2 or min(self.widths) < 1):
            raise ValueError("NCF: fc_layers[0] must be even and every width positive, got %s" % (self.layers,))
        if mode != "NCF_MLP" and self.mf < 1:
            raise ValueError("NCF: mf_dim must be positive")
        self.half = self.widths[0] // 2 if self.widths else 0
        self.nfc = max(len(self.widths) - 1, 0)
        self.cu = self.mf + self.half
        self.desc = k.ncf_desc(self.num_users, self.num_items, self.mf, self.widths)
        f32 = dict(dtype=torch.float32, device=self.device)
        # the packed tables and their moments, and the flat dense buffer four times
        self.packed = {s: {"user": torch.zeros(self.num_users, self.cu, **f32), "item": torch.zeros(self.num_items, self.cu, **f32)}
                       for s in ("p", "m", "v")}
        self.layout, self.P = k.ncf_dense_layout(self.mf, self.widths)
        self.flat = {s: torch.zeros(self.P, **f32) for s in ("p", "g", "m", "v")}
        self.fused = k.ncf_fused_eligible(self.desc) and os.environ.get("REC_NCF_FUSED", "1") != "0"
        self._init()
        self._scratch, self._buf = {}, {}

    # ---------------------------------------------------------------- parameters
    def _views(self, store):
        """{reference name: view} of one store ("p", "m", "v"; "g": the dense gradients only)."""
        out = {}
        if store != "g":
            u, i = self.packed[store]["user"], self.packed[store]["item"]
            if self.mf:
                out["MF_Embedding_User.weight"], out["MF_Embedding_Item.weight"] = u[:, :self.mf], i[:, :self.mf]
            if self.half:
                out["MLP_Embedding_User.weight"], out["MLP_Embedding_Item.weight"] = u[:, self.mf:], i[:, self.mf:]
        for name, off, shape in self.layout:
            out[name] = self.flat[store][off:off + math.prod(shape)].view(shape)
        return out

    def _init(self):
        """net.py: tables Normal(0, 0.01); layer_i TruncatedNormal(std = 1/sqrt(fan_in)) (two standard deviations), zero
        bias; prediction KaimingUniform, limit sqrt(6 / fan_in) with the fan_in the reference passes (2 layers[2] for NeuMF,
        2 layers[3] for MLP, the weight's own for GMF)."""
        p = self._views("p")
        for name, t in p.items():
            if "Embedding" in name:
                t.copy_(torch.randn(t.shape, device=self.device) * 0.01)
            elif name.startswith("layer_") and name.endswith(".weight"):
                std = 1.0 / math.sqrt(t.shape[0])
                t.copy_(torch.nn.init.trunc_normal_(torch.empty(t.shape, device=self.device), std=std, a=-2 * std, b=2 * std))
        w = p["prediction.weight"]
        w.copy_((torch.rand(w.shape, device=self.device) * 2 - 1) * self.kaiming_limit())

    def kaiming_limit(self):
        fan_in = {"NCF_NeuMF": lambda: 2 * self.layers[2], "NCF_GMF": lambda: self.pred_width,
                  "NCF_MLP": lambda: 2 * self.layers[3]}[self.mode]()
        return math.sqrt(6.0 / fan_in)

    def state_dict(self):
        return self._views("p")

    def moments(self):
        return self._views("m"), self._views("v")

    def load_state_dict(self, sd):
        self.set_dict(sd)

    def _optimizer_views(self):
        """Adam's moments of every parameter, under the parameter's own name."""
        return {"ncf.%s.%s" % (s, k): v for s in ("m", "v") for k, v in self._views(s).items()}

    # ---------------------------------------------------------------- forward
    def _feeds(self, users, items, labels=None):
        out = []
        for t, name in ((users, "users"), (items, "items"), (labels, "labels")):
            if t is None:
                continue
            if t.dtype != torch.int64:
                raise ValueError("%s must be int64, got %s" % (name, t.dtype))
            out.append(t.reshape(-1).contiguous())
        if len({t.numel() for t in out}) != 1:
            raise ValueError("users, items and labels must have one entry per sample")
        return out

    def _general_bufs(self, B):
        """The general route's buffers for a batch of B: pred_in [B, ld] (ld: the prediction width rounded up to 4; the extra
        columns are zero and stay zero), mlp_in [B, widths[0]], d_pred_in [B, ld]."""
        b = self._buf.get(B)
        if b is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            ld = -(-self.pred_width // 4) * 4
            b = self._buf[B] = dict(pred_in=torch.zeros(B, ld, **f32), d_pred_in=torch.zeros(B, ld, **f32),
                                    mlp_in=torch.zeros(B, self.widths[0], **f32) if self.nfc else None)
            if len(self._buf) > 4:
                self._buf.pop(next(iter(self._buf)))
        return b

    def _general_fwd(self, u, i, bufs):
        """-> (logit [B, 1], acts): acts[l] = the input of Linear l + 1."""
        k, p, mf = self.k, self._views("p"), self.mf
        T = self.packed["p"]
        k.ncf_gather_fwd(self.desc, u, i, T["user"], T["item"], bufs["pred_in"] if mf else None, bufs["mlp_in"], self.status)
        x, acts = bufs["mlp_in"], []
        for l in range(1, self.nfc + 1):
            acts.append(x)
            out = bufs["pred_in"][:, mf:mf + self.widths[-1]] if l == self.nfc else None
            x = k.gemm(x, p["layer_%d.weight" % l], self.ws, epilogue="bias_relu", bias=p["layer_%d.bias" % l], out=out)
        logit = k.gemm(bufs["pred_in"][:, :self.pred_width], p["prediction.weight"], self.ws, epilogue="bias",
                       bias=p["prediction.bias"])
        return logit, acts

    def forward(self, users, items):
        """net.py forward: sigmoid(prediction(...)) -> [B, 1]."""
        k = self.k
        u, i = self._feeds(users, items)
        T = self.packed["p"]
        if self.fused:
            return k.ncf_score(self.desc, u, i, T["user"], T["item"], self.flat["p"], self.status).view(-1, 1)
        if u.numel() == 0:
            return torch.empty(0, 1, dtype=torch.float32, device=self.device)
        logit, _ = self._general_fwd(u, i, self._general_bufs(u.numel()))
        zeros = torch.zeros(u.numel(), dtype=torch.int64, device=self.device)
        return k.sigmoid_logloss(logit.view(-1), None, None, zeros, self.ws, want_dz=False)[0]

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, users, items, labels, lr=0.001, mean_over=0):
        """dygraph_model.py:50-80: forward, log loss, backward and Adam on every parameter -> loss [1]."""
        k, T, fl = self.k, self.packed, self.flat
        u, i, y = self._feeds(users, items, labels)
        B = u.numel()
        self.step_count += 1
        if self.fused:
            pred, gu, gi, loss = k.ncf_step(self.desc, u, i, y, T["p"]["user"], T["p"]["item"], fl["p"], fl["g"], mean_over,
                                            self.status, scratch=self._scratch)
        else:
            p, g, mf = self._views("p"), self._views("g"), self.mf
            bufs = self._general_bufs(B)
            logit, acts = self._general_fwd(u, i, bufs)
            pred, dz, loss = k.sigmoid_logloss(logit.view(-1), None, None, y, self.ws, mean_over=mean_over)
            ld = bufs["pred_in"].shape[1]
            off = dict((n, o) for n, o, _ in self.layout)["prediction.weight"]
            # the head reads the MF columns too, which sit behind no ReLU: its backward runs unmasked over the padded width
            k.mlp_head_bwd(bufs["pred_in"], dz, fl["p"][off:off + ld], self.ws, fl["g"][off:off + ld], g["prediction.bias"],
                           relu=False, out=bufs["d_pred_in"])
            d = None
            if self.nfc:
                d = bufs["d_pred_in"][:, mf:mf + self.widths[-1]]
                k.relu_mask_(d, bufs["pred_in"][:, mf:mf + self.widths[-1]])
                for l in range(self.nfc, 0, -1):
                    d = k.linear_backward(acts[l - 1], d, p["layer_%d.weight" % l], self.ws, g["layer_%d.weight" % l],
                                          g["layer_%d.bias" % l], relu_src=acts[l - 1] if l > 1 else None)
            gu, gi = k.ncf_gather_bwd(self.desc, u, i, T["p"]["user"], T["p"]["item"], bufs["d_pred_in"] if mf else None, d)
            pred = pred.view(-1)
        k.adam_dense(fl["p"], fl["m"], fl["v"], fl["g"], self.step_count, lr=lr)
        for side, ids, rows, grad in (("user", u, self.num_users, gu), ("item", i, self.num_items, gi)):
            groups = self._grouped(side, ids, rows, None, self._group_status)
            k.adam_rows_all(groups, grad, 1, T["p"][side], T["m"][side], T["v"][side], self.step_count, lr=lr)
        self._last = dict(u=u, i=i, gu=gu, gi=gi, pred=pred)
        return loss

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}; the tables' dense gradients are rebuilt on
        the host from the step's gradient rows (for inspection, not on the step's path)."""
        L, out = self._last, {n: v.clone() for n, v in self._views("g").items()}
        for side, ids, rows, n in (("User", L["u"], L["gu"], self.num_users), ("Item", L["i"], L["gi"], self.num_items)):
            keep = ((ids >= 0) & (ids < n)).cpu()
            dense = torch.zeros(n, self.cu, dtype=torch.float64).index_add_(0, ids.cpu()[keep], rows.cpu().double()[keep])
            dense = dense.to(torch.float32).to(self.device)
            if self.mf:
                out["MF_Embedding_%s.weight" % side] = dense[:, :self.mf]
            if self.half:
                out["MLP_Embedding_%s.weight" % side] = dense[:, self.mf:]
        return out


def hr_ndcg(pred, label, chunk=100, top=10):
    """evaluate.py:51-64 on the device: the (prediction, label) lines in file order in chunks of `chunk` (the last may be
    shorter); each sorted by prediction, descending and stable; HR = 1 if a label 1 is among the first `top`, NDCG =
    log 2 / log(i + 2) for the first such place i.  -> (user_num, hit ratio, ndcg).  evaluate.py's result[:-1] is not
    reproduced."""
    pred, label = pred.reshape(-1), label.reshape(-1)
    n = pred.numel()
    if n == 0:
        return 0, 0.0, 0.0
    users = -(-n // chunk)
    pad = users * chunk - n
    if pad:
        pred = torch.cat([pred, torch.full((pad,), float("-inf"), dtype=pred.dtype, device=pred.device)])
        label = torch.cat([label, torch.zeros(pad, dtype=label.dtype, device=label.device)])
    order = torch.sort(pred.view(users, chunk), dim=1, descending=True, stable=True).indices[:, :top]
    hit = torch.gather(label.view(users, chunk), 1, order) == 1
    hit = hit.double()                                    # a short chunk's padding: -inf, label 0, never a hit
    first = torch.argmax(hit, dim=1)
    any_hit = hit.sum(1) > 0
    ndcg = torch.where(any_hit, math.log(2.0) / torch.log(first.double() + 2.0), torch.zeros_like(first, dtype=torch.float64))
    return users, float(any_hit.double().mean().item()), float(ndcg.mean().item())


class DygraphModel:
    """ncf/dygraph_model.py — same method names; tensors are torch device tensors.  infer_summary(): evaluate.py's user_num,
    hit ratio and ndcg over the lines seen since the last call."""

    def __init__(self):
        self._pred, self._label = [], []

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return NCFLayer(g("hyper_parameters.num_users"), g("hyper_parameters.num_items"), g("hyper_parameters.mf_dim"),
                        g("hyper_parameters.fc_layers"), g("hyper_parameters.mode"), device=device, kernels=kernels)

    def create_feeds(self, batch_data, device="cuda"):
        """dygraph_model.py:40-47: three int64 [B, 1] tensors; one that already is int64 on the device is passed through."""
        dev = torch.device(device)
        out = []
        for b in batch_data:
            if not torch.is_tensor(b):
                b = torch.as_tensor(np.asarray(b))
            same = b.device.type == dev.type and (dev.index is None or b.device.index == dev.index)
            out.append((b if same and b.dtype == torch.int64 else b.to(dev).to(torch.int64)).reshape(-1, 1))
        return out

    def create_loss(self, prediction, label):
        """dygraph_model.py:50-55 with torch (train_forward takes the loss from the step's kernels)."""
        y, p = label.to(torch.float32).reshape(-1), prediction.reshape(-1)
        return (-y * torch.log(p + 1e-4) - (1 - y) * torch.log(1 - p + 1e-4)).mean()

    def create_optimizer(self, dy_model, config):
        return None                                          # Adam is part of train_step

    def create_metrics(self, device="cuda"):
        return [], []

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        u, i, y = self.create_feeds(batch_data, dy_model.device)
        loss = dy_model.train_step(u, i, y, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        u, i, y = self.create_feeds(batch_data, dy_model.device)
        pred = dy_model.forward(u, i)
        self._pred.append(pred.reshape(-1))
        self._label.append(y.reshape(-1))
        return metrics_list, {"user": u, "prediction": pred, "label": y}

    def infer_summary(self):
        if not self._pred:
            return {"user_num": 0, "hit ratio": 0.0, "ndcg": 0.0}
        n, hr, nd = hr_ndcg(torch.cat(self._pred), torch.cat(self._label))
        self._pred, self._label = [], []
        return {"user_num": n, "hit ratio": hr, "ndcg": nd}
