"""Host-side mirror of the reference's MatchPyramid plugin (models/match/match-pyramid/net.py MatchPyramidLayer;
dygraph_model.py) on the recengine HIP kernels: text matching as image recognition over the word-by-word interaction of two
sentences.

The reference forms cross [B, 1, Ll, Lr] = emb(left) emb(right)^T, convolves it ("SAME") to K channels, rectifies and
max-pools ("VALID") it — [B, K, Ll, Lr] twice in memory — and feeds the K * PH * PW = 240 pooled numbers to two Linears.  A
step here is:

  * rec_mpyr_fwd: lookups, interaction, convolution, ReLU and pool in one launch, one block per (sample, row of pool windows)
    with that band of the image in LDS -> pooled [B, 240] and the winners' cells (argmax);
  * rec_gemm_f32 with its BIAS_RELU / BIAS epilogue for fc1 / fc2;
  * rec_mpyr_hinge: the pairwise hinge over the rows [0:64] against [64:128] and d(prediction);
  * rec_gemm_f32_pair per Linear on the way back;
  * rec_mpyr_bwd: the image recomputed band by band for the ReLU gate and d(conv), then d(cross) gathered from the winners and
    multiplied back into dL / dR, every row written;
  * rec_ids_group over the left and right ids together and rec_adam_rows_all on the table, rec_adam_dense on the rest.
Paddle's dygraph Adam is not lazy: every row of the table moves every step."""
import math
import os

import numpy as np
import torch

from .net_base import FlatStore, LayerBase, scatter_rows

PADDING_IDX = 193367                                           # net.py:47,55: a constant, whatever vocab_size is
FC1_IN = 240                                                   # net.py:67
LOSS_PAIRS = 64                                                # dygraph_model.py:56-62
QUIRKS = ("padding_idx is the constant 193367 whatever vocab_size is, so vocab_size <= 193367 fails in the reference and is "
          "refused here; fc1 has in_features 240 hard-coded, so any shape with kernel_num * PH * PW != 240 is refused; "
          "pool_type other than 'max' and hidden_act other than 'relu' leave a name unbound in the reference's forward and are "
          "refused; conv_act other than 'relu' means no activation; the loss slices the rows [0:64] and [64:128] with "
          "full([64, 1]) constants, so training needs a batch of at least 128, rows from 128 on run forward and get a zero "
          "gradient; the hinge is maximum(0, x), whose gradient flows at x == 0; `channels` is read from the YAML by nobody; "
          "create_metrics is empty")


def _pair(x, name):
    x = [int(v) for v in (x if isinstance(x, (list, tuple)) else [x, x])]
    if len(x) != 2:
        raise ValueError("MatchPyramid: %s must be one or two integers" % name)
    return x


class MatchPyramidLayer(LayerBase):
    """net.py:23-92.  forward(inputs) -> prediction [B, 1];  train_step(inputs, lr) -> loss [1].
    inputs: [sentence_left int64 [B, Ll], sentence_right int64 [B, Lr]]."""

    def __init__(self, emb_path, vocab_size, emb_size, kernel_num, conv_filter, conv_act, hidden_size, out_size, pool_size,
                 pool_stride, pool_padding, pool_type, hidden_act, sentence_left_size, sentence_right_size, device="cuda",
                 kernels=None):
        self._init_runtime(device, kernels, group_status=True)
        k = self.k
        if pool_type != "max":
            raise ValueError("MatchPyramid: pool_type %r: the reference's forward leaves `pool` unbound (net.py:79-85)" % (pool_type,))
        if hidden_act != "relu":
            raise ValueError("MatchPyramid: hidden_act %r: the reference's forward leaves `relu_hid` unbound (net.py:89-91)"
                             % (hidden_act,))
        if str(pool_padding).upper() != "VALID":
            raise ValueError("MatchPyramid: pool_padding %r: the kernels pool VALID, as the shipped YAML does" % (pool_padding,))
        if int(out_size) != 1:
            raise ValueError("MatchPyramid: out_size %r: the loss reads column 0 alone; the mirror builds out_size 1" % (out_size,))
        self.vocab_size, self.emb_size, self.hidden = int(vocab_size), int(emb_size), int(hidden_size)
        if self.vocab_size <= PADDING_IDX:
            raise ValueError("MatchPyramid: vocab_size %d does not hold padding_idx %d (the reference fails there)"
                             % (self.vocab_size, PADDING_IDX))
        kh, kw = _pair(conv_filter, "conv_filter")
        ph, pw = _pair(pool_size, "pool_size")
        sh, sw = _pair(pool_stride, "pool_stride")
        self.shape = k.MpyrShape(int(sentence_left_size), int(sentence_right_size), self.emb_size, int(kernel_num), kh, kw, ph, pw,
                                 sh, sw, int(conv_act == "relu"))
        why = k.mpyr_shape_error(self.shape)
        if why is not None or self.hidden < 1:
            raise ValueError("MatchPyramid: %s" % (why or "hidden_size must be positive"))
        self.PH, self.PW = k.mpyr_pooled_shape(self.shape)
        self.features = self.shape.channels * self.PH * self.PW
        if self.features != FC1_IN:
            raise ValueError("MatchPyramid: kernel_num * PH * PW = %d * %d * %d = %d, and fc1 has in_features %d hard-coded "
                             "(net.py:67)" % (self.shape.channels, self.PH, self.PW, self.features, FC1_IN))
        self.store = FlatStore([("conv.weight", (self.shape.channels, 1, kh, kw)), ("conv.bias", (self.shape.channels,)),
                                ("fc1.weight", (FC1_IN, self.hidden)), ("fc1.bias", (self.hidden,)),
                                ("fc2.weight", (self.hidden, 1)), ("fc2.bias", (1,))], self.device)
        self.flat = self.store.flat
        f32 = dict(dtype=torch.float32, device=self.device)
        self.emb_store = {s: torch.zeros(self.vocab_size, self.emb_size, **f32) for s in ("p", "m", "v")}
        self._bufs = {}
        self._init(emb_path)

    # ---------------------------------------------------------------- parameters
    def _init(self, emb_path):
        """net.py:42-69: the table from emb_path when that file exists, XavierNormal otherwise (padding row zeroed by
        Embedding); Conv2D Normal(0, sqrt(2 / (in_channels kh kw))), Linear XavierUniform, biases zero: Paddle's defaults."""
        p, T = self.store.view["p"], self.emb_store["p"]
        if emb_path and os.path.isfile(emb_path):
            T.copy_(torch.as_tensor(np.load(emb_path).astype(np.float32)).reshape(T.shape))
        else:
            T.copy_(torch.randn(T.shape, device=self.device) * math.sqrt(2.0 / (self.vocab_size + self.emb_size)))
        T[PADDING_IDX].zero_()
        s = self.shape
        p["conv.weight"].copy_(torch.randn(p["conv.weight"].shape, device=self.device) * math.sqrt(2.0 / (s.filter_h * s.filter_w)))
        for name, fi, fo in (("fc1", FC1_IN, self.hidden), ("fc2", self.hidden, 1)):
            lim = math.sqrt(6.0 / (fi + fo))
            p[name + ".weight"].copy_((torch.rand(fi, fo, device=self.device) * 2 - 1) * lim)

    def state_dict(self):
        sd = {"emb.weight": self.emb_store["p"]}
        sd.update(self.store.view["p"])
        return sd

    def moments(self):
        return tuple(dict([("emb.weight", self.emb_store[s])] + list(self.store.view[s].items())) for s in ("m", "v"))

    def load_state_dict(self, sd):
        self.set_dict(sd)

    def _optimizer_views(self):
        m, v = self.moments()
        return {"match_pyramid.%s.%s" % (s, k): t for s, d in (("m", m), ("v", v)) for k, t in d.items()}

    # ---------------------------------------------------------------- feeds
    def _inputs(self, inputs):
        if len(inputs) < 2:
            raise ValueError("MatchPyramid: inputs must be [sentence_left, sentence_right]")
        left = inputs[0].reshape(-1, self.shape.left_len).to(torch.int64).contiguous()
        right = inputs[1].reshape(-1, self.shape.right_len).to(torch.int64).contiguous()
        if left.shape[0] != right.shape[0] or left.shape[0] < 1:
            raise ValueError("MatchPyramid: the two sentences must hold one batch of at least one sample")
        return left, right

    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            if len(self._bufs) >= 4:
                self._bufs.pop(next(iter(self._bufs)))
            f32, s = dict(dtype=torch.float32, device=self.device), self.shape
            b = self._bufs[B] = dict(pooled=torch.empty(B, self.features, **f32),
                                     argmax=torch.empty(B, self.features, dtype=torch.int32, device=self.device),
                                     hinge=(torch.empty(1, **f32), torch.empty(B, **f32)),
                                     rows=torch.empty(B * (s.left_len + s.right_len), s.emb_dim, **f32), scratch={})
        return b

    # ---------------------------------------------------------------- forward
    def _towers(self, left, right, bufs):
        k, p = self.k, self.store.view["p"]
        pooled, argmax = k.mpyr_fwd(self.shape, left, right, self.emb_store["p"], p["conv.weight"], p["conv.bias"], PADDING_IDX,
                                    self.status, out=(bufs["pooled"], bufs["argmax"]))
        hid = k.gemm(pooled, p["fc1.weight"], self.ws, epilogue="bias_relu", bias=p["fc1.bias"])
        pred = k.gemm(hid, p["fc2.weight"], self.ws, epilogue="bias", bias=p["fc2.bias"])
        return pooled, argmax, hid, pred

    def forward(self, inputs):
        """net.py:71-92 -> prediction [B, 1]."""
        left, right = self._inputs(inputs)
        return self._towers(left, right, self._buffers(left.shape[0]))[3]

    __call__ = forward

    # ---------------------------------------------------------------- training
    def train_step(self, inputs, lr=0.001):
        """dygraph_model.py:55-69,86-98 and the trainer's backward / Adam step -> loss [1]."""
        k, fl, s = self.k, self.flat, self.shape
        p, g, T = self.store.view["p"], self.store.view["g"], self.emb_store
        left, right = self._inputs(inputs)
        B = left.shape[0]
        if B < 2 * LOSS_PAIRS:
            raise ValueError("MatchPyramid: the loss slices the rows [0:64] and [64:128] (dygraph_model.py:56-59): a batch of %d "
                             "is too small" % B)
        self.step_count += 1
        bufs = self._buffers(B)
        pooled, argmax, hid, pred = self._towers(left, right, bufs)
        loss, d_pred = k.mpyr_hinge(pred, LOSS_PAIRS, out=bufs["hinge"])
        d_hid = k.linear_backward(hid, d_pred.view(B, 1), p["fc2.weight"], self.ws, g["fc2.weight"], g["fc2.bias"], relu_src=hid)
        d_pooled = k.linear_backward(pooled, d_hid, p["fc1.weight"], self.ws, g["fc1.weight"], g["fc1.bias"])
        rows = bufs["rows"]
        k.mpyr_bwd(s, left, right, T["p"], p["conv.weight"], p["conv.bias"], d_pooled, argmax, rows[:B * s.left_len],
                   rows[B * s.left_len:], g["conv.weight"], g["conv.bias"], PADDING_IDX, scratch=bufs["scratch"])
        ids = torch.cat((left.reshape(-1), right.reshape(-1)))
        groups = self._grouped("emb", ids, self.vocab_size, PADDING_IDX, self._group_status)
        k.adam_rows_all(groups, rows, 1, T["p"], T["m"], T["v"], self.step_count, lr=lr)
        k.adam_dense(fl["p"], fl["m"], fl["v"], fl["g"], self.step_count, lr=lr)
        self._last = dict(ids=ids, rows=rows, pred=pred, pooled=pooled, argmax=argmax, B=B)
        return loss

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}; the table's dense gradient is rebuilt from the
        step's gradient rows (for inspection, not on the step's path)."""
        L = self._last
        out = {n: v.clone() for n, v in self.store.view["g"].items()}
        out["emb.weight"] = scatter_rows(self.emb_store["p"], L["ids"], L["rows"], L["rows"].stride(0))
        return out

    def last_outputs(self):
        """prediction [B, 1], pooled [B, 240] and argmax of the newest train_step."""
        L = self._last
        return L["pred"], L["pooled"], L["argmax"]


class DygraphModel:
    """match-pyramid/dygraph_model.py — same method names; tensors are torch device tensors."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        h = "hyper_parameters."
        return MatchPyramidLayer(g(h + "emb_path"), g(h + "vocab_size"), g(h + "emb_size"), g(h + "kernel_num"),
                                 g(h + "conv_filter"), g(h + "conv_act"), g(h + "hidden_size"), g(h + "out_size"),
                                 g(h + "pool_size"), g(h + "pool_stride"), g(h + "pool_padding"), g(h + "pool_type"),
                                 g(h + "hidden_act"), g(h + "sentence_left_size"), g(h + "sentence_right_size"), device=device,
                                 kernels=kernels)

    def create_feeds(self, batch_data, sentence_left_size, sentence_right_size, device="cuda"):
        """dygraph_model.py:46-52: int64 [B, Ll] and [B, Lr]."""
        out = []
        for x, n in ((batch_data[0], sentence_left_size), (batch_data[1], sentence_right_size)):
            if not torch.is_tensor(x):
                x = torch.as_tensor(np.asarray(x))
            out.append(x.to(device).to(torch.int64).reshape(-1, n))
        return out

    def create_loss(self, prediction):
        """dygraph_model.py:55-69 with torch (train_forward takes the loss from the step's kernels)."""
        pos, neg = prediction[0:LOSS_PAIRS, 0:1], prediction[LOSS_PAIRS:2 * LOSS_PAIRS, 0:1]
        return torch.clamp(1.0 - pos + neg, min=0.0).mean()

    def create_optimizer(self, dy_model, config):
        return None                                          # Adam is part of train_step

    def create_metrics(self, device="cuda"):
        return [], []

    def _inputs(self, dy_model, batch_data, config):
        return self.create_feeds(batch_data, config.get("hyper_parameters.sentence_left_size"),
                                 config.get("hyper_parameters.sentence_right_size"), dy_model.device)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        loss = dy_model.train_step(self._inputs(dy_model, batch_data, config),
                                   config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        prediction = dy_model.forward(self._inputs(dy_model, batch_data, config))
        return metrics_list, {"prediction": prediction}
