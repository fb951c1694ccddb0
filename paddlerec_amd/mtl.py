"""What the host mirrors of the reference's multitask nets share (models/multitask/mmoe, ple: net.py, dygraph_model.py,
census_reader.py): the layer that runs a PLAN of expert / gate levels on the recengine HIP kernels, and the DygraphModel.

A plan (mmoe.py / ple.py write it from the reference's constructor and forward) is
    params:   [(name, in, out, weight constant, bias constant)] — every nn.Linear of the net in state_dict order, also the
              ones forward() never calls; in place of a constant, a callable that fills the tensor it is given
    aliases:  {second state_dict name: first} of one Linear
    levels:   [{"slots": [(expert name, input)], "gates": [(gate name, input, (first0, count0, first1, count1))]}] — the
              expert outputs of a level in the order the reference concatenates them (a SLOT is one column block of
              expert_size floats; an expert called twice fills two), and per gate the slot ranges it mixes
    n_inputs: inputs of a level (all equal to the features at level 0); a level's outputs, one per gate, feed the next
    tasks:    the first `tasks` outputs of the last level feed tower_t (ReLU) -> tower_out_t -> softmax / clip

How it runs, with the same result as the reference:
  * every expert and gate Linear that reads the same input is a column range of ONE packed image W [in, N] | b [N], columns
    = the image's slots in slot order, then its gates: one rec_gemm_f32 (REC_EPI_BIAS) per image, rec_leaky_relu_fwd with
    slope 0 over the slot columns.  Level 0 reads one input, so it is one image and the GEMM's output IS H | logits.  A
    level >= 1 has one image per input; their outputs are staged and moved into H | logits by the ReLU pass and one strided
    copy per gate (the only glue of such a level; the shipped configs have one level);
  * rec_mtl_mix_fwd turns H | logits into the gate probabilities and the level's outputs, rec_mtl_mix_bwd returns
    dH | dlogits in the same column layout, so the weight gradient of an image is one GEMM (level 0: dW and db; level >= 1:
    rec_gemm_f32_pair, dX too, written straight into the lower level's d(output));
  * an expert that fills two slots exists once per slot in the images; its gradient is the sum over its slots, in slot
    order, written back to every copy, so Adam keeps the copies bit-identical.  state_dict, checkpoints and the optimizer
    state show one tensor, the first slot's;
  * Adam (beta 0.9 / 0.999, epsilon 1e-8, non-lazy) is one rec_adam_dense per image and one over all towers.  A Linear that
    forward() never calls is in no image: it has no gradient and never moves, as under the reference's optimizer;
  * tower_out's backward uses d z0 = -d z1 (train_step has why);
  * the head is rec_mtl_head: predictions, per-sample cost and d(logits) of (1 / B) sum cost in one pass.  The loss value
    (sum over tasks of the batch mean) is only taken, with torch, when something reads it.  A subclass may put another
    head in its place (_head, _loss) and ask for the features' gradient (level0_dx): escm2.py does both.
The train step is eager (no graph capture); the only torch work on its path is allocation."""
import torch

from .net_base import FlatStore, LayerBase, auc_metrics, auc_update

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
STORES = ("p", "g", "m", "v")


class _Image(FlatStore):
    """The packed image of the Linears that read one input: cols = [(name, width)] in column order."""

    def __init__(self, K, cols, device):
        self.K, self.N = int(K), sum(w for _, w in cols)
        super().__init__([("W", (self.K, self.N)), ("b", (self.N,))], device)
        self.cols, c = [], 0
        for name, w in cols:
            self.cols.append((name, c, c + w))
            c += w

    def part(self, s, i):
        """(weight [K, width], bias [width]) views of column block i in store s."""
        _, c0, c1 = self.cols[i]
        return self.view[s]["W"][:, c0:c1], self.view[s]["b"][c0:c1]


class LazyLoss:
    """The step's loss, sum over tasks of the batch mean of cost [B, T]: reduced (torch) when it is read."""

    def __init__(self, cost):
        self.cost, self._v = cost, None

    def value(self):
        if self._v is None:
            self._v = self.cost.mean(0).sum().reshape(1)
        return self._v

    def reshape(self, *shape):
        return self.value().reshape(*shape)

    def item(self):
        return self.value().item()

    __float__ = item


class MtlLayer(LayerBase):
    """forward(x [B, F]) -> [pred_t [B, 2]] per task; train_step(x, label [B, T] float32, lr) -> (loss, pred [B, 2T])."""

    def __init__(self, plan, device="cuda", kernels=None):
        self._init_runtime(device, kernels)
        self.plan, self.tasks = plan, int(plan["tasks"])
        shape = {n: (int(i), int(o)) for n, i, o, _, _ in plan["params"]}
        self.levels, self._copies = [], {}                   # _copies: name -> [(image, column block)] in slot order
        for li, lev in enumerate(plan["levels"]):
            S = shape[lev["slots"][0][0]][1]
            if any(shape[n][1] != S for n, _ in lev["slots"]):
                raise ValueError("the experts of a level must have one size")
            inputs = sorted({i for _, i in lev["slots"]} | {i for _, i, _ in lev["gates"]})
            groups = [inputs] if li == 0 else [[i] for i in inputs]        # level 0: every input is the features
            n_slots, images = len(lev["slots"]), []
            gate_col, c = [], 0
            for n, _, r in lev["gates"]:
                if shape[n][1] != r[1] + r[3]:
                    raise ValueError("gate %s has %d outputs and mixes %d experts" % (n, shape[n][1], r[1] + r[3]))
                gate_col.append(c)
                c += r[1] + r[3]
            for grp in groups:
                sl = [e for e, (_, i) in enumerate(lev["slots"]) if i in grp]
                gt = [g for g, (_, i, _) in enumerate(lev["gates"]) if i in grp]
                if sl != list(range(sl[0], sl[0] + len(sl))):
                    raise ValueError("the slots that read one input must be consecutive")
                names = [lev["slots"][e][0] for e in sl] + [lev["gates"][g][0] for g in gt]
                img = _Image(shape[names[0]][0], [(n, shape[n][1]) for n in names], self.device)
                for pos, n in enumerate(names):
                    if shape[n][0] != img.K:
                        raise ValueError("%s does not have the input width of its image" % n)
                    self._copies.setdefault(n, []).append((img, pos))
                images.append(dict(img=img, input=grp[0], slot0=sl[0], n_sl=len(sl),
                                   gates=[(gate_col[g], shape[lev["gates"][g][0]][1]) for g in gt]))
            self.levels.append(dict(S=S, n_slots=n_slots, n_logit=c, images=images,
                                    mix=self.k.MtlMix(S, n_slots, [r for _, _, r in lev["gates"]])))
        towers = []
        for t in range(self.tasks):
            for n in ("tower_%d" % t, "tower_out_%d" % t):
                towers += [(n + ".weight", shape[n]), (n + ".bias", (shape[n][1],))]
        self.tail = FlatStore(towers, self.device)
        # the reference's separate tensors: the first slot's column range, a tower's entry, or a tensor of its own
        self.params, self._views = {}, {s: {} for s in STORES}
        for n, i, o, wv, bv in plan["params"]:
            if n in self._copies:
                img, pos = self._copies[n][0]
                for s in STORES:
                    self._views[s][n + ".weight"], self._views[s][n + ".bias"] = img.part(s, pos)
            elif n + ".weight" in self.tail.view["p"]:
                for s in STORES:
                    self._views[s][n + ".weight"], self._views[s][n + ".bias"] = (self.tail.view[s][n + ".weight"],
                                                                                 self.tail.view[s][n + ".bias"])
            else:                                             # never called by forward(): no gradient, no optimizer state
                self._views["p"][n + ".weight"] = torch.empty(i, o, dtype=torch.float32, device=self.device)
                self._views["p"][n + ".bias"] = torch.empty(o, dtype=torch.float32, device=self.device)
            for view, init in ((self._views["p"][n + ".weight"], wv), (self._views["p"][n + ".bias"], bv)):
                if callable(init):                            # an initialiser other than a constant: fills the view in place
                    init(view)
                else:
                    view.fill_(float(init))
            self.params[n + ".weight"], self.params[n + ".bias"] = self._views["p"][n + ".weight"], self._views["p"][n + ".bias"]
        self.aliases = {}
        for a, n in plan.get("aliases", {}).items():
            for suffix in (".weight", ".bias"):
                self.aliases[a + suffix] = n + suffix
        self._sync_copies(("p",))
        self._minus_plus = torch.tensor([[-1.0], [1.0]], dtype=torch.float32, device=self.device)
        self.level0_dx = False      # True: train_step also runs level 0's dX GEMM and keeps it as self._last["dX"]

    # ---------------------------------------------------------------- parameters
    def _sync_copies(self, stores=STORES):
        for copies in self._copies.values():
            img0, pos0 = copies[0]
            for img, pos in copies[1:]:
                for s in stores:
                    for dst, src in zip(img.part(s, pos), img0.part(s, pos0)):
                        dst.copy_(src)

    def state_dict(self):
        sd = {}
        for n, _, _, _, _ in self.plan["params"]:
            for suffix in (".weight", ".bias"):
                sd[n + suffix] = self.params[n + suffix]
                for a, t in self.aliases.items():
                    if t == n + suffix:
                        sd[a] = self.params[t]
        return sd

    def parameters(self):
        return list(self.params.values())       # every Linear once: state_dict shows an aliased one twice

    def set_dict(self, sd):
        super().set_dict(sd)                    # an alias key: state_dict holds the same tensor under it
        self._sync_copies(("p",))

    def trainable(self):
        """The state_dict keys the optimizer moves (every Linear forward() calls)."""
        return [k for k in self.params if k in self._views["g"]]

    def _optimizer_views(self):
        """Adam's moments of every trainable parameter, under the parameter's own name."""
        return {"mtl.%s.%s" % (s, k): self._views[s][k] for k in self.trainable() for s in ("m", "v")}

    def set_extra_optimizer_state(self, st):
        super().set_extra_optimizer_state(st)
        self._sync_copies(("m", "v"))

    # ---------------------------------------------------------------- forward
    def _run(self, x, keep=None):
        """-> z [B, 2T], the towers' logits.  keep: a dict that receives what the backward needs."""
        k, ws = self.k, self.ws
        if x.dim() != 2 or x.shape[1] != self.levels[0]["images"][0]["img"].K:
            raise ValueError("expected features [B, %d], got %s" % (self.levels[0]["images"][0]["img"].K, tuple(x.shape)))
        B = x.shape[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        top, tape = x, []
        for li, lev in enumerate(self.levels):
            S, nH = lev["S"], lev["n_slots"] * lev["S"]
            Y = torch.empty(B, nH + lev["n_logit"], **f32)
            H, logits = Y[:, :nH], Y[:, nH:]
            xin = []
            for im in lev["images"]:
                img = im["img"]
                xi = top if li == 0 else top[:, im["input"] * img.K:(im["input"] + 1) * img.K]
                xin.append(xi)
                W, b = img.view["p"]["W"], img.view["p"]["b"]
                if len(lev["images"]) == 1:
                    k.gemm(xi, W, ws, epilogue="bias", bias=b, out=Y)
                    k.leaky_relu_fwd(H, 0.0)
                else:
                    Z = k.gemm(xi, W, ws, epilogue="bias", bias=b)
                    w_sl = im["n_sl"] * S
                    k.leaky_relu_fwd(Z[:, :w_sl], 0.0, out=H[:, im["slot0"] * S:im["slot0"] * S + w_sl])
                    c = w_sl
                    for col, n in im["gates"]:
                        k.bst_add(Z[:, c:c + n], None, out=logits[:, col:col + n])
                        c += n
            prob, mix = k.mtl_mix_fwd(lev["mix"], H, logits)
            tape.append(dict(xin=xin, H=H, prob=prob))
            top = mix
        S = self.levels[-1]["S"]
        p = self.params
        z, acts = torch.empty(B, 2 * self.tasks, **f32), []
        for t in range(self.tasks):
            a = k.gemm(top[:, t * S:(t + 1) * S], p["tower_%d.weight" % t], ws, epilogue="bias_relu", bias=p["tower_%d.bias" % t])
            k.gemm(a, p["tower_out_%d.weight" % t], ws, epilogue="bias", bias=p["tower_out_%d.bias" % t], out=z[:, 2 * t:2 * t + 2])
            acts.append(a)
        if keep is not None:
            keep.update(tape=tape, top=top, acts=acts, B=B)
        return z

    def predict(self, x):
        """-> pred [B, 2T]: the clipped softmax of every task, side by side."""
        z = self._run(x)
        B = z.shape[0]
        pred, _, _ = self.k.mtl_head(z, torch.zeros(B, self.tasks, dtype=torch.float32, device=self.device), 1.0, want_grad=False)
        return pred

    def forward(self, x):
        """net.py forward: -> one clipped softmax [B, 2] per task (column views of predict()'s tensor)."""
        pred = self.predict(x)
        return [pred[:, 2 * t:2 * t + 2] for t in range(self.tasks)]

    __call__ = forward

    # ---------------------------------------------------------------- training
    def _fold_copies(self):
        """An expert in several slots: its gradient is the sum over the slots, in slot order, on every copy."""
        k = self.k
        for copies in self._copies.values():
            if len(copies) == 1:
                continue
            img0, pos0 = copies[0]
            gw0, gb0 = img0.part("g", pos0)
            for img, pos in copies[1:]:
                gw, gb = img.part("g", pos)
                k.bst_add(gw0, gw)
                k.bst_add(gb0.view(1, -1), gb.view(1, -1))
            for img, pos in copies[1:]:
                gw, gb = img.part("g", pos)
                k.bst_add(gw0, None, out=gw)
                k.bst_add(gb0.view(1, -1), None, out=gb.view(1, -1))

    def train_step(self, x, label, lr=1e-3):
        """dygraph_model.py train_forward + backward + Adam.  x [B, F], label [B, T] float32 (columns in task order).
        -> (loss: a LazyLoss, pred [B, 2T])."""
        k, ws, p, g = self.k, self.ws, self.params, self._views["g"]
        self.step_count += 1
        sv = {}
        z = self._run(x, keep=sv)
        B, T = sv["B"], self.tasks
        pred, cost, dz = self._head(z, label, B)
        f32 = dict(dtype=torch.float32, device=self.device)
        S = self.levels[-1]["S"]
        dtop = torch.empty(B, len(self.plan["levels"][-1]["gates"]) * S, **f32)
        if dtop.shape[1] != T * S:
            raise ValueError("the last level must have one gate per task")
        for t in range(T):
            n, no = "tower_%d" % t, "tower_out_%d" % t
            a = sv["acts"][t]
            # d z0 = -d z1 exactly (rec_mtl_head), so d a = d z1 (W[:, 1] - W[:, 0]): with the reference's constant
            # initialisers the two columns are equal and the gradient below tower_out is the exact zero of exact
            # arithmetic — a K = 2 product -x c + x c leaves a rounding residue that Adam would turn into a step of lr
            k.gemm(a, dz[:, 2 * t:2 * t + 2], ws, trans_a=True, out=g[no + ".weight"], b_colsum=g[no + ".bias"])
            wd = k.gemm(p[no + ".weight"], self._minus_plus, ws)
            da = k.gemm(dz[:, 2 * t + 1:2 * t + 2], wd, ws, trans_b=True, epilogue="relu_mask", aux0=a)
            k.linear_backward(sv["top"][:, t * S:(t + 1) * S], da, p[n + ".weight"], ws, g[n + ".weight"], g[n + ".bias"],
                              out=dtop[:, t * S:(t + 1) * S])
        dx0 = None
        for li in reversed(range(len(self.levels))):
            lev, tp = self.levels[li], sv["tape"][li]
            S, nH = lev["S"], lev["n_slots"] * lev["S"]
            G = torch.empty(B, nH + lev["n_logit"], **f32)
            dH, dlogits = G[:, :nH], G[:, nH:]
            k.mtl_mix_bwd(lev["mix"], tp["H"], tp["prob"], dtop, True, dH, dlogits)
            below = torch.empty(B, self.plan["n_inputs"] * lev["images"][0]["img"].K, **f32) if li > 0 else None
            for im, xi in zip(lev["images"], tp["xin"]):
                img = im["img"]
                W, gW, gb = img.view["p"]["W"], img.view["g"]["W"], img.view["g"]["b"]
                if len(lev["images"]) == 1:
                    Gi = G
                else:
                    Gi = torch.empty(B, img.N, **f32)
                    w_sl = im["n_sl"] * S
                    k.bst_add(dH[:, im["slot0"] * S:im["slot0"] * S + w_sl], None, out=Gi[:, :w_sl])
                    c = w_sl
                    for col, n in im["gates"]:
                        k.bst_add(dlogits[:, col:col + n], None, out=Gi[:, c:c + n])
                        c += n
                if li == 0 and self.level0_dx:                # a subclass trains what makes the features
                    dx0 = k.linear_backward(xi, Gi, W, ws, gW, gb)
                elif li == 0:                                 # the features need no gradient: dW and db alone
                    k.gemm(xi, Gi, ws, trans_a=True, out=gW, b_colsum=gb)
                else:
                    k.linear_backward(xi, Gi, W, ws, gW, gb, out=below[:, im["input"] * img.K:(im["input"] + 1) * img.K])
            dtop = below
        self._fold_copies()
        self._last = dict(dz=dz, dX=dx0)
        for lev in self.levels:
            for im in lev["images"]:
                f = im["img"].flat
                k.adam_dense(f["p"], f["m"], f["v"], f["g"], self.step_count, lr, BETA1, BETA2, ADAM_EPS)
        f = self.tail.flat
        k.adam_dense(f["p"], f["m"], f["v"], f["g"], self.step_count, lr, BETA1, BETA2, ADAM_EPS)
        return self._loss(cost), pred

    def _head(self, z, label, B):
        """The head of the step: towers' logits z [B, 2T] and the labels -> (pred, cost, dz = d(loss) / dz).  A subclass with
        another head returns a dz with dz[:, 2t] == -dz[:, 2t + 1] exactly (the towers' backward above relies on it)."""
        T = self.tasks
        if tuple(label.shape) != (B, T) or label.dtype != torch.float32:
            raise ValueError("label must be float32 [B, %d], got %s %s" % (T, label.dtype, tuple(label.shape)))
        return self.k.mtl_head(z, label, 1.0 / B)

    def _loss(self, cost):
        """The loss object train_step returns for the head's per-sample cost."""
        return LazyLoss(cost)

    def last_gradients(self):
        """The gradients of the newest train_step as {state_dict key: tensor}, for the parameters that have one."""
        return {kk: self._views["g"][kk].clone() for kk in self.trainable()}


class MtlDygraphModel:
    """mmoe / ple dygraph_model.py — same method names; tensors are torch device tensors.  Subclasses give create_model."""

    def create_feeds(self, batch_data, config, device="cuda"):
        """dygraph_model.py create_feeds: (features, label_income, label_marital) as the reader yields them (the data's
        columns are marital, income; reader.CensusReader) -> (x [B, feature_size], label [B, 2] = income | marital)."""
        fs = config.get("hyper_parameters.feature_size", None)
        x = torch.as_tensor(batch_data[0]).to(device).to(torch.float32)
        x = x.reshape(-1, int(fs) if fs else x.shape[-1])
        labels = [torch.as_tensor(b).to(device).to(torch.float32).reshape(-1, 1) for b in batch_data[1:3]]
        return x, torch.cat(labels, 1)

    def create_metrics(self, device="cuda"):
        return auc_metrics(device, ("auc_income", "auc_marital"))

    def _auc(self, dy_model, metrics_list, pred, label):
        for t, m in enumerate(metrics_list[:2]):               # column 1 of task t's prediction
            auc_update(dy_model.k, m, pred[:, 2 * t + 1], label[:, t])

    def _check(self, dy_model):
        if dy_model.tasks != 2:
            raise ValueError("the census feeds carry two labels (income, marital); the model has %d tasks" % dy_model.tasks)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        self._check(dy_model)
        x, label = self.create_feeds(batch_data, config, dy_model.device)
        loss, pred = dy_model.train_step(x, label, config.get("hyper_parameters.optimizer.learning_rate", 0.001))
        self._auc(dy_model, metrics_list, pred, label)
        return loss, metrics_list, {"loss": loss}

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        self._check(dy_model)
        x, label = self.create_feeds(batch_data, config, dy_model.device)
        pred = dy_model.predict(x)
        self._auc(dy_model, metrics_list, pred, label)
        return metrics_list, None
