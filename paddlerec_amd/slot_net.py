"""What the host mirrors of the Criteo slot nets share: `SlotLayerBase` (the bookkeeping of a layer and of its
train_step) and `SlotDygraphModel` (the reference's DygraphModel of a slot model).

A mirror supplies its docstring, its constructor (shapes and initialisers, after `_init_runtime`), `state_dict`, its
forward and the net-specific middle of `train_step`:
    t, cur, side, groups = self._begin_step(B * S)
    ... forward, `ids_group` under `with _OnSide(side, cur):` where the net wants it, loss head, backward ...
    self._update_rows(t, lr, cur, side, (groups, grad, grad_div, P, M, V), ...)
    self._finish_step(t, lr, cur, side)
The two optimizer calls behind them are Adam's; a layer with another rule overrides `_rows_update` / `_dense_update`.
A layer whose trainer may switch the Adam form declares `lazy_mode = False` on its class; one with a fixed form sets it
on the instance (paddlerec_amd.trainer probes the class).  The base defines neither.
"""
import torch

from .net_base import NUM_THRESHOLDS, LayerBase, auc_metrics  # noqa: F401 (re-exported)


class _OnSide:
    """`with _OnSide(side, cur):` — issue on the side stream, ordered after everything issued so far on `cur`.
    side None (a CPU device: orchestration tests with an injected operator backend) makes it a no-op."""

    def __init__(self, side, cur):
        self.side, self.cur = side, cur

    def __enter__(self):
        if self.side is not None:
            self.side.wait_stream(self.cur)
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.side is not None:
            self.ctx.__exit__(*a)


def _round_up(x, m):
    return (x + m - 1) // m * m


_PARTIALS = ("_pp", "_pp1")     # the attributes that keep a step's segment_partials outputs, one per table


class SlotLayerBase(LayerBase):
    """Parameters live in `self.dense` (a _FlatParams) and in the tables `state_dict` names; `self.k` is the operator
    backend."""

    def _init_runtime(self, device, kernels):
        super()._init_runtime(device, kernels)
        self.sparse_state = None
        self._side = None
        self._groups = None

    def grad_dict(self):
        """Dense gradients of the last train_step under the reference's parameter names."""
        return dict(self.dense.g)

    def _linears(self, stem, n):
        """(weights, biases, weight gradients, bias gradients) of the Linears `stem % i`, i < n."""
        p, g = self.dense.p, self.dense.g
        return ([p[stem % i + ".weight"] for i in range(n)], [p[stem % i + ".bias"] for i in range(n)],
                [g[stem % i + ".weight"] for i in range(n)], [g[stem % i + ".bias"] for i in range(n)])

    @staticmethod
    def _concat_ids(sparse_inputs):
        if isinstance(sparse_inputs, (list, tuple)):
            return torch.cat(list(sparse_inputs), dim=1).contiguous()
        return sparse_inputs

    def _buf(self, name, shape, zero=False):
        """The float32 buffer kept in attribute `name`, made anew (empty, or zeros for zero=True) on a new shape."""
        b = getattr(self, name, None)
        if b is None or b.shape != shape:
            b = (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=self.device)
            setattr(self, name, b)
        return b

    # -- the two layouts of the sparse Adam moments ----------------------------------------------
    def _packed_moments(self, rows, D):
        """m and v of a [rows, D] table as views of ONE line-aligned buffer `mv`."""
        Dp = _round_up(D, 4)
        mv = torch.zeros(rows, _round_up(2 * Dp, 32), dtype=torch.float32, device=self.device)
        return dict(mv=mv, m=mv[:, :D], v=mv[:, Dp:Dp + D])

    def _separate_moments(self, rows, width):
        """m, v [rows, width] and the first-order table's m1, v1 [rows, 1] as four tensors."""
        z = lambda w: torch.zeros(rows, w, dtype=torch.float32, device=self.device)
        return dict(m=z(width), v=z(width), m1=z(1), v1=z(1))

    def _ensure_sparse_state(self):
        if self.sparse_state is None:
            self.sparse_state = self._packed_moments(self.rec.shape[0], self.sparse_feature_dim)

    # -- the frame of a train_step -----------------------------------------------------------------
    def _begin_step(self, *key_counts):
        """-> (t, cur, side, groups): the step number, the current and the side stream (None on a CPU device) and the
        IdGroups of key_counts merge keys (a tuple of them for several counts), kept from step to step.  `self._groups`
        is the first of them on every net; setting it to None makes the next step build them anew."""
        self._ensure_sparse_state()
        self.step_count += 1
        cur = side = None
        if self.device.type == "cuda":
            cur = torch.cuda.current_stream()
            if self._side is None:
                self._side = self.k.concurrent_stream(self.device)
            side = self._side
        if self._groups is None or self._group_keys != key_counts:
            made = tuple(self.k.IdGroups(n, self.device) for n in key_counts)
            self._group_keys, self._groups = key_counts, made[0]
            self._step_groups = made[0] if len(made) == 1 else made
        return self.step_count, cur, side, self._step_groups

    # -- the optimizer: Adam unless a layer overrides these two (flen.py: Adagrad) ---------------------
    def _rows_update(self, t, lr, groups, grad, div, P, M, V, **kw):
        """The update of one table's touched rows: Adam, lazy or every row as self.lazy_mode says."""
        (self.k.sparse_adam_rows if self.lazy_mode else self.k.adam_rows_all)(groups, grad, div, P, M, V, t, lr, **kw)

    def _dense_update(self, t, lr, p, m, v, g):
        """The update of the flat dense buffer (or a head of it)."""
        self.k.adam_dense(p, m, v, g, t, lr)

    def _update_rows(self, t, lr, cur, side, *tables, l2=None, **layout):
        """On the side stream: the hot-row partial sums of every table of the step, then their row updates
        (_rows_update: Adam, lazy or every row as self.lazy_mode says, unless the layer overrides it).  tables: (groups,
        grad, grad_div, P, M, V); layout: grad_group / grad_group_stride of a gradient read in place from a wider row."""
        k = self.k
        ukw = layout if l2 is None else dict(layout, l2=l2)
        assert len(tables) <= len(_PARTIALS)
        with _OnSide(side, cur):
            pps = []
            for name, (groups, grad, div, P, _, _) in zip(_PARTIALS, tables):
                pp = k.segment_partials(groups, grad, P.shape[1], out=getattr(self, name, None),
                                        **(layout if div == 1 else dict(layout, grad_div=div)))
                setattr(self, name, pp)
                pps.append(pp)
            for pp, (groups, grad, div, P, M, V) in zip(pps, tables):
                self._rows_update(t, lr, groups, grad, div, P, M, V, partials=pp, **ukw)

    def _finish_step(self, t, lr, cur, side, n_adam=None):
        """The dense update (_dense_update: Adam) on the flat buffer (its first n_adam floats), then the side stream joins
        the current one."""
        d = self.dense
        if n_adam is None:
            self._dense_update(t, lr, d.data, d.m, d.v, d.grad)
        else:
            self._dense_update(t, lr, d.data[:n_adam], d.m[:n_adam], d.v[:n_adam], d.grad[:n_adam])
        if side is not None:
            cur.wait_stream(side)


def slot_feeds(batch_data, config, device):
    """create_feeds of the Criteo slot models (deepfm/dygraph_model.py:41-51, same code in fm / wide_deep / dcn_v2):
    -> (label [B,1] i64, sparse, dense [B,Dn] f32) on `device`.  batch_data is either the reference's 28 arrays
    [label, C1..C26, dense] (sparse = list of 26 [B,1] tensors) or the (label [B,1], ids [B,26], dense [B,13]) device
    tensors of paddlerec_amd.reader (sparse = the [B,26] tensor: no per-slot split and re-concat)."""
    if len(batch_data) == 3 and torch.is_tensor(batch_data[1]) and batch_data[1].dim() == 2 \
            and batch_data[1].shape[1] > 1:
        label, ids, dense = batch_data
        return label.to(device), ids.to(device), dense.to(device)
    dn = config.get("hyper_parameters.dense_input_dim")
    sparse = [torch.as_tensor(b).to(torch.int64).reshape(-1, 1).to(device) for b in batch_data[:-1]]
    dense = torch.as_tensor(batch_data[-1]).to(torch.float32).reshape(-1, dn).to(device)
    return sparse[0], sparse[1:], dense


class SlotDygraphModel:
    """The reference's DygraphModel of a slot model — same method names; tensors are torch device tensors.  A model
    module derives its `DygraphModel` from it and supplies `create_model`."""
    print_loss = False      # train_forward's third value, what the reference's loop prints: {"loss": loss} or None

    def create_feeds(self, batch_data, config, device="cuda"):
        return slot_feeds(batch_data, config, device)

    def create_metrics(self, device="cuda"):
        return auc_metrics(device)

    def train_forward(self, dy_model, metrics_list, batch_data, config):
        label, sparse, dense = self.create_feeds(batch_data, config, dy_model.device)
        lr = config.get("hyper_parameters.optimizer.learning_rate", 0.001)
        loss, _ = dy_model.train_step(sparse, dense, label, lr, metrics_list[0] if metrics_list else None)
        return loss, metrics_list, {"loss": loss} if self.print_loss else None

    def predict(self, dy_model, out):
        """The click probability [B,1] from what the layer's forward returns (a two-class head overrides it)."""
        return out

    def infer_forward(self, dy_model, metrics_list, batch_data, config):
        label, sparse, dense = self.create_feeds(batch_data, config, dy_model.device)
        pred = self.predict(dy_model, dy_model.forward(sparse, dense))
        if metrics_list:
            dy_model.k.auc_histogram(pred.contiguous(), label.contiguous(), metrics_list[0][0], metrics_list[0][1],
                                     NUM_THRESHOLDS)
        return metrics_list, None
