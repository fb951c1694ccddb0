"""What every host mirror shares, whatever its net: the padded flat store of its dense parameters (`FlatStore`), the
bookkeeping of a layer (`LayerBase`: the runtime block of its constructor, the parameter protocol, the checkpoint of its
optimizer state and the cached grouping of a table's ids) and the AUC metric pair of a DygraphModel.

A mirror supplies its constructor (shapes and initialisers; `_init_runtime` gives it device, backend, workspaces and status
word), `state_dict`, `_optimizer_views` where its optimizer has state, its forward and its train_step.  The update rule of a
table — segment_partials and the row update, each net with its own arguments — stays in the net; `_grouped` only groups.
slot_net.py builds the Criteo slot nets' `SlotLayerBase` on `LayerBase`."""
import math

import numpy as np
import torch

from . import ops

NUM_THRESHOLDS = 4095  # paddle.metric.Auc default [EXT]


def pad4(n):
    return (n + 3) // 4 * 4


class FlatStore:
    """Named tensors in one flat float32 buffer per store — by default four: values "p", gradients "g", and two optimizer
    moments "m" and "v" — so that a dense optimizer step is one launch.  entries: [(name, shape)]; every tensor starts on a
    4-float boundary (16 bytes: the kernels read float4), in the order given.  `.flat[s]` is the buffer of store s and
    `.view[s][name]` the tensor in it.  fill: {store: constant} for a store that does not start at zero, gaps included."""

    def __init__(self, entries, device, stores=("p", "g", "m", "v"), fill=None):
        total = sum(pad4(math.prod(sh)) for _, sh in entries)
        fill = fill or {}
        self.flat = {s: torch.full((total,), float(fill.get(s, 0.0)), dtype=torch.float32, device=device) for s in stores}
        self.view, o = {s: {} for s in stores}, 0
        for name, sh in entries:
            n = math.prod(sh)
            for s in stores:
                self.view[s][name] = self.flat[s][o:o + n].view(sh)
            o += pad4(n)


class LayerBase:
    """The bookkeeping of a host mirror.  `self.k` is the operator backend; parameters are whatever `state_dict` names."""

    def _init_runtime(self, device, kernels, group_status=False):
        """group_status: the groupings get a status word of their own, `_group_status` (a net that hands the grouping ids
        it has made invalid on purpose, or whose forward has flagged the real ones already)."""
        self.device = torch.device(device)
        self.k = kernels if kernels is not None else ops     # tests may inject a stand-in backend (host logic only)
        self.ws = self.k.Workspace(self.device)
        self.ws_group = self.k.Workspace(self.device)
        self.status = self.k.new_status(self.device)
        if group_status:
            self._group_status = self.k.new_status(self.device)
        self._id_groups = {}            # _grouped's cache: {key: IdGroups}
        self.step_count = 0
        self.training = True
        self._last = None

    # -- parameters under the reference's state_dict keys ---------------------------------------
    def parameters(self):
        return list(self.state_dict().values())

    def set_dict(self, sd):
        """Copies every value of sd (a tensor, an ndarray or nested lists) into the parameter of its key.  A layer that
        knows a key under a second name, or keeps copies of a tensor, translates first and calls this."""
        cur = self.state_dict()
        for key, v in sd.items():
            dst = cur[key]
            dst.copy_(torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v)).to(dst.device).reshape(dst.shape))

    def set_state_dict(self, sd):
        self.set_dict(sd)

    def train(self):
        self.training = True

    def eval(self):
        self.training = False

    # -- the optimizer's own state in a checkpoint (checkpoint.py) --------------------------------
    def _optimizer_views(self):
        """{checkpoint key: tensor} of the optimizer's state (moments, accumulators); none for plain SGD.  The keys are the
        ON-DISK FORMAT of every checkpoint written so far and must not change — also where they look wrong: aitm, esmm,
        escm2, mind and tisas write "mtl.m.<parameter>" / "mtl.v.<parameter>", the prefix of the module (mtl.py) their
        first version was copied from."""
        return {}

    def extra_optimizer_state(self):
        return {key: t.detach().cpu().numpy().copy() for key, t in self._optimizer_views().items()}

    def set_extra_optimizer_state(self, st):
        for key, dst in self._optimizer_views().items():
            if key in st:
                dst.copy_(torch.as_tensor(st[key]).to(dst.device).reshape(dst.shape))

    # -- grouping a table's lookups by row --------------------------------------------------------
    def _grouped(self, key, ids, num_rows, padding_idx, status):
        """-> the IdGroups of `ids` (flat int64) by table row.  The result buffers are kept under `key` from step to step
        and made anew when the number of ids changes."""
        groups = self._id_groups.get(key)
        if groups is None or groups.n != ids.numel():
            groups = self._id_groups[key] = self.k.IdGroups(ids.numel(), self.device)
        self.k.ids_group(ids, num_rows, padding_idx, self.ws_group, None, status, groups)
        return groups


def scatter_rows(table, ids, grad, row_stride):
    """The dense [rows, dim] gradient of `table` from the gradient rows a step kept: lookup i takes dim floats at
    grad's first element + i * row_stride (torch index_add; for last_gradients, not on a step's path)."""
    rows = torch.as_strided(grad, (ids.numel(), table.shape[1]), (row_stride, 1), grad.storage_offset())
    return torch.zeros_like(table).index_add_(0, ids, rows)


def auc_metrics(device, names=("auc",), num_thresholds=NUM_THRESHOLDS):
    """create_metrics: one paddle.metric.Auc("ROC") per name = the two int64 bucket arrays of rec_auc_histogram, on the
    device.  -> (metrics_list, names)."""
    pair = lambda: (torch.zeros(num_thresholds + 1, dtype=torch.int64, device=device),
                    torch.zeros(num_thresholds + 1, dtype=torch.int64, device=device))
    return [pair() for _ in names], list(names)


def auc_update(k, stats, pred, label):
    """Adds a batch to one metric pair: pred [B,1] or [B] float32, label of any integer or float type."""
    k.auc_histogram(pred.contiguous(), label.to(torch.int64).contiguous(), stats[0], stats[1], NUM_THRESHOLDS)
