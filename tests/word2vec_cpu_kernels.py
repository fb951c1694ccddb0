"""Stand-in for paddlerec_amd.ops on CPU tensors for the host logic of paddlerec_amd/word2vec.py — TEST INFRASTRUCTURE ONLY.

The id grouping that drops a row outside [0, num_rows) (tests/aitm_cpu_kernels.py), the segment partials and the row SGD
(tests/cpu_kernels.py), and the three new ops: rec_w2v_sgns_fwd_bwd, rec_w2v_target_update and rec_w2v_analogy_topk evaluate
the formulas of tests/word2vec_ref.py in float32, writing through the same views the device kernels write through.  The
product never imports this module."""
import numpy as np
import torch

import word2vec_ref as R
from aitm_cpu_kernels import ids_group  # noqa: F401
from cpu_kernels import IdGroups as _IdGroups
from cpu_kernels import Workspace, new_status, segment_partials, sparse_sgd_rows  # noqa: F401
from mtl_cpu_kernels import _n, _t

F32 = np.float32


class IdGroups(_IdGroups):
    def host(self):
        return self.spos, self.uniq, self.offs


def raise_on_status(status, what="lookup"):
    from paddlerec_amd._lib import RecError
    if int(status.item()) & 1:
        raise RecError("%s: index out of range [0, num_rows)" % what)


def w2v_sgns_fwd_bwd(in_ids, target_ids, emb, emb_w, emb_b, grad_scale=1.0, status=None, d_in=None):
    i, t = in_ids.numpy(), target_ids.numpy()
    V = emb.shape[0]
    if status is None:
        status = new_status("cpu")
    if ((i < 0) | (i >= V)).any() or ((t < 0) | (t >= V)).any():
        status |= 1
    c = R.sgns(_n(emb), _n(emb_w), _n(emb_b), i, t, grad_scale, F32)
    d = _t(c["d_in"])
    return (_t(c["true_logits"]), _t(c["neg_logits"]), _t(c["g"]), d if d_in is None else d_in.copy_(d), _t(c["loss"]), status)


def w2v_target_update(groups, g, in_ids, emb, emb_w, emb_b, lr, d_w_rows=None, d_b_rows=None):
    assert emb.data_ptr() != emb_w.data_ptr()
    tw = g.shape[1]
    i = in_ids.numpy()
    V = emb.shape[0]
    e, w, b, gf = _n(emb), _n(emb_w), _n(emb_b), _n(g).reshape(-1)
    for u, r in enumerate(groups.uniq):
        dw, db = np.zeros(e.shape[1], F32), F32(0)
        for kk in range(groups.offs[u], groups.offs[u + 1]):          # ascending positions
            pos = int(groups.spos[kk])
            if 0 <= i[pos // tw] < V:
                dw = dw + gf[pos] * e[i[pos // tw]]
                db = F32(db + gf[pos])
        w[r] = w[r] - F32(lr) * dw
        b[r, 0] = b[r, 0] - F32(lr) * db
        if d_w_rows is not None:
            d_w_rows[u] = _t(dw)
        if d_b_rows is not None:
            d_b_rows[u] = float(db)


def w2v_analogy_topk(a, b, c, W, k=4, status=None, cand=None):
    v, i = R.topk(R.scores(_n(W), a.numpy(), b.numpy(), c.numpy(), F32), k)
    return _t(v), torch.from_numpy(np.ascontiguousarray(i))
