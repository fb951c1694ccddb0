"""paddlerec_amd/net_base.py without a GPU: what the mirrors' own tests do not reach — the layout rules of FlatStore and the
input forms, the foreign keys and the grouping cache of LayerBase, on the CPU operator backend."""
import math

import numpy as np
import torch

import cpu_kernels
from paddlerec_amd.net_base import FlatStore, LayerBase

ENTRIES = [("one", (1,)), ("three", (3,)), ("four", (4,)), ("five", (5,)), ("mat", (2, 3))]
OFFSETS = {"one": 0, "three": 4, "four": 8, "five": 12, "mat": 20}        # 4-float padding, declaration order
TOTAL = 28


def test_flat_store_views_start_on_four_floats_and_alias_their_buffer():
    fs = FlatStore(ENTRIES, "cpu")
    assert sorted(fs.flat) == sorted(fs.view) == ["g", "m", "p", "v"]
    for s, buf in fs.flat.items():
        assert buf.dtype == torch.float32 and tuple(buf.shape) == (TOTAL,)
        for i, (name, sh) in enumerate(ENTRIES):
            v, n = fs.view[s][name], math.prod(sh)
            o = v.storage_offset()
            assert tuple(v.shape) == sh and o % 4 == 0 and o == OFFSETS[name]
            v.fill_(i + 1.0)                                                # through the view ...
            assert (buf[o:o + n] == i + 1.0).all()
            buf[o + n - 1] = -7.0                                           # ... and through the buffer
            assert v.reshape(-1)[-1] == -7.0
            v.fill_(i + 1.0)
        gaps = torch.ones(TOTAL, dtype=torch.bool)
        for name, sh in ENTRIES:
            gaps[OFFSETS[name]:OFFSETS[name] + math.prod(sh)] = False
        assert int(gaps.sum()) == 3 + 1 + 3 + 2 and not buf[gaps].any()     # no view reaches into a gap


def test_flat_store_makes_the_stores_it_is_asked_for_and_fills_gaps_too():
    two = FlatStore(ENTRIES, "cpu", stores=("p", "g"))
    assert sorted(two.flat) == sorted(two.view) == ["g", "p"]
    assert two.view["g"]["mat"].storage_offset() == OFFSETS["mat"] and tuple(two.flat["g"].shape) == (TOTAL,)
    fs = FlatStore(ENTRIES, "cpu", fill={"m": 0.1})
    assert (fs.flat["m"] == np.float32(0.1)).all()                          # the whole buffer, so the gaps as well
    assert all((fs.view["m"][name] == np.float32(0.1)).all() for name, _ in ENTRIES)
    for s in ("p", "g", "v"):
        assert not fs.flat[s].any()


class _Tiny(LayerBase):
    def __init__(self):
        self._init_runtime("cpu", cpu_kernels)
        self.w, self.m, self.untouched = torch.zeros(2, 3), torch.zeros(2, 3), torch.full((2,), 5.0)

    def state_dict(self):
        return {"w": self.w}

    def _optimizer_views(self):
        return {"tiny.m.w": self.m}


def test_set_dict_takes_a_tensor_an_ndarray_and_nested_lists():
    want = np.arange(6, dtype=np.float32).reshape(2, 3)
    for value in (torch.as_tensor(want), want, want.tolist(), want.astype(np.float64).reshape(6)):
        m = _Tiny()
        m.set_dict({"w": value})
        assert np.array_equal(m.w.numpy(), want) and m.w.dtype == torch.float32
        m2 = _Tiny()
        m2.set_state_dict({"w": value})
        assert torch.equal(m2.w, m.w)
    assert [p.data_ptr() for p in m.parameters()] == [m.w.data_ptr()]
    m.eval()
    assert m.training is False
    m.train()
    assert m.training is True and m.step_count == 0


def test_optimizer_state_ignores_foreign_keys_and_leaves_unnamed_tensors_alone():
    m = _Tiny()
    m.m.copy_(torch.arange(6.0).reshape(2, 3))
    st = m.extra_optimizer_state()
    assert list(st) == ["tiny.m.w"] and isinstance(st["tiny.m.w"], np.ndarray)
    st["tiny.m.w"][0, 0] = 99.0                                             # a copy, not a view of the layer's tensor
    assert m.m[0, 0] == 0.0
    m2 = _Tiny()
    m2.set_extra_optimizer_state({"tiny.m.w": st["tiny.m.w"].tolist(), "other.m.w": np.ones(7), "dense.m": 3})
    assert np.array_equal(m2.m.numpy(), st["tiny.m.w"])
    assert torch.equal(m2.untouched, torch.full((2,), 5.0)) and not m2.w.any()
    m2.set_extra_optimizer_state({"other.m.w": np.ones(7)})                 # nothing of ours: nothing moves
    assert np.array_equal(m2.m.numpy(), st["tiny.m.w"])
    assert LayerBase().extra_optimizer_state() == {}                        # a layer that names none (plain SGD)


def test_grouped_keeps_the_id_groups_of_a_key_until_the_count_changes():
    m = _Tiny()
    ids = torch.tensor([3, 1, 3, 0, 1, 3])
    a = m._grouped("emb", ids, 5, None, m.status)
    assert a.n == 6 and list(a.uniq) == [0, 1, 3]                           # the backend's grouping has run on it
    b = m._grouped("emb", torch.tensor([4, 4, 4, 4, 4, 2]), 5, None, m.status)
    assert b is a and list(b.uniq) == [2, 4]                                # same count: the same buffers, filled anew
    other = m._grouped("bias", ids, 5, None, m.status)
    assert other is not a and m._id_groups == {"emb": a, "bias": other}     # one per key
    c = m._grouped("emb", ids[:4], 5, 0, m.status)
    assert c is not a and c.n == 4 and m._id_groups["emb"] is c             # a new count replaces it
    assert list(c.uniq) == [1, 3]                                           # padding_idx 0 leaves the grouping
