"""The memory contract of the C-ABI (include/recengine.h: the caller owns every buffer, sizes the scratch with the
matching *_bytes query and gets REC_EWORKSPACE when it is too small), held against every workspace-taking entry point
of tests/workspace_cases.py:

  a. baseline      two runs on a plain ops.Workspace are bit-identical (or the case says where the header allows not)
  b. exact size    on helpers.GuardedWorkspace — exactly the queried bytes, the whole allocation pre-filled with 0xFF and
                   again with 0x00, every output pre-filled with NaN — the outputs equal the baseline and no guard byte
                   changed; the wrapper asked for exactly what the query returns
  c. stale reuse   X, then a case of another kernel file, then X again on ONE workspace that is never refilled
  d. refusal       one byte short, and with no bytes at all: REC_EWORKSPACE, guards and outputs untouched
  e. correctness   the baseline against the family's float64 reference at the family's own bar
"""
import pytest
import torch

import workspace_cases as WC
from helpers import GuardedWorkspace

pytestmark = pytest.mark.gpu
DEV = WC.DEV
NAMES = list(WC.CASES)
REFUSED = [n for n in NAMES if WC.CASES[n].refusal is True]      # the others say why not (workspace_cases.py)
_built, _base = {}, {}


def built(name):
    if name not in _built:
        _built[name] = WC.CASES[name].build()
    return _built[name]


def _bits(outs):
    torch.cuda.synchronize()
    return [None if t is None else t.detach().cpu().contiguous().numpy().tobytes() for t in outs]


def _run(name, ws):
    b = built(name)
    return b.run(ws, b.new_outs())


def baseline(name):
    """(bits of the outputs, deterministic?) of the case on a plain ops.Workspace; computed once."""
    if name not in _base:
        from paddlerec_amd import ops
        first = _bits(_run(name, ops.Workspace(DEV)))
        second = _bits(_run(name, ops.Workspace(DEV)))
        _base[name] = (first, first == second)
    return _base[name]


def same_as_baseline(name, outs, what):
    """Bit equality with the baseline; for a case whose header allows an order-dependent result, its float64 bar."""
    bits, det = baseline(name)
    if det:
        got = _bits(outs)
        bad = [i for i, (x, y) in enumerate(zip(got, bits)) if x != y]
        assert not bad, "%s: %s: outputs %s differ from the baseline" % (name, what, bad)
    else:
        torch.cuda.synchronize()
        built(name).check(outs)


@pytest.mark.parametrize("name", NAMES)
def test_a_baseline_reruns_bit_identical(engine_lib, name):
    _, det = baseline(name)
    assert det or WC.CASES[name].nondet, \
        "%s: two runs differ, and neither recengine.h nor the kernel says that they may" % name


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("name", NAMES)
def test_b_exact_size_poisoned(engine_lib, name, fill):
    b = built(name)
    ws = GuardedWorkspace(DEV, fill=fill)
    outs = b.run(ws, b.new_outs())
    torch.cuda.synchronize()
    assert ws.intact(), "%s wrote outside the %d bytes it declared" % (name, ws.gets[-1][0])
    assert [g[0] for g in ws.gets] == [b.nbytes()], "%s: asked for %s bytes, the query says %d" % (
        name, [g[0] for g in ws.gets], b.nbytes())
    assert ws.gets[-1][1].numel() == b.nbytes() and ws.gets[-1][1].data_ptr() % 256 == 0
    same_as_baseline(name, outs, "exact workspace filled with 0x%02X" % fill)


@pytest.mark.parametrize("name", NAMES)
def test_c_stale_reuse(engine_lib, name):
    other = WC.CASES[name].stale_with
    assert other != name
    ws = GuardedWorkspace(DEV, fill=0xFF, refill=False)
    same_as_baseline(name, _run(name, ws), "first run")
    _run(other, ws)
    same_as_baseline(name, _run(name, ws), "after %s on the same workspace" % other)


@pytest.mark.parametrize("name", REFUSED)
def test_d_refusal(engine_lib, name):
    from paddlerec_amd import ops
    b = built(name)
    n = b.nbytes()
    assert n > 0, "%s: pick a shape whose query is not 0" % name
    for short in (1, n):
        ws = GuardedWorkspace(DEV, fill=0xFF, short=short)
        outs = b.new_outs()
        kept = (lambda: b.state(outs)) if b.state else (lambda: outs)
        before = _bits(kept())
        with pytest.raises(ops.RecError, match=r"rc=-3\b"):
            b.run(ws, outs)
        assert _bits(kept()) == before, "%s: a refused call (short by %d) wrote an output" % (name, short)
        assert ws.intact(), "%s: a refused call (short by %d) wrote the workspace" % (name, short)


@pytest.mark.parametrize("name", NAMES)
def test_e_baseline_is_correct(engine_lib, name):
    from paddlerec_amd import ops
    b = built(name)
    outs = b.run(ops.Workspace(DEV), b.new_outs())
    torch.cuda.synchronize()
    b.check(outs)
