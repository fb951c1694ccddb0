"""Every *_bytes query of the C-ABI is held to its contract by a case of tests/workspace_cases.py (run on the GPU by
tests/test_workspace_contract_gpu.py), and the guarded workspace those cases run on works as stated.  Runs anywhere."""
import pytest
import torch

import workspace_cases as WC
from helpers import GuardedWorkspace


def test_every_bytes_query_has_a_case():
    from paddlerec_amd import _lib
    queries = sorted(n for n in _lib.SIGNATURES if n.endswith("_bytes"))
    assert len(queries) >= 30
    named = {q for c in WC.CASES.values() for q in c.queries}
    assert named <= set(queries), "cases name queries the ABI does not export: %s" % sorted(named - set(queries))
    assert not set(WC.EXEMPT) & named, "exempt AND covered: %s" % sorted(set(WC.EXEMPT) & named)
    assert all(isinstance(r, str) and r.strip() for r in WC.EXEMPT.values())
    missing = [q for q in queries if q not in named and q not in WC.EXEMPT]
    assert not missing, "no workspace-contract case (tests/workspace_cases.py) for: %s" % missing


def _workspace_taking_exports():
    """Every function of include/recengine.h whose parameters hold `size_t workspace_bytes` (test_abi.py's header parse)."""
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "recengine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\bint\s+(rec_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)
                  if "workspace_bytes" in m.group(2))


def test_every_workspace_taking_entry_point_has_a_case():
    """Per ENTRY POINT, not per query: a sibling that shares a query (rec_gemm_f32_pair, rec_ids_group_payload, a later
    foo_v2) fails here until a case names it, or EXEMPT_ENTRY says in one line why none does."""
    from paddlerec_amd import _lib
    need = _workspace_taking_exports()
    assert len(need) >= 40 and "rec_gemm_f32_pair" in need and "rec_ids_group_payload" in need
    need = sorted(set(need) | set(WC.DECLARED_SIZE_ENTRIES))
    assert set(need) <= set(_lib.SIGNATURES)
    named = {e for c in WC.CASES.values() for e in c.entry}
    assert named <= set(_lib.SIGNATURES), sorted(named - set(_lib.SIGNATURES))
    assert not set(WC.EXEMPT_ENTRY) & named and set(WC.EXEMPT_ENTRY) <= set(need)
    assert all(isinstance(r, str) and r.strip() for r in WC.EXEMPT_ENTRY.values()) and len(WC.EXEMPT_ENTRY) <= 3
    missing = [e for e in need if e not in named and e not in WC.EXEMPT_ENTRY]
    assert not missing, "no workspace-contract case (tests/workspace_cases.py) names: %s" % missing


def test_case_table_is_well_formed():
    for c in WC.CASES.values():
        assert c.queries and c.bar and c.zero and callable(c.build) and c.entry
        assert c.stale_with in WC.CASES and c.stale_with != c.name
        assert c.refusal is True or (isinstance(c.refusal, str) and c.refusal.strip())
    skipped = [c.name for c in WC.CASES.values() if c.refusal is not True]
    assert len(skipped) <= 7, skipped        # buffers without a size argument, and the two layers refused elsewhere


@pytest.mark.parametrize("nbytes", [1, 100, 256, 70000, 65536 + 300])
@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_guarded_workspace_layout(nbytes, fill):
    ws = GuardedWorkspace("cpu", fill=fill)
    v = ws.get(nbytes)
    assert v.numel() == nbytes and v.dtype == torch.uint8 and v.data_ptr() % 256 == 0
    assert bool((v == fill).all()) and ws.intact()
    assert len(ws.gets) == 1 and ws.gets[0][0] == nbytes and ws.gets[0][1] is v
    guard = GuardedWorkspace.guard_bytes(nbytes)
    assert guard % 256 == 0 and guard >= max(64 * 1024, nbytes)
    lo = v.data_ptr() - ws.buf.data_ptr()
    assert lo >= guard and ws.buf.numel() - (lo + nbytes) >= guard      # an overrun of a whole view stays inside
    v.fill_(0x5A)                                                        # writing every byte of the view is allowed
    assert ws.intact()
    ws.buf[lo - 1] = 0x5A                                                # one byte before the view
    assert not ws.intact()
    v = ws.get(nbytes)                                                   # refilled
    assert ws.intact()
    ws.buf[lo + nbytes] = 0x5A                                           # one byte after it
    assert not ws.intact()
    ws.get(nbytes)
    ws.buf[-1] = 0x5A                                                    # the far end of the rear guard
    assert not ws.intact()
    ws.get(nbytes)
    ws.buf[0] = 0x5A
    assert not ws.intact()


@pytest.mark.parametrize("nbytes,short", [(1000, 1), (1000, 999), (1000, 1000), (4, 1)])
def test_guarded_workspace_short(nbytes, short):
    ws = GuardedWorkspace("cpu", short=short)
    v = ws.get(nbytes)
    assert v.numel() == nbytes - short and ws.gets[-1][0] == nbytes
    if v.numel():
        assert v.data_ptr() % 256 == 0
    else:
        assert v.data_ptr() == 0             # what torch reports for a zero-length view: the callee sees (NULL, 0)
    lo = ws._lo
    assert ws.intact()
    ws.buf[lo + nbytes - 1] = 0              # the byte a call that ignores the size would write last: inside, and seen
    assert not ws.intact()
    assert ws.buf.numel() - (lo + nbytes) >= GuardedWorkspace.guard_bytes(nbytes)   # the rear guard starts after the FULL view


def test_guarded_workspace_zero_bytes_and_stale_mode():
    assert GuardedWorkspace("cpu").get(0).numel() == 0
    z = GuardedWorkspace("cpu", zero_view=True)
    v = z.get(0)
    assert v.numel() == 256 and v.data_ptr() % 256 == 0 and z.gets[-1][0] == 0
    st = GuardedWorkspace("cpu", fill=0xFF, refill=False)
    a = st.get(100000)
    a.fill_(7)
    b = st.get(300)                          # a smaller request afterwards starts at the same byte and sees the 7s
    assert b.data_ptr() == a.data_ptr() and bool((b == 7).all())
    c = st.get(200000)                       # growing keeps what was there
    assert int((c == 7).sum()) >= 300
