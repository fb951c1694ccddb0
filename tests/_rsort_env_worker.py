"""One process of tests/test_grouping_sort_plans_gpu.py: the small-n sweep of the grouping sort (_grouping_cases.SWEEP_N x
SWEEP_ROWS) through rec_ids_group under the process-wide switches of the environment — REC_RSORT_PACK, REC_GROUP_DROP
and REC_RSORT_DIGIT are read once per process, hence a process per setting.

    REC_RSORT_PACK=1 python tests/_rsort_env_worker.py <out.npz>

Writes, per (n, N): the plan rec_ids_group_plan reports in this process (passes, waves, key bytes, packed, drop, the
digit widths), sorted_pos[:n_valid], uniq_rows[:U], seg_offset[:U + 1], n_uniq[:3] and the status word."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from paddlerec_amd import _lib, ops  # noqa: E402

from _grouping_cases import SWEEP_N, SWEEP_ROWS, plan_of, sweep_ids, sweep_key  # noqa: E402


def main():
    out = sys.argv[1]
    res = {}
    ws = ops.Workspace("cuda")
    for N in SWEEP_ROWS:
        for n in SWEEP_N:
            p = plan_of(_lib.lib(), n, N)
            ids = torch.as_tensor(sweep_ids(n, N)).cuda()
            groups, status = ops.ids_group(ids, N, 0, ws)
            spos, uniq, offs = groups.host()
            k = sweep_key(n, N)
            res["plan_" + k] = np.array([p["passes"], p["waves"], p["key_bytes"], p["packed"], p["drop"]] + p["bits"], np.int64)
            res["spos_" + k], res["uniq_" + k], res["offs_" + k] = spos, uniq, offs
            res["nuniq_" + k] = np.array(groups.n_uniq.tolist()[:3] + [int(status.item())], np.int64)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
