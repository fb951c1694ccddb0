"""One process of tests/test_gemm_dw_form_gpu.py: the bf16 x 3 weight gradient (dW = X^T G, db = colsum G) through the
engine on the kernel form that REC_X3_DW_FORM selects (read once per process, hence a process per form).

    REC_X3_DW_FORM=<0|1> python tests/_dw_form_worker.py <out.npz> rows,kin,nout [rows,kin,nout ...]

Every shape runs twice; the second result must equal the first (the worker exits non-zero otherwise)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from paddlerec_amd import ops  # noqa: E402


def main():
    out, shapes = sys.argv[1], [tuple(int(v) for v in s.split(",")) for s in sys.argv[2:]]
    os.environ["REC_GEMM_BF16X3"] = "1"
    res = {}
    for rows, kin, nout in shapes:
        rng = np.random.default_rng(rows + kin + nout)
        X = torch.as_tensor(rng.uniform(-1, 1, size=(rows, kin)).astype(np.float32)).cuda()
        G = torch.as_tensor(rng.uniform(-1, 1, size=(rows, nout)).astype(np.float32)).cuda()
        ws = ops.Workspace("cuda")
        got = []
        for _ in range(2):
            C_, b_ = torch.zeros(kin, nout, device="cuda"), torch.zeros(nout, device="cuda")
            ops.gemm(X, G, ws, trans_a=True, out=C_, b_colsum=b_)
            got.append((C_.cpu().numpy(), b_.cpu().numpy()))
        if not (np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])):
            print("not deterministic at %d x %d x %d" % (rows, kin, nout), file=sys.stderr)
            sys.exit(3)
        res["C_%d_%d_%d" % (rows, kin, nout)], res["b_%d_%d_%d" % (rows, kin, nout)] = got[0]
    np.savez(out, **res)


if __name__ == "__main__":
    main()
