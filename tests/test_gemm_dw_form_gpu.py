"""The two forms of the bf16 x 3 weight-gradient kernel (csrc/gemm_bf16x3.h, REC_X3_DW_FORM): 0 = gemm_bf16x3_dw_kernel
(four waves, one per SIMD), 1 = gemm_bf16x3_dw_kernel_w8 (eight waves, two per SIMD).  Both run on the same slice plan
and multiply the same operands in the same order, so dW and db must be bit-identical; each form is deterministic and
inside the float64 bound of the exact-f32 GEMM.  The form is read once per process: one worker process per form."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_dw_form_worker.py")

# the bench's dW_2 / dW_1 and dW_0, and the odd shapes of test_gemm_gpu.test_gemm_bf16x3_weight_gradient: a partial last
# slice, kin / nout not a multiple of 16, output blocks of 13 / 12 / 11 / 10 / 9 tiles, the CrossNet widths
SHAPES = [(65536, 400, 400), (65536, 432, 400), (8192 + 64, 400, 400), (16384, 432, 400), (8192, 336, 416),
          (12000 - 32, 448, 340), (8192, 344, 404)]


def _run(form, out):
    env = dict(os.environ, REC_X3_DW_FORM=str(form))
    r = subprocess.run([sys.executable, WORKER, out] + ["%d,%d,%d" % s for s in SHAPES], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, "form %d: %s" % (form, r.stderr[-2000:])
    return np.load(out)


@pytest.mark.gpu
def test_dw_forms_bit_identical_deterministic_and_bounded(tmp_path):
    old, new = _run(0, str(tmp_path / "f0.npz")), _run(1, str(tmp_path / "f1.npz"))
    for rows, kin, nout in SHAPES:
        key = "%d_%d_%d" % (rows, kin, nout)
        assert np.array_equal(old["C_" + key], new["C_" + key]), "dW differs between the forms at " + key
        assert np.array_equal(old["b_" + key], new["b_" + key]), "db differs between the forms at " + key
        rng = np.random.default_rng(rows + kin + nout)
        X = rng.uniform(-1, 1, size=(rows, kin)).astype(np.float32).astype(np.float64)
        G = rng.uniform(-1, 1, size=(rows, nout)).astype(np.float32).astype(np.float64)
        want, bound = X.T @ G, 4e-7 * (np.abs(X).T @ np.abs(G))
        err = np.abs(new["C_" + key].astype(np.float64) - want)
        assert np.all(err <= bound + 1e-30), "%s: max err %.3e, bound %.3e" % (key, err.max(), bound.max())
        cerr = np.abs(new["b_" + key].astype(np.float64) - G.sum(0))
        assert np.all(cerr <= 4e-7 * np.abs(G).sum(0) + 1e-30), key
