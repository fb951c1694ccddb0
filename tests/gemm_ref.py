"""One float64 reference, and one error bound per epilogue, for every rec_gemm_f32 test.

The GEMM is an exact-f32 accumulate (or f32-grade: bf16 x 3), so against float64 the error of the product is f32
round-off of a K-term dot product: at most 4e-7 * sum_k |a_ik||b_kj| (tests/test_gemm_gpu.py).  An epilogue adds a few
f32 roundings of its own operations (1.2e-7 = 2^-23 per rounding, of the magnitudes that are rounded) and scales the
product's error by its own factor; expf / tanhf of the device are a few ulp of a result <= 1: + 1e-6.
"""
import numpy as np

EPILOGUES = ("none", "bias", "bias_relu", "relu_mask", "cross", "bias_sigmoid", "bias_tanh", "add", "moe", "dsigmoid",
             "dtanh")
# the operands an epilogue reads (bias of "bias_tanh" / "add" and aux0 of "add" are optional)
NEEDS_BIAS = ("bias", "bias_relu", "cross", "bias_sigmoid", "bias_tanh", "add", "moe")
NEEDS_AUX0 = ("relu_mask", "cross", "add", "moe", "dtanh", "dsigmoid")
NEEDS_AUX1 = ("cross", "add", "moe")


def product(A, B):
    """(A @ B, |A| @ |B|) in float64 for A [M,K], B [K,N]: compute once per shape, pass as prod= below."""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    return A64 @ B64, np.abs(A64) @ np.abs(B64)


def epi_reference(epi, A, B, bias, X0, X1, rs, prod=None):
    """-> (want64, bound): the float64 value of epi(A @ B) and the largest |C - want64| an f32 kernel may show.
    A [M,K], B [K,N] as the logical operands; bias [N], X0 = aux0, X1 = aux1 [M,N], rs = row_scale [M]; an operand the
    epilogue does not read (or an optional one that is absent) is None."""
    acc, mag = prod if prod is not None else product(A, B)
    bound = 4e-7 * mag
    if epi.startswith("bias") and bias is not None:
        acc = acc + bias
        bound = bound + 1.2e-7 * np.abs(acc)                 # the f32 add of the bias
    if epi == "bias_relu":
        acc = np.maximum(acc, 0)
    if epi == "relu_mask":
        acc = np.where(X0 > 0, acc, 0)
    if epi == "cross":                                       # dcn_v2/net.py:225: X_l + X_0 * (X_l W + b)
        acc = X1 + X0.astype(np.float64) * (acc + bias)
        bound = bound * np.abs(X0) + 2.4e-7 * (np.abs(acc) + np.abs(X1)) + 1e-7
    if epi == "add":
        z0 = X0 if X0 is not None else 0.0
        acc = acc + (bias if bias is not None else 0.0) + X1.astype(np.float64) + z0
        bound = bound + 3.6e-7 * (np.abs(acc) + np.abs(X1) + np.abs(z0)) + 1e-7
    if epi == "moe":                                         # x_l + x_0 * gate_e * (U_e v + b)
        acc = X1 + X0.astype(np.float64) * rs[:, None] * (acc + bias)
        bound = bound * np.abs(X0 * rs[:, None]) + 3.6e-7 * (np.abs(acc) + np.abs(X1)) + 1e-7
    if epi in ("bias_tanh", "bias_sigmoid"):                 # expf / tanhf of the device: a few ulp of the result
        acc = np.tanh(acc) if epi == "bias_tanh" else 1.0 / (1.0 + np.exp(-acc))
        bound = bound + 1e-6
    if epi == "dtanh":
        acc = acc * (1.0 - X0.astype(np.float64) ** 2)
        bound = bound * np.abs(1.0 - X0.astype(np.float64) ** 2) + 2.4e-7 * np.abs(acc) + 1e-7
    if epi == "dsigmoid":
        acc = acc * X0.astype(np.float64) * (1.0 - X0)
        bound = bound * np.abs(X0 * (1.0 - X0)) + 3.6e-7 * np.abs(acc) + 1e-7
    return acc, bound


def cross_out2_reference(A, B, bias, prod=None):
    """-> (want64, bound) of the second output of "cross": u = A @ B + bias (saved for the backward)."""
    acc, mag = prod if prod is not None else product(A, B)
    u = acc + bias
    return u, 4e-7 * mag + 1.2e-7 * np.abs(u)


def check(C, want, bound, what=""):
    err = np.abs(C.astype(np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    bad = ~(err <= bound + 1e-30)                            # (a NaN fails)
    if bad.any():
        at = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(bad, np.nan_to_num(err, nan=np.inf), -1.0)), err.shape))
        raise AssertionError("%s: %d of %d outside the bound, worst at %s: got %r want %r, bound %.3e" % (
            what, int(bad.sum()), err.size, at, float(C[at]), float(want[at]), float(bound[at])))
