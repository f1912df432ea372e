"""A float64 NumPy restatement of the Gaussian-process decoder's predictive variance (ratinabox_amd/_gp_decoder.py,
riab_gp_predict_var in csrc/riab_gp.hip) in scikit-learn's formulation, its log marginal likelihood, and an fp32 emulation
of the two kernels' arithmetic that the GPU tolerance rests on.  Test infrastructure only; written from the definitions on
top of tests/gp_decoder_oracle.py (the direct-difference kernel matrix), sharing no code with the package."""
import math

import numpy as np

from tests import gp_decoder_oracle as gp

# max |emulated fp32 var - float64 var| measured by tests/test_gp_variance_cpu.py::test_fp32_budget over the three golden
# cases and the N = 512 case (alpha = 0.01), rounded up; the GPU tests allow MARGIN times it, because the kernels' summation
# order (one fmaf chain per row, then one per position) differs from NumPy's pairwise and blocked sums.
FP32_VAR_ERROR = 1.6e-6
MARGIN = 8.0
GPU_VAR_TOLERANCE = MARGIN * FP32_VAR_ERROR


def forward_substitute(L, B):
    """L^-1 B for a lower-triangular L (N, N) and B (N, S), row by row"""
    V = np.zeros_like(B, dtype=np.float64)
    for i in range(L.shape[0]):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i]
    return V


def factor(X, ell, alpha):
    return np.linalg.cholesky(gp.gram(X, ell, alpha))


def variance(Xq, X, ell, alpha):
    """1 - |L^-1 k*|^2 per query, float64, NOT clamped (S,)"""
    V = forward_substitute(factor(X, ell, alpha), gp.kernel(Xq, X, ell).T)
    return 1.0 - (V * V).sum(axis=0)


def std(Xq, X, ell, alpha):
    return np.sqrt(np.maximum(variance(Xq, X, ell, alpha), 0.0))


def log_marginal_likelihood(X, y, ell, alpha):
    """sum over the target columns of -1/2 y^T alpha_ - sum log L_ii - N/2 log 2 pi"""
    L = factor(X, ell, alpha)
    y = np.asarray(y, dtype=np.float64)
    a = np.linalg.solve(L.T, forward_substitute(L, y))
    N, D = y.shape
    return -0.5 * float((y * a).sum()) - D * float(np.log(np.diag(L)).sum()) - 0.5 * D * N * math.log(2.0 * math.pi)


def linv_t_table(X, ell, alpha):
    """what riab_gp_predict_var takes: float32 (Np, Np), table[j][i] = (L^-1)[i][j], zero above the diagonal and in the padding"""
    N = X.shape[0]
    Np = (N + 31) // 32 * 32
    linv = np.tril(forward_substitute(factor(X, ell, alpha), np.eye(N)))
    table = np.zeros((Np, Np), dtype=np.float32)
    table[:N, :N] = linv.T
    return table


def kstar_fp32(Xq, X, ell):
    """k* the way gp_decoder_oracle.emulate_fp32 builds it: float32 operands, the GEMM-form distance clamped at 0, a float32
    exponential -> (S, N) float32"""
    Xq32, X32 = np.asarray(Xq, dtype=np.float32), np.asarray(X, dtype=np.float32)
    sq_t = (X32.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    sq_q = (Xq32 * Xq32).sum(axis=1, dtype=np.float32)
    d2 = (sq_q[:, None] + sq_t[None, :]) - np.float32(2.0) * (Xq32 @ X32.T)
    return np.exp(-(np.maximum(d2, np.float32(0.0)) * np.float32(1.0 / (2.0 * ell * ell)))).astype(np.float32)


def emulate_fp32(Xq, X, ell, alpha):
    """The kernels' arithmetic in float32: k* as above, L^-1 rounded to float32, float32 products and sums, 1 - sum of
    squares -> (S,) float32, not clamped"""
    N = X.shape[0]
    k = kstar_fp32(Xq, X, ell)
    v = k @ linv_t_table(X, ell, alpha)[:N, :N]               # (S, N) float32: v[s][i] = sum_j k[s][j] (L^-1)[i][j]
    assert v.dtype == np.float32
    return np.float32(1.0) - (v * v).sum(axis=1, dtype=np.float32)
