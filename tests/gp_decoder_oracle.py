"""A float64 NumPy restatement of the Gaussian-process decoder (ratinabox_amd/_gp_decoder.py, csrc/riab_gp.hip): the rule
that chooses the training samples, the RBF kernel matrix BY DIRECT DIFFERENCES (not the GEMM form the product uses), the
Cholesky solve, the predictive mean, and an fp32 emulation of the kernel's arithmetic that the GPU allowance rests on.
Test infrastructure only; written from the definitions, sharing no code with the package."""
import math

import numpy as np

PHI = (math.sqrt(5.0) - 1.0) / 2.0


def select_samples(R, B, max_samples):
    """(row indices, agents), time-major.  All R * B candidates when they fit; otherwise sample i of max_samples takes row
    floor(i R / max_samples), agent floor(B frac((i + 1) phi)); duplicates removed."""
    if R * B <= max_samples:
        return (np.repeat(np.arange(R, dtype=np.int64), B), np.tile(np.arange(B, dtype=np.int64), R))
    chosen = set()
    for i in range(max_samples):
        x = (i + 1) * PHI
        chosen.add(((i * R) // max_samples, int(math.floor(B * (x - math.floor(x))))))
    chosen = sorted(chosen)
    return (np.array([c[0] for c in chosen], dtype=np.int64), np.array([c[1] for c in chosen], dtype=np.int64))


def kernel(A, B, ell):
    """exp(-|a - b|^2 / (2 ell^2)), (S, n) x (N, n) -> (S, N), float64, by direct differences"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d2 = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        d = A[:, k][:, None] - B[:, k][None, :]
        d2 += d * d
    return np.exp(-d2 / (2.0 * ell * ell))


def gram(X, ell, alpha):
    K = kernel(X, X, ell)
    K[np.diag_indices_from(K)] += alpha
    return K


def fit(X, y, ell, alpha):
    """alpha_ (N, D) = (K + alpha I)^-1 y through the Cholesky factor; no centring (normalize_y=False)"""
    L = np.linalg.cholesky(gram(X, ell, alpha))
    return np.linalg.solve(L.T, np.linalg.solve(L, np.asarray(y, dtype=np.float64)))


def fit_large(X, y, ell, alpha):
    """(K + alpha I)^-1 y for training sets of thousands, where `gram`'s loop over the cells of an N x N matrix takes minutes:
    K in the GEMM form clamped at 0, one symmetric solve.  For checks in which any fixed coefficients serve."""
    X = np.asarray(X, dtype=np.float64)
    sq = (X * X).sum(axis=1)
    K = sq[:, None] + sq[None, :] - 2.0 * (X @ X.T)
    np.maximum(K, 0.0, out=K)
    K *= -1.0 / (2.0 * ell * ell)
    np.exp(K, out=K)
    K[np.diag_indices_from(K)] += alpha
    try:
        from scipy.linalg import solve
        return solve(K, np.asarray(y, dtype=np.float64), assume_a="pos", overwrite_a=True, check_finite=False)
    except ImportError:
        return np.linalg.solve(K, np.asarray(y, dtype=np.float64))


def predict(Xq, X, alpha_, ell):
    return kernel(Xq, X, ell) @ alpha_


def emulate_fp32(Xq, X, alpha_, ell, block=2048):
    """The kernel's arithmetic in float32: training matrix, |x_j|^2 and alpha_ rounded to float32, the GEMM-form distance
    |x*|^2 + |x_j|^2 - 2 x*.x_j in float32 clamped at 0, a float32 exponential, float32 accumulation.  -> (S, D) float32"""
    Xq32, X32 = np.asarray(Xq, dtype=np.float32), np.asarray(X, dtype=np.float32)
    al32 = np.asarray(alpha_, dtype=np.float32)
    sq_t = (X32.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    inv = np.float32(1.0 / (2.0 * ell * ell))
    out = np.zeros((Xq32.shape[0], al32.shape[1]), dtype=np.float32)
    for s in range(0, Xq32.shape[0], block):
        q = Xq32[s:s + block]
        sq_q = (q * q).sum(axis=1, dtype=np.float32)
        d2 = (sq_q[:, None] + sq_t[None, :]) - np.float32(2.0) * (q @ X32.T)
        k = np.exp(-(np.maximum(d2, np.float32(0.0)) * inv)).astype(np.float32)
        out[s:s + block] = k @ al32
    return out


def l1(alpha_):
    """sum_j |alpha_[j][d]| per target column: the scale of every fp32 allowance"""
    return np.abs(np.asarray(alpha_, dtype=np.float64)).sum(axis=0)
