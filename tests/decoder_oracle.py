"""Float64 NumPy restatement of the linear decoder (csrc/riab_decoder.hip + ratinabox_amd/_decoder.py): the moment
matrix of the augmented sample vector with the kernel's masking rule, sklearn's Ridge with an intercept solved from it,
and predictions.  Test infrastructure only."""
import numpy as np


def samples(inputs, traj, target_rows, n_real, t_step=1):
    """(Z float64 (S, m), n_dropped): the kept samples of history rows 0, t_step, ... as rows [x ; y ; 1].
    inputs: list of float32 (T, n_l, B); traj float32 (T, 8, B).  Left out: lanes b >= n_real; samples with a non-finite
    target value (counted)."""
    x = np.concatenate([np.asarray(a)[::t_step, :, :n_real] for a in inputs], axis=1).astype(np.float64)   # (Tu, n, B)
    y = np.asarray(traj)[::t_step][:, list(target_rows), :n_real].astype(np.float64)                          # (Tu, D, B)
    keep = np.isfinite(y).all(axis=1)                                                                        # (Tu, B)
    z = np.concatenate((x, y, np.ones_like(y[:, :1])), axis=1).transpose(0, 2, 1)[keep]                      # (S, m)
    return z, int((~keep).sum())


def moments(inputs, traj, target_rows, n_real, t_step=1):
    """(M float64 (m, m) = sum of z z^T over the kept samples, n_dropped)."""
    z, dropped = samples(inputs, traj, target_rows, n_real, t_step)
    return z.T @ z, dropped


def abs_moments(inputs, traj, target_rows, n_real, t_step=1):
    """sum of |z_i z_j|: the scale of the rounding allowance of a reordered float64 sum."""
    z, _ = samples(inputs, traj, target_rows, n_real, t_step)
    return np.abs(z).T @ np.abs(z)


def centred(M, n, D):
    """(A without the ridge term = G - N xbar xbar^T, C_c = C - N xbar ybar^T, xbar, ybar, N) from a moment matrix."""
    N = M[-1, -1]
    xbar, ybar = M[-1, :n] / N, M[-1, n:n + D] / N
    return M[:n, :n] - N * np.outer(xbar, xbar), M[:n, n:n + D] - N * np.outer(xbar, ybar), xbar, ybar, N


def ridge(M, n, D, alpha):
    """sklearn.linear_model.Ridge(alpha, fit_intercept=True) from the moments: (coef (D, n), intercept (D,))."""
    A, Cc, xbar, ybar, _ = centred(M, n, D)
    W = np.linalg.solve(A + alpha * np.eye(n), Cc)          # (n, D)
    return W.T.copy(), ybar - xbar @ W


def predict(coef, intercept, x):
    """x (S, n) float -> (S, D) float64."""
    return np.asarray(x, dtype=np.float64) @ np.asarray(coef).T + np.asarray(intercept)
