"""A float64 NumPy restatement of the Bayesian decoder's backward smoother (ratinabox_amd/_bayes_decoder.py:
BayesianSmoother, csrc/riab_bayes_smooth.hip), on top of tests/bayes_filter_oracle.py, whose notation this keeps.

The forward filter gives l_t, its six outputs and ev_t = its row 4 = log p(k_t | k_<t); p_t(j) = exp(l_t(j) - ev_t).  With
beta of the last window 1 and t descending,

    u_{t+1}(j) = exp(loglik_{t+1}(j) - ev_{t+1}) beta_{t+1}(j)                        0 where j is not admissible
    c_t        = sum_j prior_j u_{t+1}(j)
    beta_t(j') = (1 - mixing) inv_norm_j' sum_j G(j - j') u_{t+1}(j) + mixing c_t ok_j'
    gamma_t    = p_t beta_t / sum_i p_t(i) beta_t(i)

The chain is cut at window t (beta_t = 1: gamma_t = p_t and the six outputs are the filter's) when t is the last window, when
window t + 1 has its restart flag set or came out as NaN, and when window t came out as NaN.  Outputs (T, B, 6): the mean of
gamma_t (x, y); the centre of its MAP bin (the lowest index among the maxima); ev_t; gamma_t at the MAP bin.

`smooth_float64` is that recursion.  `smooth_dense` is written apart from it: the dense transition matrix of the definition,
T = (1 - mixing) dense_transition + mixing prior 1^T, and the textbook alpha / beta passes over every segment between restarts.
`smooth_float32` is the recursion with every array and operation in float32 NumPy: the yardstick the kernel's error is set
against."""
import numpy as np

from tests import bayes_filter_oracle as flt


def loglik(k, L, S, tau, log_prior, dtype=np.float64):
    """sum_c k_c L_cj - tau S_j, -inf where the bin is not admissible: (T, B, J)"""
    k, L, S = np.asarray(k, dtype=dtype), np.asarray(L, dtype=dtype), np.asarray(S, dtype=dtype)
    with np.errstate(invalid="ignore"):
        lik = k @ L - dtype(tau) * S[None, None, :]
    lik[:, :, ~np.isfinite(np.asarray(log_prior))] = -np.inf
    return lik


def cuts(filtered, restart):
    """bool (T, B): the chain is cut at window t of column b"""
    T, B = filtered.shape[:2]
    bad = np.isnan(filtered[:, :, 4])
    cut = bad.copy()
    cut[T - 1] = True
    cut[:-1] |= bad[1:]
    if restart is not None:
        cut[:-1] |= np.asarray(restart, dtype=bool)[1:, :B]
    return cut


def _smooth(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, dtype):
    filtered, ells = flt._filter(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, dtype)
    lik = loglik(k, L, S, tau, log_prior, dtype)
    T, B, J = ells.shape
    logp = np.asarray(log_prior, dtype=dtype)
    ok = np.isfinite(logp)
    prior = np.exp(logp)
    g = np.asarray(g, dtype=np.float64)
    inv = flt.inv_norm(ok.reshape(shape), g).reshape(-1).astype(dtype)
    g, eps, cen = g.astype(dtype), dtype(mixing), np.asarray(centres, dtype=dtype)
    cut = cuts(filtered, restart)
    ev = filtered[:, :, 4]
    out = filtered.copy()
    gamma = np.zeros((T, B, J), dtype=dtype)
    total = np.ones((T, B), dtype=dtype)                     # sum_i p_t(i) beta_t(i) before it is divided out
    beta = np.ones((B, J), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(T - 1, -1, -1):
            if t < T - 1:
                u = np.exp(lik[t + 1] - ev[t + 1][:, None]) * beta
                u[:, ~ok] = 0
                c = (prior[None, :] * u).sum(axis=1, dtype=dtype)
                carried = (dtype(1) - eps) * inv[None, :] * flt.blur(u.reshape((B,) + tuple(shape)), g).reshape(B, J) \
                    + eps * c[:, None] * ok[None, :]
                beta = np.where(cut[t][:, None], dtype(1), carried).astype(dtype)
            gm = np.exp(ells[t] - ev[t][:, None]) * beta
            gm[:, ~ok] = 0
            z = gm.sum(axis=1, dtype=dtype)
            total[t] = z
            gamma[t] = gm / z[:, None]
            live = ~cut[t]
            if live.any():
                j = np.argmax(gm[live], axis=1)              # the first of the maxima
                out[t, live, 0], out[t, live, 1] = (gm[live] @ cen[0]) / z[live], (gm[live] @ cen[1]) / z[live]
                out[t, live, 2], out[t, live, 3] = cen[0, j], cen[1, j]
                out[t, live, 5] = gm[live, j] / z[live]
    return out, gamma, filtered, total


def smooth_float64(k, L, S, tau, log_prior, shape, g, mixing, centres, restart=None):
    """k (T, B, n) counts of the consecutive windows of one run, the other arguments as `filter_float64` takes them ->
    (outputs (T, B, 6), gamma (T, B, J), the filter's outputs (T, B, 6), sum_i p_t beta_t (T, B)) float64"""
    return _smooth(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, np.float64)


def smooth_float32(k, L, S, tau, log_prior, shape, g, mixing, centres, restart=None):
    """The same recursion with every array and every operation in float32"""
    return _smooth(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, np.float32)


def transition_matrix(log_prior, shape, g, mixing):
    """T[j, j'] = p(x_t+1 = j | x_t = j') (J, J) float64 = (1 - mixing) dense_transition + mixing prior 1^T"""
    logp = np.asarray(log_prior, dtype=np.float64)
    ok = np.isfinite(logp)
    return (1.0 - mixing) * flt.dense_transition(ok.reshape(shape), np.asarray(g, dtype=np.float64)) \
        + mixing * np.exp(logp)[:, None] * np.ones(len(logp))[None, :]


def smooth_dense(k, L, S, tau, log_prior, shape, g, mixing, restart=None):
    """gamma (T, B, J) float64 by the textbook forward-backward passes with the dense matrix, segment by segment (a segment
    starts at window 0 and at every set restart flag).  Finite inputs only."""
    lik = loglik(k, L, S, tau, log_prior)
    T, B, J = lik.shape
    logp = np.asarray(log_prior, dtype=np.float64)
    ok, prior = np.isfinite(logp), np.exp(logp)
    Tm = transition_matrix(log_prior, shape, g, mixing)
    gamma = np.zeros((T, B, J))
    for b in range(B):
        starts = [0] + [t for t in range(1, T) if restart is not None and restart[t][b]] + [T]
        for s0, s1 in zip(starts[:-1], starts[1:]):
            n = s1 - s0
            e = np.exp(lik[s0:s1, b] - lik[s0:s1, b][:, ok].max(axis=1, keepdims=True))      # (n, J), 0 where not admissible
            alpha, beta = np.zeros((n, J)), np.ones((n, J))
            alpha[0] = prior * e[0]
            alpha[0] /= alpha[0].sum()
            for i in range(1, n):
                alpha[i] = e[i] * (Tm @ alpha[i - 1])
                alpha[i] /= alpha[i].sum()
            for i in range(n - 2, -1, -1):
                beta[i] = Tm.T @ (e[i + 1] * beta[i + 1])
                beta[i] /= beta[i].max()
            gm = alpha * beta
            gamma[s0:s1, b] = gm / gm.sum(axis=1, keepdims=True)
    return gamma
