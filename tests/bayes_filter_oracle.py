"""A float64 NumPy restatement of the Bayesian decoder's forward filter (ratinabox_amd/_bayes_decoder.py: BayesianFilter,
csrc/riab_bayes_filter.hip), on top of tests/bayes_oracle.py.

Bins j = 0..J-1 on a grid (ny, nx), row-major, square, `dx` wide; ok_j: log prior_j is finite; prior_j = exp(log prior_j).

    taps        R = max(1, ceil(3 sigma / dx)), g[d] ~ exp(-(d dx)^2 / (2 sigma^2)), d = -R..R, sum 1
    transition  G(j - j') = g[r - r'] g[c - c'] (0 beyond R either way); norm_j' = sum_j G(j - j') ok_j;
                T[j, j'] = ok_j G(j - j') / norm_j' for an admissible j', 0 otherwise
    predict     pred_t = (1 - mixing) T p_{t-1} + mixing prior;  pred_t = prior on the first window, on a window whose
                restart flag is set and on the window after one whose outputs are NaN
    update      l_t(j) = sum_c k_c L_cj - tau S_j + log pred_t(j);  p_t = softmax(l_t);  six outputs as bayes_oracle.outputs

`filter_float32` is the same recursion in plain float32 NumPy: the yardstick the kernel's measured error is set against."""
import numpy as np

from tests import bayes_oracle as orc


def taps(sigma, dx):
    """(R, g float64 (2R + 1,))"""
    sigma, dx = float(sigma), float(dx)
    R = max(1, int(np.ceil(3.0 * sigma / dx)))
    d = np.arange(-R, R + 1, dtype=np.float64) * dx
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    return R, g / g.sum()


def blur(P, g):
    """The separable step sum_j' G(j - j') P(j') of P (..., ny, nx), taps that leave the grid dropped: first along x, then
    along y, each as a sum over d ascending."""
    R = (len(g) - 1) // 2
    ny, nx = P.shape[-2:]
    X = np.zeros_like(P)
    for d in range(-R, R + 1):          # X(r, c) += g[d] P(r, c + d)
        lo, hi = max(0, -d), min(nx, nx - d)
        if lo < hi:
            X[..., :, lo:hi] += g[d + R] * P[..., :, lo + d:hi + d]
    Y = np.zeros_like(P)
    for d in range(-R, R + 1):
        lo, hi = max(0, -d), min(ny, ny - d)
        if lo < hi:
            Y[..., lo:hi, :] += g[d + R] * X[..., lo + d:hi + d, :]
    return Y


def inv_norm(ok, g):
    """ok bool (ny, nx) -> 1 / norm_j' (ny, nx) float64, 0 where the bin is not admissible"""
    norm = blur(ok.astype(np.float64), g)
    with np.errstate(divide="ignore"):
        return np.where(ok, 1.0 / norm, 0.0)


def propagate(p, ok, g):
    """T p for p (..., J): the separable form the filter uses"""
    ny, nx = ok.shape
    q = p.reshape(p.shape[:-1] + (ny, nx)) * inv_norm(ok, g).astype(p.dtype)
    return (blur(q, g.astype(p.dtype)) * ok).reshape(p.shape)


def dense_transition(ok, g):
    """T (J, J) float64 from the definition, entry by entry: T[j, j'] = ok_j g[r - r'] g[c - c'] / norm_j'"""
    R = (len(g) - 1) // 2
    ny, nx = ok.shape
    J = ny * nx
    G = np.zeros((J, J))
    for j in range(J):
        r, c = divmod(j, nx)
        for jp in range(J):
            rp, cp = divmod(jp, nx)
            if abs(r - rp) <= R and abs(c - cp) <= R:
                G[j, jp] = g[r - rp + R] * g[c - cp + R]
    flat = ok.reshape(-1)
    norm = (G * flat[:, None]).sum(axis=0)
    T = np.zeros((J, J))
    for jp in range(J):
        if flat[jp]:
            T[:, jp] = flat * G[:, jp] / norm[jp]
    return T


def _outputs(ell, centres, dtype):
    if dtype == np.float64:
        return orc.outputs(ell, centres)
    c32 = np.asarray(centres, dtype=np.float32)
    out = np.full((ell.shape[0], 6), np.nan, dtype=np.float32)
    j = orc.map_bin(ell)
    good = j >= 0
    if good.any():
        e, js = ell[good], j[good]
        m = e.max(axis=1)
        p = np.exp(e - m[:, None])
        Z = p.sum(axis=1, dtype=np.float32)
        out[good, 0], out[good, 1] = (p @ c32[0]) / Z, (p @ c32[1]) / Z
        out[good, 2], out[good, 3] = c32[0, js], c32[1, js]
        out[good, 4] = m + np.log(Z)
        out[good, 5] = np.float32(1.0) / Z
    return out


def _filter(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, dtype):
    k = np.asarray(k, dtype=dtype)                            # (T, B, n)
    T, B = k.shape[:2]
    L, S = np.asarray(L, dtype=dtype), np.asarray(S, dtype=dtype)
    logp = np.asarray(log_prior, dtype=dtype)
    ok = np.isfinite(logp)
    prior = np.exp(logp)
    g = np.asarray(g, dtype=np.float64)
    eps = dtype(mixing)
    with np.errstate(invalid="ignore"):
        lik = k @ L - dtype(tau) * S[None, None, :]
    lik[:, :, ~ok] = -np.inf
    out = np.full((T, B, 6), np.nan, dtype=dtype)
    ells = np.empty((T, B, len(logp)), dtype=dtype)
    fresh = np.ones(B, dtype=bool)
    p = None
    for t in range(T):
        f = fresh if restart is None else fresh | np.asarray(restart[t], dtype=bool)[:B]
        logpred = np.broadcast_to(logp, (B, len(logp))).copy()
        if p is not None and not f.all():
            pred = (dtype(1) - eps) * propagate(p, ok.reshape(shape), g) + eps * prior[None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                logpred[~f] = np.log(pred[~f])
        with np.errstate(invalid="ignore"):
            ell = lik[t] + logpred
        ells[t] = ell
        out[t] = _outputs(ell, centres, dtype)
        fresh = np.isnan(out[t, :, 4])
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.where(fresh, dtype(0), np.where(np.isfinite(ell), ell, -np.inf).max(axis=1))
            e = np.exp(ell - m[:, None])
            p = e / e.sum(axis=1, keepdims=True, dtype=dtype)
        p[fresh] = 0
    return out, ells


def filter_float64(k, L, S, tau, log_prior, shape, g, mixing, centres, restart=None):
    """k (T, B, n) counts of consecutive windows, L (n, J), S (J,), log_prior (J,), shape (ny, nx), g the taps (2R + 1,),
    centres (2, J), restart bool (T, B) or None -> (outputs (T, B, 6), l (T, B, J)) float64"""
    return _filter(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, np.float64)


def filter_float32(k, L, S, tau, log_prior, shape, g, mixing, centres, restart=None):
    """The same recursion with every array and every operation in float32 -> (outputs, l) float32"""
    return _filter(k, L, S, tau, log_prior, shape, g, mixing, centres, restart, np.float32)
