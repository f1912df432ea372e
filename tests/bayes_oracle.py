"""A float64 NumPy restatement of the Bayesian (Poisson maximum-likelihood) decoder (ratinabox_amd/_bayes_decoder.py,
csrc/riab_bayes.hip): the tables from tuning curves, the log posterior, the six outputs of a sample and the window counts.

Cells c = 1..n, bins j = 1..J with centres x_j and tuning f_cj >= 0 (Hz); a window of W rows has duration tau = W dt and k_c
spikes of cell c (inputs "rates": k_c = tau rate_c, W = 1).

    L_cj   = log max(f_cj, rate_floor)          S_j = sum_c max(f_cj, rate_floor)
    bias_j = log prior_j - tau S_j              (-inf for a bin that is not admissible)
    l_j    = sum_c k_c L_cj + bias_j

    outputs: sum_j softmax(l)_j x_j (x, y); x_j* (x, y), j* the LOWEST j among the maxima; logsumexp_j l_j; softmax(l)_j*
    — six NaNs if no bin is admissible.

`decode_float32` is the same formula in plain float32 NumPy: the yardstick the kernel's measured error is set against."""
import numpy as np


def tables(curves, admissible=None, prior_weights=None, rate_floor=1e-2):
    """(L (n, J), S (J,), log prior (J,)) float64 from tuning curves (n, J) (or a list of them, stacked)"""
    f = np.concatenate([np.asarray(c, dtype=np.float64) for c in curves], axis=0) if isinstance(curves, (list, tuple)) \
        else np.asarray(curves, dtype=np.float64)
    J = f.shape[1]
    F = np.maximum(f, float(rate_floor))
    ok = np.ones(J, dtype=bool) if admissible is None else np.asarray(admissible, dtype=bool).reshape(J)
    w = ok.astype(np.float64) if prior_weights is None else ok * np.asarray(prior_weights, dtype=np.float64).reshape(J)
    with np.errstate(divide="ignore"):
        logp = np.where(w > 0, np.log(w / w.sum()), -np.inf)
    return np.log(F), F.sum(axis=0), logp


def bias(log_prior, S, tau):
    return np.asarray(log_prior, dtype=np.float64) - float(tau) * np.asarray(S, dtype=np.float64)


def log_posterior(k, L, b):
    """k (S, n) counts, L (n, J), b (J,) -> l (S, J) float64"""
    return np.asarray(k, dtype=np.float64) @ np.asarray(L, dtype=np.float64) + np.asarray(b, dtype=np.float64)[None, :]


def map_bin(ell):
    """the lowest index among the maxima of every row (np.argmax's rule); -1 where no bin is admissible"""
    j = np.argmax(ell, axis=1)
    return np.where(np.isfinite(ell[np.arange(len(ell)), j]), j, -1)


def outputs(ell, centres):
    """l (S, J), centres (2, J) -> (S, 6) float64"""
    ell = np.asarray(ell, dtype=np.float64)
    centres = np.asarray(centres, dtype=np.float64)
    out = np.full((ell.shape[0], 6), np.nan)
    j = map_bin(ell)
    ok = j >= 0
    if ok.any():
        e, js = ell[ok], j[ok]
        m = e.max(axis=1)
        p = np.exp(e - m[:, None])
        Z = p.sum(axis=1)
        out[ok, 0], out[ok, 1] = (p @ centres[0]) / Z, (p @ centres[1]) / Z
        out[ok, 2], out[ok, 3] = centres[0, js], centres[1, js]
        out[ok, 4] = m + np.log(Z)
        out[ok, 5] = 1.0 / Z
    return out


def decode(k, L, b, centres):
    return outputs(log_posterior(k, L, b), centres)


def decode_float32(k, L, b, centres):
    """The same formula in plain float32 NumPy (float32 matmul, max, exp, sums): (S, 6) float32."""
    k32, L32, b32 = np.asarray(k, dtype=np.float32), np.asarray(L, dtype=np.float32), np.asarray(b, dtype=np.float32)
    c32 = np.asarray(centres, dtype=np.float32)
    ell = k32 @ L32 + b32[None, :]
    out = np.full((ell.shape[0], 6), np.nan, dtype=np.float32)
    j = map_bin(ell)
    ok = j >= 0
    if ok.any():
        e, js = ell[ok], j[ok]
        m = e.max(axis=1)
        p = np.exp(e - m[:, None])
        Z = p.sum(axis=1, dtype=np.float32)
        out[ok, 0], out[ok, 1] = (p @ c32[0]) / Z, (p @ c32[1]) / Z
        out[ok, 2], out[ok, 3] = c32[0, js], c32[1, js]
        out[ok, 4] = m + np.log(Z)
        out[ok, 5] = np.float32(1.0) / Z
    return out


def delta(k, L, b):
    """The a-priori fp32 bound on a sample's log posterior: (n + 3) 2^-24 max_j (sum_c k_c |L_cj| + |bias_j|) over the
    admissible bins, (S,) float64 (0 where none is admissible)."""
    k, L, b = np.asarray(k, dtype=np.float64), np.asarray(L, dtype=np.float64), np.asarray(b, dtype=np.float64)
    mag = np.abs(k) @ np.abs(L) + np.abs(b)[None, :]
    mag = np.where(np.isfinite(b)[None, :], mag, 0.0)
    return (L.shape[0] + 3) * 2.0 ** -24 * mag.max(axis=1)


def window_counts(spikes, window, modulo=True):
    """spikes (T, n, B) -> counts (T // window, n, B): the sums of `window` consecutive rows, trailing rows dropped; as uint8
    modulo 256 (what a byte holds) or as int64"""
    spikes = np.asarray(spikes)
    W = int(window)
    nw = spikes.shape[0] // W
    c = spikes[:nw * W].astype(np.int64).reshape((nw, W) + spikes.shape[1:]).sum(axis=1)
    return (c % 256).astype(np.uint8) if modulo else c


def window_of_rows(row0, length, window, n_windows):
    """the window of every row of a piece (row0 + r) // window, -1 for rows of windows >= n_windows"""
    w = (int(row0) + np.arange(int(length))) // int(window)
    return np.where(w < int(n_windows), w, -1)


def grid_centres(extent, dx):
    """centres (2, ny nx) of the maps np.histogram2d makes on np.arange(lo, hi + dx, dx) edges, flattened row-major over
    (ny, nx) with the first row the top of the room; -> (centres, ny, nx)"""
    ex = np.arange(float(extent[0]), float(extent[1]) + dx, dx)
    ey = np.arange(float(extent[2]), float(extent[3]) + dx, dx)
    nx, ny = len(ex) - 1, len(ey) - 1
    cx, cy = 0.5 * (ex[:-1] + ex[1:]), 0.5 * (ey[:-1] + ey[1:])
    X, Y = np.meshgrid(cx, cy[::-1])
    return np.stack((X.reshape(-1), Y.reshape(-1))), ny, nx
