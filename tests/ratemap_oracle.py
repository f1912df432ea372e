"""The float64 restatement the rate-map tests hold the device path to: plain np.histogram2d with explicit edges on the
fp32 samples widened to float64 (reference utils.py:544-589).  Shared by the CPU and the GPU tests."""
import numpy as np


def edges(extent, dx):
    return np.arange(extent[0], extent[1] + dx, dx), np.arange(extent[2], extent[3] + dx, dx)


def oriented(h):
    """heatmap[kx, ky] -> the reference's heatmap.T[::-1, :]: (ny, nx), first row the top of the room."""
    return np.ascontiguousarray(h.T[::-1, :])


def samples(traj, n_real):
    """(x, y) float64 of every (step, real agent) sample of trajectory rows traj float32 (T, 8, B)."""
    t = np.asarray(traj)
    assert t.dtype == np.float32
    return t[:, 0, :n_real].astype(np.float64).reshape(-1), t[:, 1, :n_real].astype(np.float64).reshape(-1)


def counts(traj, n_real, ex, ey):
    x, y = samples(traj, n_real)
    return oriented(np.histogram2d(x, y, bins=[ex, ey])[0])


def rate_maps(traj, rows, n_real, ex, ey, norm):
    """(maps (n, ny, nx) float64, zero_bins (ny, nx) bool, counts (ny, nx)) for rows (T, n, B) float32 or uint8."""
    x, y = samples(traj, n_real)
    r = np.asarray(rows)
    cnt = np.histogram2d(x, y, bins=[ex, ey])[0]
    zero = cnt == 0
    div = cnt.copy()
    div[zero] = 1
    out = []
    for c in range(r.shape[1]):
        w = r[:, c, :n_real].astype(np.float64).reshape(-1)
        h = np.histogram2d(x, y, bins=[ex, ey], weights=w)[0]
        out.append(oriented(h / div if norm else h))
    shape = oriented(cnt).shape
    return np.array(out).reshape((r.shape[1],) + shape), oriented(zero), oriented(cnt)


def searchsorted_bins(x, e):
    """The bin of each x on edges e by the searchsorted rule (k, or -1 for a dropped sample)."""
    x = np.asarray(x, dtype=np.float64)
    k = np.searchsorted(e, x, side="right") - 1
    k[x == e[-1]] = len(e) - 2
    k[(k < 0) | (x > e[-1]) | np.isnan(x)] = -1
    return k
