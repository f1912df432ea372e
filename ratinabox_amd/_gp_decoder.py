"""Gaussian-process decoders fitted and run where the history lives.

Beside its Ridge the reference decodes position with `sklearn.gaussian_process.GaussianProcessRegressor(alpha=0.01,
kernel=RBF(sqrt(n / 20), length_scale_bounds="fixed"))` (tests/test_advanced.py::test_decoding_position, the decoding demo):
the decoder that works on grid-cell and thresholded place-cell rates, where a linear read-out is weak.  Here a training set
of (row, agent) samples is GATHERED from the history chunks by torch indexing on the device (it is small and chosen once,
by a deterministic rule), the N x N system

    K = exp(-max(0, sq_i + sq_j - 2 X X^T) / (2 l^2)) + alpha I,     alpha_ = K^-1 y        (Cholesky, float64)

is solved with torch.linalg on the same device (sklearn's default normalize_y=False: nothing is centred), and the predictive
mean of every (row, agent) sample of the history,

    mean(x*) = sum_j exp(-|x* - x_j|^2 / (2 l^2)) alpha_[j],

goes through `torch.ops.riab.gp_predict` (csrc/riab_gp.hip): one fused kernel on the fp32 matrix cores that never writes
the (samples x N) kernel matrix to memory.  There is no `as_layer()`: a GP is not a FeedForwardLayer.

With `return_std=True` the predictive standard deviation comes with the mean, in sklearn's own formulation
(`predict(return_std=True)`): with K + alpha I = L L^T and k*_j = k(x*, x_j),

    var(x*) = 1 - |L^-1 k*|^2,     std = sqrt(max(var, 0))                (k(x*, x*) = 1 for the RBF; NaN stays NaN)

one number per query, the same for every target column.  `torch.ops.riab.gp_predict_var` runs it in two launches: the mean's
kernel also stores k* into a workspace `[T][Np][B]`, and a second kernel contracts it with the transposed inverse factor
(`GPDecoder._variance_table`) over the triangular half and sums the squares.  The workspace is the one thing that scales
with the number of queries, so the work is cut into pieces that fit `max_workspace_bytes`; the result does not depend on
the cut."""
import math

import numpy as np
import torch

from . import _lib as _L
from . import ops as _ops  # noqa: F401  (registers torch.ops.riab.gp_predict)
from ._decoder import TARGETS, HistoryDecoder, _check_populations, _rows

MAX_SAMPLES = _L.GP_MAX_TRAIN
GOLDEN_RATIO_FRAC = (math.sqrt(5.0) - 1.0) / 2.0


def select_samples(n_rows, n_agents, max_samples):
    """The training set's candidates, deterministic and without a random number: (row indices into the R selected rows,
    agents), int64 arrays in time-major order.  R * B <= max_samples: every (row, agent).  Otherwise sample i of
    max_samples takes row floor(i R / max_samples) and agent floor(B frac((i + 1) phi)), phi = (sqrt(5) - 1) / 2 in
    float64 — a low-discrepancy walk over the agents, so that no agent is favoured whatever R B / max_samples is (a plain
    stride over the flattened index lands on ONE agent whenever that ratio is a multiple of B) — with duplicates removed."""
    R, B, N = int(n_rows), int(n_agents), int(max_samples)
    if R < 1 or B < 1:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if R * B <= N:
        flat = np.arange(R * B, dtype=np.int64)
    else:
        i = np.arange(N, dtype=np.int64)
        rows = (i * R) // N
        agents = np.minimum(np.floor(B * np.modf((i + 1).astype(np.float64) * GOLDEN_RATIO_FRAC)[0]).astype(np.int64), B - 1)
        flat = np.unique(rows * B + agents)
    return flat // B, flat % B


def workspace_pieces(T, B, Np, max_workspace_bytes):
    """How `predict_tensor(return_std=True)` cuts T rows of B columns into pieces whose workspace (4 Np bytes per (row,
    column)) fits `max_workspace_bytes`: [(t0, t1, c0, c1)], every (row, column) once, rows ascending and columns ascending
    within a row.  Whole rows while one fits; otherwise one row at a time in blocks of columns that are multiples of 128
    (the kernels' position tile).  Raises ValueError when 128 columns of one row do not fit."""
    T, B, Np, limit = int(T), int(B), int(Np), int(max_workspace_bytes)
    rows = limit // (4 * Np * B) if B > 0 else T
    if rows >= 1:
        return [(t, min(t + rows, T), 0, B) for t in range(0, T, rows)]
    cols = limit // (4 * Np) // 128 * 128
    if cols < 128:
        raise ValueError(f"max_workspace_bytes = {limit} is too small: one row of {min(B, 128)} columns against {Np} "
                         f"(padded) training samples needs {4 * Np * min(B, 128)} bytes")
    return [(t, t + 1, c, min(c + cols, B)) for t in range(T) for c in range(0, B, cols)]


def _check_hyper(alpha, length_scale, n_total):
    if not float(alpha) >= 0:
        raise ValueError(f"alpha must be >= 0, got {alpha}")
    if length_scale is None:
        return math.sqrt(n_total / 20.0)   # the reference's rule
    if np.ndim(length_scale) != 0 or isinstance(length_scale, (str, bytes)):
        raise ValueError("length_scale must be a scalar (anisotropic length scales are not built)")
    ell = float(length_scale)
    if not (ell > 0 and math.isfinite(ell)):
        raise ValueError(f"length_scale must be a finite positive number, got {length_scale}")
    return ell


class GPDecoder(HistoryDecoder):
    """GaussianProcessRegressor(alpha, RBF(length_scale), optimizer=None, normalize_y=False), fitted.  `X_train_` (N, n)
    and `alpha_` (N, D) are float64 tensors on the fit's device; `train_rows` / `train_agents` int64 tensors (history row
    and agent of every training sample, time-major) or None for a decoder made from bare samples.
    `log_marginal_likelihood_` is the float64 log marginal likelihood of the training targets under these hyper-parameters
    (sklearn's `log_marginal_likelihood_value_`: summed over the target columns), a Python float, or None for a decoder
    constructed directly: what two choices of `length_scale` or `alpha` are compared with."""

    def __init__(self, X, alpha_, length_scale, alpha, widths=None, target="pos", populations=None, train_rows=None,
                 train_agents=None, n_dropped=0, log_marginal_likelihood=None):
        self.X_train_, self.alpha_ = X, alpha_
        self.length_scale, self.alpha = float(length_scale), float(alpha)
        self.widths = [int(X.shape[1])] if widths is None else [int(w) for w in widths]
        if sum(self.widths) != int(X.shape[1]):
            raise ValueError(f"widths {self.widths} do not add up to the {int(X.shape[1])} columns of X")
        self.target = target
        self.populations = None if populations is None else list(populations)
        self.train_rows, self.train_agents = train_rows, train_agents
        self.n_samples, self.n_dropped = int(X.shape[0]), int(n_dropped)
        self.log_marginal_likelihood_ = None if log_marginal_likelihood is None else float(log_marginal_likelihood)
        self._tables = None
        self._linv_t = None

    @classmethod
    def from_samples(cls, X, y, length_scale=None, alpha=0.01, **kw):
        """The fit from bare samples: X float64 (N, n), y float64 (N, D), D = 1..4, on any device (the CPU included)."""
        if X.dtype != torch.float64 or y.dtype != torch.float64 or X.dim() != 2 or y.dim() != 2 or y.shape[0] != X.shape[0] \
                or X.device != y.device:
            raise ValueError("X must be a float64 tensor (N, n) and y a float64 tensor (N, D) on the same device")
        N, n = int(X.shape[0]), int(X.shape[1])
        if not 1 <= N <= MAX_SAMPLES or n < 1 or not 1 <= int(y.shape[1]) <= _L.GP_MAX_OUT:
            raise ValueError(f"a GP decoder takes 1..{MAX_SAMPLES} training samples of >= 1 cells and 1..{_L.GP_MAX_OUT} "
                             f"target columns, got X {tuple(X.shape)}, y {tuple(y.shape)}")
        ell = _check_hyper(alpha, length_scale, n)
        if not bool(torch.isfinite(X).all()):
            raise ValueError("a training rate is not finite")
        if not bool(torch.isfinite(y).all()):
            raise ValueError("a training target is not finite")
        K = kernel_matrix(X, X, ell)
        K.diagonal().add_(float(alpha))
        L, info = torch.linalg.cholesky_ex(K)
        if int(info.item()) != 0:
            raise ValueError(f"the kernel matrix + alpha I is not positive definite at alpha = {alpha} (leading minor "
                             f"{int(info.item())}): duplicate or nearly equal training samples need a larger alpha")
        alpha_ = torch.cholesky_solve(y, L)
        # -1/2 y^T alpha_ - sum log L_ii - N/2 log 2 pi per target column, summed over the columns (L is not kept)
        D = int(y.shape[1])
        lml = -0.5 * float((y * alpha_).sum()) - D * float(torch.log(L.diagonal()).sum()) - 0.5 * D * N * math.log(2.0 * math.pi)
        return cls(X, alpha_, ell, alpha, log_marginal_likelihood=lml, **kw)

    def mean_float64(self, X):
        """The predictive mean in float64 with torch on X's device, X float64 (S, n) -> (S, D): the definition the kernel is
        checked against, for a handful of samples (it materialises the S x N kernel matrix)."""
        return kernel_matrix(X, self.X_train_.to(X.device), self.length_scale) @ self.alpha_.to(X.device)

    def _factor(self, dev):
        """L of K + alpha I = L L^T, float64 on `dev`, factorised again from X_train_ (the fit does not keep it)"""
        X = self.X_train_.to(dev)
        K = kernel_matrix(X, X, self.length_scale)
        K.diagonal().add_(self.alpha)
        return torch.linalg.cholesky(K)

    def std_float64(self, X):
        """The predictive standard deviation in float64 with torch on X's device, X float64 (S, n) -> (S,): sklearn's
        sqrt(max(0, 1 - |L^-1 k*|^2)), the definition the kernels are checked against, for a handful of samples (it
        factorises K + alpha I again and materialises the S x N kernel matrix)."""
        ks = kernel_matrix(X, self.X_train_.to(X.device), self.length_scale)
        V = torch.linalg.solve_triangular(self._factor(X.device), ks.T, upper=False)      # (N, S)
        var = 1.0 - (V * V).sum(dim=0)
        return torch.sqrt(torch.where(var < 0, torch.zeros_like(var), var))

    # ---- running the decoder (riab_gp_predict) ---------------------------------------------------------------------------
    def _populations(self):
        if self.populations is None:
            raise ValueError("this decoder was built from bare samples: it has no populations to read rates from")
        return self.populations

    def _device_tables(self, dev):
        """(training matrix per population TRANSPOSED float32 (n_l, Np), |x_j|^2 float32 (Np,), alpha float32 (D, Np)),
        Np = N rounded up to 32, zero padded: what riab_gp_predict reads"""
        if self._tables is None or self._tables[1].device != torch.device(dev):
            N, D = self.n_samples, int(self.alpha_.shape[1])
            Np = (N + 31) // 32 * 32
            X = self.X_train_.to(dev)
            wts, k = [], 0
            for w in self.widths:
                wt = torch.zeros((w, Np), dtype=torch.float32, device=dev)
                wt[:, :N] = X[:, k:k + w].T.to(torch.float32)
                wts.append(wt)
                k += w
            sq = torch.zeros(Np, dtype=torch.float32, device=dev)
            sq[:N] = (X * X).sum(dim=1).to(torch.float32)
            al = torch.zeros((D, Np), dtype=torch.float32, device=dev)
            al[:, :N] = self.alpha_.to(dev).T.to(torch.float32)
            self._tables = (wts, sq, al)
        return self._tables

    def _variance_table(self, dev):
        """linv_t float32 (Np, Np): linv_t[j][i] = (L^-1)[i][j], exactly zero above the diagonal of L^-1 and in the padding:
        what riab_gp_predict_var reads.  Built on first use (K + alpha I is factorised again in float64 on `dev`, L^-1 taken
        by a triangular solve against the identity) and kept per device like `_device_tables`: 4 Np^2 bytes, 1 GB at the
        16 384-sample limit (and four float64 N x N matrices, 8 GB there, while it is built).  Calls without return_std
        never build it."""
        if self._linv_t is None or self._linv_t.device != torch.device(dev):
            N = self.n_samples
            Np = (N + 31) // 32 * 32
            eye = torch.eye(N, dtype=torch.float64, device=dev)
            linv = torch.linalg.solve_triangular(self._factor(dev), eye, upper=False).tril_()
            del eye
            table = torch.zeros((Np, Np), dtype=torch.float32, device=dev)
            table[:N, :N] = linv.T.to(torch.float32)
            self._linv_t = table
        return self._linv_t

    def predict_tensor(self, rates, return_std=False, max_workspace_bytes=2 ** 28):
        """The predictive mean of rates that are not in a history: a list of float32 `[T][n_l][Bp]` device tensors, one per
        population (widths as fitted) -> float32 `[T][D][Bp]`.  return_std=True: (mean `[T][D][Bp]`, std `[T][Bp]`), the
        mean with the bits it has without the flag.  The kernel values pass through a workspace of 4 Np bytes per (row,
        column); the work is cut into the `workspace_pieces` that fit `max_workspace_bytes` (whole rows first, then blocks of
        columns that are multiples of 128, which are copied to make them contiguous), and the result is bit-identical for
        every cut.  ValueError when 128 columns of one row do not fit `max_workspace_bytes`."""
        rates = list(rates)
        if len(rates) != len(self.widths) or any(int(x.shape[1]) != w for x, w in zip(rates, self.widths)):
            raise ValueError(f"this decoder takes {len(self.widths)} rate tensors (T, n_l, Bp) of widths {self.widths}")
        dev = rates[0].device
        wts, sq, al = self._device_tables(dev)
        inv = 1.0 / (2.0 * self.length_scale ** 2)
        if not return_std:
            return torch.ops.riab.gp_predict(rates, wts, sq, al, self.n_samples, inv)
        T, B, Np, D = int(rates[0].shape[0]), int(rates[0].shape[2]), int(sq.shape[0]), int(al.shape[0])
        pieces = workspace_pieces(T, B, Np, max_workspace_bytes)
        linv_t = self._variance_table(dev)
        ws = torch.empty(max([(t1 - t0) * Np * (c1 - c0) for t0, t1, c0, c1 in pieces], default=0), dtype=torch.float32,
                         device=dev)
        mean = var = None
        for t0, t1, c0, c1 in pieces:
            whole = c0 == 0 and c1 == B
            part = [x[t0:t1] if whole else x[t0:t1, :, c0:c1].contiguous() for x in rates]
            v, m = torch.ops.riab.gp_predict_var(part, wts, sq, al, linv_t, self.n_samples, inv, ws, True)
            if len(pieces) == 1:
                mean, var = m, v
                break
            if mean is None:
                mean = torch.empty((T, D, B), dtype=torch.float32, device=dev)
                var = torch.empty((T, B), dtype=torch.float32, device=dev)
            mean[t0:t1, :, c0:c1] = m
            var[t0:t1, c0:c1] = v
        if mean is None:      # T = 0
            mean = torch.empty((T, D, B), dtype=torch.float32, device=dev)
            var = torch.empty((T, B), dtype=torch.float32, device=dev)
        return mean, torch.sqrt(var)

    def decode_tensor(self, t_start=None, t_end=None, return_std=False, max_workspace_bytes=2 ** 28):
        """The decoded target of the history rows `get_history_slice(t_start, t_end)` (both None: every row): float32
        `[T][D][Bp]` on the device; return_std=True: (that, the predictive std float32 `[T][Bp]`), as `predict_tensor`."""
        agent, pieces = self._pieces_of_rates(t_start, t_end)
        if not return_std:
            return self._joined(agent, [self.predict_tensor(views) for views in pieces])
        parts = [self.predict_tensor(views, True, max_workspace_bytes) for views in pieces]
        if not parts:
            return self._joined(agent, []), torch.empty((0, agent._Bp), dtype=torch.float32, device=agent._device)
        return self._joined(agent, [m for m, _ in parts]), self._joined(agent, [s for _, s in parts])

    def decode(self, t_start=None, t_end=None, return_std=False, max_workspace_bytes=2 ** 28):
        """`decode_tensor` on the host: NumPy (T, B, D), or (T, D) for one agent; return_std=True: (that, std (T, B) or (T,))."""
        if not return_std:
            return super().decode(t_start, t_end)
        agent = self._populations()[0].Agent
        mean, std = self.decode_tensor(t_start, t_end, True, max_workspace_bytes)
        m, s = mean[:, :, :agent._B].permute(0, 2, 1).cpu().numpy(), std[:, :agent._B].cpu().numpy()
        return (m[:, 0], s[:, 0]) if agent._B == 1 else (m, s)


def kernel_matrix(A, B, length_scale):
    """RBF kernel of two float64 sample matrices (S, n), (N, n) -> (S, N), in the GEMM form clamped at 0."""
    d2 = (A * A).sum(dim=1)[:, None] + (B * B).sum(dim=1)[None, :] - 2.0 * (A @ B.T)
    return torch.exp(d2.clamp_(min=0.0).mul_(-1.0 / (2.0 * float(length_scale) ** 2)))


def _gather(hist, rows, agents, take):
    """take(chunk, local rows, agents) of every chunk of `hist` that holds one of the global `rows` (ascending), joined"""
    parts, base = [], 0
    for chunk, filled in zip(hist.chunks, hist.filled):
        sel = (rows >= base) & (rows < base + filled)
        if bool(sel.any()):
            parts.append(take(chunk, rows[sel] - base, agents[sel]))
        base += filled
    return torch.cat(parts, dim=0)


def fit_gp_decoder(populations, target="pos", t_start=None, t_end=None, stride=1, alpha=0.01, length_scale=None,
                   max_samples=4096, samples=None):
    """A `GPDecoder` from the populations' recorded rates to the agent's recorded target.  Rows and populations as
    `fit_linear_decoder`.  The training set is `select_samples(R, B, max_samples)` over the R rows start:stop:stride and
    the B agents (all of them when R B <= max_samples: one agent and the reference's `[::5]` is exactly sklearn's set), or
    `samples=(rows, agents)`: indices into the R selected rows and agent numbers (put in time-major order, duplicates
    removed: two identical samples would be two identical rows of K).  Candidates whose target is not finite are
    dropped and counted (`n_dropped`); a training rate that is not finite raises.  length_scale=None: sqrt(n_total / 20)."""
    if target not in TARGETS:
        raise ValueError(f"target must be one of {sorted(TARGETS)}, got {target!r}")
    if int(stride) < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    if isinstance(max_samples, bool) or int(max_samples) != max_samples or not 1 <= int(max_samples) <= MAX_SAMPLES:
        raise ValueError(f"max_samples must be an integer in 1..{MAX_SAMPLES}, got {max_samples}")
    populations, agent = _check_populations(populations)
    widths = [int(p.n) for p in populations]
    ell = _check_hyper(alpha, length_scale, sum(widths))
    start, stop = _rows(agent, populations, t_start, t_end)
    R, B, dev = len(range(start, stop, int(stride))), int(agent._B), agent._device
    if samples is None:
        ridx, agents = select_samples(R, B, int(max_samples))
    else:
        ridx, agents = (np.asarray(s, dtype=np.int64).reshape(-1) for s in samples)
        if len(ridx) != len(agents) or len(ridx) > MAX_SAMPLES:
            raise ValueError(f"samples must be (rows, agents) of equal length <= {MAX_SAMPLES}")
        if len(ridx) and (ridx.min() < 0 or ridx.max() >= R or agents.min() < 0 or agents.max() >= B):
            raise ValueError(f"samples must index the {R} selected rows and the {B} agents")
        flat = np.unique(ridx * B + agents)     # time-major, and a pair given twice is taken once, as the rule does
        ridx, agents = flat // B, flat % B
    if len(ridx) == 0:
        raise ValueError("no training sample: the rows asked for are empty")
    rows_d = torch.from_numpy(start + ridx * int(stride)).to(dev)
    agents_d = torch.from_numpy(agents).to(dev)
    trows = torch.tensor(TARGETS[target], dtype=torch.int64, device=dev)
    y = _gather(agent._hist, rows_d, agents_d, lambda c, r, b: c[r[:, None], trows[None, :], b[:, None]])     # (S, D) fp32
    keep = torch.isfinite(y).all(dim=1)
    n_dropped = int((~keep).sum().item())
    rows_d, agents_d, y = rows_d[keep], agents_d[keep], y[keep]
    if len(rows_d) == 0:
        raise ValueError("no training sample is left: every candidate's target is not finite")
    X = torch.cat([_gather(p._hist_fr, rows_d, agents_d, lambda c, r, b: c[r, :, b]) for p in populations], dim=1)   # (N, n)
    return GPDecoder.from_samples(X.to(torch.float64), y.to(torch.float64), ell, alpha, widths=widths, target=target,
                                  populations=populations, train_rows=rows_d, train_agents=agents_d, n_dropped=n_dropped)
