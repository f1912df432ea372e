"""Bayesian (Poisson maximum-likelihood) position decoding from spikes, fitted and run where the history lives.

The decoder of the place-cell literature: the spike counts k_c of the cells in a time window of duration tau = W dt are set
against the cells' tuning curves f_cj over J position bins with centres x_j, and under independent Poisson firing the log
posterior of bin j is

    l_j = sum_c k_c log max(f_cj, floor) + log prior_j - tau sum_c max(f_cj, floor)

(`rate_floor` keeps a silent cell from vetoing a bin).  The tuning curves come from `_ratemap.rate_map_tensors` over the fit
rows (tuning="history": rates, or spikes / dt) or from `get_state_tensor(evaluate_at="all")` on the environment's own grid
(tuning="groundtruth"); the tables are built in float64 with torch on the device and stored as float32.  The decode walks
the spike history's chunks: windows of W > 1 rows are counted by `torch.ops.riab.history_window_counts` across chunk
boundaries, and every (window, agent) sample goes through `torch.ops.riab.bayes_decode` (csrc/riab_bayes.hip): one fused
kernel on the fp32 matrix cores with a running softmax that never writes the (samples x J) log posterior to memory.  Per
sample it returns the posterior mean, the MAP bin's centre, the log evidence and the MAP probability.

`BayesianDecoder.with_continuity()` adds the continuity prior of the literature (Zhang et al. 1998): `BayesianFilter` carries
the posterior of a window to the next through a Gaussian step over the admissible bins, as a causal forward filter.  The
likelihood of a batch of windows is `torch.ops.riab.feedforward` on the same tables, the scan over the windows
`torch.ops.riab.bayes_filter` (csrc/riab_bayes_filter.hip): two kernels per window issued by one native call.

`BayesianFilter.smoothed()` puts a backward pass behind that filter (`BayesianSmoother`): the history is a recorded run, so
window t can be decoded from every window of the run, p(x_t | k_1..k_T).  The forward pass keeps the log posterior of every
window (`torch.ops.riab.bayes_filter_keep`), the backward scan is `torch.ops.riab.bayes_smooth` (csrc/riab_bayes_smooth.hip)."""
import numpy as np
import torch

from . import _lib as _L
from . import ops as _ops  # noqa: F401  (registers torch.ops.riab.bayes_decode / history_window_counts)
from . import utils
from ._decoder import MAX_POPULATIONS, HistoryDecoder, _check_populations, _max_rows, _rows
from ._ratemap import history_pieces, rate_map_tensors

MAX_BINS = _L.RATEMAP_MAX_BINS
MAX_WINDOW = _L.BAYES_MAX_WINDOW
OUT_ROWS = {"mean": (0, 1), "map": (2, 3), "log_evidence": (4,), "map_probability": (5,)}


def window_pieces(filled, start, stop, window, max_rows=None):
    """The windows of `window` consecutive rows of [start, stop) over several histories of the same steps: (n_windows,
    [(first rows, length, row0)]) where the pieces are `history_pieces` of the rows [start, start + n_windows window) —
    each lies in ONE chunk of every history — and `row0` is the piece's first row counted from `start`, so that its row r
    belongs to window (row0 + r) // window.  Trailing rows that do not fill a window are dropped."""
    start, stop, window = int(start), int(stop), int(window)
    if not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"window must be 1..{MAX_WINDOW} rows, got {window}")
    n_windows = max(0, stop - start) // window
    end = start + n_windows * window
    out, g = [], start
    for first, length in (history_pieces(filled, start, end, 1, max_rows) if n_windows else []):
        out.append((first, length, g - start))
        g += length
    return n_windows, out


def window_centre_rows(start, n_windows, window):
    """The history row at the centre of every window: start + w window + window // 2, an int64 array."""
    return int(start) + np.arange(int(n_windows), dtype=np.int64) * int(window) + int(window) // 2


def grid_centres(extent, dx):
    """Bin centres float64 (2, ny nx) of the maps `rate_map_tensors` returns over `extent` at bins `dx` wide, from the same
    edges and in the maps' flattening: row-major over (ny, nx) with the first row the TOP of the room.  -> (centres, ny, nx)"""
    ex, ey = utils.histogram_bin_edges(extent, dx)
    nx, ny = len(ex) - 1, len(ey) - 1
    if nx < 1 or ny < 1:
        raise ValueError("the grid has no bins")
    cx, cy = 0.5 * (ex[:-1] + ex[1:]), 0.5 * (ey[:-1] + ey[1:])
    return np.stack((np.tile(cx, ny), np.repeat(cy[::-1], nx))), ny, nx


class BayesianDecoder(HistoryDecoder):
    """A fitted Poisson maximum-likelihood decoder.  `log_rates`: one float32 (n_l, Jp) table log max(f, floor) per
    population; `S` float32 (Jp,) = sum_c max(f_cj, floor); `log_prior` float32 (Jp,), -inf for a bin that is not admissible
    (never visited, or padding); `centres` float32 (2, Jp); Jp = `n_bins` rounded up to 32.  All on the fit's device."""

    target = "pos"

    def __init__(self, log_rates, S, log_prior, centres, n_bins, dt, window=1, populations=None, grid_shape=None,
                 tuning="history", prior="uniform", rate_floor=1e-2, bin_width=None):
        self.log_rates, self.S, self.log_prior, self.centres = list(log_rates), S, log_prior, centres
        self.n_bins, self.dt = int(n_bins), float(dt)
        self.widths = [int(t.shape[0]) for t in self.log_rates]
        self.window = _check_window(window)
        self.populations = None if populations is None else list(populations)
        self.grid_shape, self.tuning, self.prior, self.rate_floor = grid_shape, tuning, prior, float(rate_floor)
        self.bin_width = None if bin_width is None else float(bin_width)   # the side of the (square) bins at fit time

    @classmethod
    def from_tuning(cls, tuning_curves, centres, dt, admissible=None, prior_weights=None, rate_floor=1e-2, **kw):
        """The tables from bare tuning curves: a list of float64 (n_l, J) tensors (Hz) on one device, `centres` float64
        (2, J), `admissible` bool (J,) or None (every bin), `prior_weights` float64 (J,) of non-negative weights or None
        (uniform over the admissible bins); the prior is normalised here."""
        tuning_curves = list(tuning_curves)
        if not 1 <= len(tuning_curves) <= MAX_POPULATIONS:
            raise ValueError(f"a decoder takes 1..{MAX_POPULATIONS} populations, got {len(tuning_curves)}")
        dev = tuning_curves[0].device
        J = int(tuning_curves[0].shape[1])
        if not 1 <= J <= MAX_BINS:
            raise ValueError(f"a Bayesian decoder takes 1..{MAX_BINS} position bins, got {J}: use larger bins")
        if not float(rate_floor) > 0:
            raise ValueError(f"rate_floor must be positive, got {rate_floor}")
        Jp = (J + 31) // 32 * 32
        ok = torch.ones(J, dtype=torch.bool, device=dev) if admissible is None else admissible.to(dev).reshape(J).bool()
        w = ok.to(torch.float64)
        if prior_weights is not None:
            w = w * prior_weights.to(dev).reshape(J).to(torch.float64)
        logp = torch.full((Jp,), -float("inf"), dtype=torch.float64, device=dev)
        logp[:J] = torch.where(w > 0, torch.log(w / w.sum()), -float("inf"))
        S = torch.zeros(Jp, dtype=torch.float64, device=dev)
        tables = []
        for f in tuning_curves:
            if f.dtype != torch.float64 or f.dim() != 2 or int(f.shape[1]) != J or f.device != dev:
                raise ValueError("tuning curves must be float64 tensors (n_l, J) on one device")
            F = f.clamp(min=float(rate_floor))
            S[:J] += F.sum(dim=0)
            L = torch.zeros((int(f.shape[0]), Jp), dtype=torch.float32, device=dev)
            L[:, :J] = torch.log(F).to(torch.float32)
            tables.append(L)
        c = torch.zeros((2, Jp), dtype=torch.float32, device=dev)
        c[:, :J] = centres.to(dev).to(torch.float32)
        return cls(tables, S.to(torch.float32), logp.to(torch.float32), c, J, dt, rate_floor=rate_floor, **kw)

    def bias(self, window=None):
        """bias_j = log prior_j - tau S_j of windows of `window` rows (tau = window dt), float32 (Jp,): formed in float64
        from the stored float32 tables."""
        tau = _check_window(self.window if window is None else window) * self.dt
        return (self.log_prior.to(torch.float64) - tau * self.S.to(torch.float64)).to(torch.float32)

    # ---- running the decoder ------------------------------------------------------------------------------------------
    def _populations(self):
        if self.populations is None:
            raise ValueError("this decoder was built from bare tuning curves: it has no populations to read spikes from")
        return self.populations

    def decode_inputs_tensor(self, inputs, window=1, block_tiles=0):
        """The six output rows of inputs that are not in a history: a list of uint8 count tensors or float32 rate tensors
        `[T][n_l][Bp]`, one per population, each sample a window of `window` rows' duration -> float32 `[T][6][Bp]`."""
        inputs = list(inputs)
        if len(inputs) != len(self.widths) or any(int(x.shape[1]) != w for x, w in zip(inputs, self.widths)):
            raise ValueError(f"this decoder takes {len(self.widths)} input tensors (T, n_l, Bp) of widths {self.widths}")
        tau = _check_window(window) * self.dt
        return torch.ops.riab.bayes_decode(inputs, self.log_rates, self.bias(window), self.centres, self.n_bins, tau,
                                           int(block_tiles))

    def _windows(self, t_start, t_end, window, inputs):
        """(agent, histories read, start, window, n_windows, pieces) of a decode"""
        window = _check_window(self.window if window is None else window)
        if inputs not in ("spikes", "rates"):
            raise ValueError(f"inputs must be 'spikes' or 'rates', got {inputs!r}")
        if inputs == "rates" and window != 1:
            raise ValueError("inputs='rates' decodes single rows (k = dt * rate): window must be 1")
        pops = self._populations()
        agent = pops[0].Agent
        start, stop = _rows(agent, pops, t_start, t_end)
        hists = [_spike_history(p, stop) for p in pops] if inputs == "spikes" else [p._hist_fr for p in pops]
        n_windows, pieces = window_pieces([h.filled for h in hists], start, stop, window, _max_rows(agent._Bp))
        return agent, hists, start, window, n_windows, pieces

    def decode_all_tensor(self, t_start=None, t_end=None, window=None, inputs="spikes"):
        """Every output of the windows of `window` (None: the fitted one) consecutive rows of the history rows
        `get_history_slice(t_start, t_end)` (both None: every row), trailing rows that do not fill a window dropped:
        float32 `[T'][6][Bp]` on the device, rows = posterior mean x, y; MAP centre x, y; log evidence; MAP probability.
        inputs="spikes": the recorded spikes, counted per window; "rates": k = dt * rate of single rows (window 1)."""
        agent, hists, _start, window, n_windows, pieces = self._windows(t_start, t_end, window, inputs)
        if n_windows == 0:
            return torch.empty((0, _L.BAYES_OUT_ROWS, agent._Bp), dtype=torch.float32, device=agent._device)
        if window == 1:      # the rows are the samples: read in place
            parts = [self.decode_inputs_tensor([h.chunks[c][r:r + length] for h, (c, r) in zip(hists, first)], 1)
                     for first, length, _row0 in pieces]
            return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        counts = [torch.zeros((n_windows, w, agent._Bp), dtype=torch.uint8, device=agent._device) for w in self.widths]
        for first, length, row0 in pieces:
            for h, (c, r), cnt in zip(hists, first, counts):
                torch.ops.riab.history_window_counts(h.chunks[c][r:r + length], row0, window, cnt)
        step = _max_rows(agent._Bp)
        parts = [self.decode_inputs_tensor([cnt[o:o + step] for cnt in counts], window) for o in range(0, n_windows, step)]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    def decode_tensor(self, t_start=None, t_end=None, window=None, inputs="spikes", estimate="mean"):
        """The decoded position of every window: float32 `[T'][2][Bp]`, the posterior mean (estimate="mean") or the MAP
        bin's centre ("map")."""
        if estimate not in ("mean", "map"):
            raise ValueError(f"estimate must be 'mean' or 'map', got {estimate!r}")
        lo = OUT_ROWS[estimate][0]
        return self.decode_all_tensor(t_start, t_end, window, inputs)[:, lo:lo + 2]

    def _target_tensor(self, t_start, t_end):
        """The recorded position at the centre row of every window (of the fitted `window`)."""
        pops = self._populations()
        agent, window = pops[0].Agent, self.window
        start, stop = _rows(agent, pops, t_start, t_end)
        n_windows = (stop - start) // window
        h = agent._hist
        rows = [_L.H_POS_X, _L.H_POS_Y]
        if n_windows == 0:
            return self._joined(agent, [])
        first_row = int(window_centre_rows(start, n_windows, window)[0])
        parts = [h.chunks[c][r:r + length:window][:, rows]
                 for ((c, r),), length in history_pieces([h.filled], first_row, start + n_windows * window, window)]
        return self._joined(agent, parts)


    def with_continuity(self, sigma=None, mixing=1e-3):
        """This decoder with a continuity prior (`BayesianFilter`): the posterior of a window is carried to the next through
        a Gaussian step of standard deviation `sigma` (m; None: agent.speed_mean x window x dt, floored at half a bin) over
        the admissible bins, mixed with a share `mixing` in (0, 1] of the fitted prior."""
        return BayesianFilter(self, sigma, mixing)


FILTER_MAX_RADIUS = _L.BAYES_FILTER_MAX_RADIUS
FILTER_LOGLIK_BYTES = 1 << 28     # the (windows, Jp, Bp) float32 log likelihood of one native call stays under this


def continuity_taps(sigma, dx):
    """(R, g): R = max(1, ceil(3 sigma / dx)) and the taps g[d] ~ exp(-(d dx)^2 / (2 sigma^2)), d = -R..R, float64 (2R + 1,)
    normalised to sum 1.  ValueError for sigma <= 0 and for R > 16 (the step is not truncated silently)."""
    sigma, dx = float(sigma), float(dx)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    if not dx > 0:
        raise ValueError(f"the bin width must be positive, got {dx}")
    R = max(1, int(np.ceil(3.0 * sigma / dx)))
    if R > FILTER_MAX_RADIUS:
        raise ValueError(f"sigma = {sigma} m reaches over {R} bins of width {dx} m, the filter takes {FILTER_MAX_RADIUS}: use a "
                         "smaller sigma or larger bins")
    d = np.arange(-R, R + 1, dtype=np.float64) * dx
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    return R, g / g.sum()


class BayesianFilter(HistoryDecoder):
    """A `BayesianDecoder` with a continuity prior, run as a causal forward filter over consecutive windows (the two-step
    reconstruction of Zhang et al. 1998).  With p_{t-1} the posterior of the window before,

        pred_t(j) = (1 - mixing) ok_j sum_j' G(j - j') p_{t-1}(j') / norm_j' + mixing prior_j
        l_t(j)    = sum_c k_c L_cj - tau S_j + log pred_t(j)

    where G is a separable Gaussian step of `radius` bins either way restricted to the admissible bins and normalised per
    source bin (norm_j' = sum_j G(j - j') ok_j); pred = prior on the first window of a call, on a restarted window and after
    a window that came out as NaN.  `taps` float64 (2 radius + 1,); `prior`, `inv_norm` float32 (Jp,) on the device."""

    target = "pos"

    def __init__(self, decoder, sigma=None, mixing=1e-3):
        if decoder.grid_shape is None or decoder.bin_width is None:
            raise ValueError("a continuity prior needs the decoder's grid (grid_shape and bin_width): a decoder built from bare "
                             "tuning curves has none")
        ny, nx = (int(v) for v in decoder.grid_shape)
        if ny * nx != decoder.n_bins:
            raise ValueError(f"the grid {ny} x {nx} does not hold the decoder's {decoder.n_bins} bins")
        if not 0.0 < float(mixing) <= 1.0:
            raise ValueError(f"mixing must lie in (0, 1], got {mixing}")
        dx = decoder.bin_width
        if sigma is None:
            agent = decoder._populations()[0].Agent
            sigma = max(float(agent.speed_mean) * decoder.window * decoder.dt, 0.5 * dx)
        self.radius, self.taps = continuity_taps(sigma, dx)
        self.decoder, self.sigma, self.mixing, self.grid_shape = decoder, float(sigma), float(mixing), (ny, nx)
        self.window = decoder.window
        J, Jp, dev, R = decoder.n_bins, int(decoder.S.shape[0]), decoder.S.device, self.radius
        logp = decoder.log_prior.to(torch.float64)
        ok = torch.isfinite(logp[:J]).reshape(ny, nx)
        g = torch.from_numpy(self.taps).to(dev)
        # norm_j' = sum_j G(j - j') ok_j: the two blurs of the mask, taps that leave the grid dropped
        along_x = torch.zeros((ny, nx), dtype=torch.float64, device=dev)
        for d in range(-R, R + 1):
            lo, hi = max(0, -d), min(nx, nx - d)
            if lo < hi:
                along_x[:, lo:hi] += g[d + R] * ok[:, lo + d:hi + d]
        norm = torch.zeros((ny, nx), dtype=torch.float64, device=dev)
        for d in range(-R, R + 1):
            lo, hi = max(0, -d), min(ny, ny - d)
            if lo < hi:
                norm[lo:hi] += g[d + R] * along_x[lo + d:hi + d]
        inv = torch.zeros(Jp, dtype=torch.float64, device=dev)
        inv[:J] = torch.where(ok, 1.0 / norm, torch.zeros_like(norm)).reshape(-1)
        self.inv_norm = inv.to(torch.float32)
        self.prior = torch.exp(logp).to(torch.float32)          # 0 where the bin is not admissible, and in the padding
        self._taps32 = [float(np.float32(v)) for v in self.taps[R:]]
        self._max_windows_per_call = None

    def _populations(self):
        return self.decoder._populations()

    def _lik_bias(self, window):
        """-tau S_j, -inf in the bins that are not admissible and in the padding: float32 (Jp,), formed in float64"""
        dec = self.decoder
        tau = _check_window(window) * dec.dt
        b = -tau * dec.S.to(torch.float64)
        return torch.where(torch.isfinite(dec.log_prior), b, torch.full_like(b, -float("inf"))).to(torch.float32)

    def filter_inputs_tensor(self, inputs, window=1, restart=None, state=None):
        """The filter over inputs that are not in a history, as `BayesianDecoder.decode_inputs_tensor` takes them: a list of
        uint8 count or float32 rate tensors `[T][n_l][Bp]`, consecutive windows -> (float32 `[T][6][Bp]`, state).  `restart`:
        bool or uint8 tensor (T, Bp) or None.  `state`: None starts a new run; the state returned continues one."""
        dec = self.decoder
        inputs = list(inputs)
        if len(inputs) != len(dec.widths) or any(int(x.shape[1]) != w for x, w in zip(inputs, dec.widths)):
            raise ValueError(f"this decoder takes {len(dec.widths)} input tensors (T, n_l, Bp) of widths {dec.widths}")
        T, Bp = int(inputs[0].shape[0]), int(inputs[0].shape[2])
        dev, Jp = inputs[0].device, int(dec.S.shape[0])
        tau = _check_window(window) * dec.dt
        out = torch.empty((T, _L.BAYES_OUT_ROWS, Bp), dtype=torch.float32, device=dev)
        first = state is None
        if first:
            state = (torch.empty((Jp, Bp), dtype=torch.float32, device=dev), torch.empty((Jp, Bp), dtype=torch.float32, device=dev),
                     torch.empty(_ops.bayes_filter_workspace_floats(Jp, Bp), dtype=torch.float32, device=dev))
        bias = self._lik_bias(window)
        step = max(1, min(65535, FILTER_LOGLIK_BYTES // (4 * Jp * Bp)))
        if self._max_windows_per_call is not None:
            step = max(1, min(step, int(self._max_windows_per_call)))
        ny, nx = self.grid_shape
        for o in range(0, T, step):
            # the likelihood stage: riab_feedforward's store-epilogue GEMM on float32 counts (k = tau x rate for rates)
            x = [t[o:o + step].to(torch.float32) if t.dtype == torch.uint8 else t[o:o + step] * float(np.float32(tau)) for t in inputs]
            loglik = torch.ops.riab.feedforward(x, dec.log_rates, bias, _L.ACTIVATIONS["linear"], [0.0, 0.0, 0.0, 0.0])
            torch.ops.riab.bayes_filter(loglik, dec.n_bins, ny, nx, self._taps32, self.mixing, self.prior, self.inv_norm,
                                        dec.centres, None if restart is None else restart[o:o + step].contiguous(),
                                        first and o == 0, state[0], state[1], state[2], out[o:o + step])
        return out, state

    def decode_all_tensor(self, t_start=None, t_end=None, window=None, inputs="spikes", restart=None):
        """Every output of the consecutive windows `BayesianDecoder.decode_all_tensor` decodes (the same rows, the same
        counts), filtered forward from the first: float32 `[T'][6][Bp]`, rows as there except that row 4 is the predictive log
        likelihood log p(k_t | k_<t).  `restart`: a bool tensor or array (T', B) — or (T', Bp) —; a set flag starts that
        agent's filter afresh at that window (episode ends, the edges of a ReplayAgent's history["replay"])."""
        agent, window, n_windows, flags, runs = self._runs(t_start, t_end, window, inputs, restart)
        if n_windows == 0:
            return torch.empty((0, _L.BAYES_OUT_ROWS, agent._Bp), dtype=torch.float32, device=agent._device)
        parts, state = [], None
        for x, w0, n in runs:
            out, state = self.filter_inputs_tensor(x, window, None if flags is None else flags[w0:w0 + n], state)
            parts.append(out)
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    def _runs(self, t_start, t_end, window, inputs, restart):
        """(agent, window, n_windows, restart flags uint8 (T', Bp) or None, [(inputs of consecutive windows, their first
        window, how many)]) of a decode: the windows `BayesianDecoder.decode_all_tensor` decodes, piece by piece"""
        dec = self.decoder
        agent, hists, _start, window, n_windows, pieces = dec._windows(t_start, t_end, window, inputs)
        dev, Bp = agent._device, agent._Bp
        if n_windows == 0:
            return agent, window, 0, None, []
        flags = None
        if restart is not None:
            r = torch.as_tensor(np.asarray(restart) if not torch.is_tensor(restart) else restart).to(dev)
            if r.dim() != 2 or int(r.shape[0]) != n_windows or int(r.shape[1]) not in (agent._B, Bp):
                raise ValueError(f"restart must be ({n_windows}, {agent._B}): one flag per window and agent, got {tuple(r.shape)}")
            flags = torch.zeros((n_windows, Bp), dtype=torch.uint8, device=dev)
            flags[:, :int(r.shape[1])] = r != 0
        if window == 1:      # the rows are the samples: read in place, piece by piece
            runs = [([h.chunks[c][r:r + length] for h, (c, r) in zip(hists, first)], row0, length) for first, length, row0 in pieces]
        else:
            counts = [torch.zeros((n_windows, w, Bp), dtype=torch.uint8, device=dev) for w in dec.widths]
            for first, length, row0 in pieces:
                for h, (c, r), cnt in zip(hists, first, counts):
                    torch.ops.riab.history_window_counts(h.chunks[c][r:r + length], row0, window, cnt)
            runs = [(counts, 0, n_windows)]
        return agent, window, n_windows, flags, runs

    def decode_tensor(self, t_start=None, t_end=None, window=None, inputs="spikes", estimate="mean", restart=None):
        """The filtered position of every window: float32 `[T'][2][Bp]`, the posterior mean (estimate="mean") or the MAP
        bin's centre ("map")."""
        if estimate not in ("mean", "map"):
            raise ValueError(f"estimate must be 'mean' or 'map', got {estimate!r}")
        lo = OUT_ROWS[estimate][0]
        return self.decode_all_tensor(t_start, t_end, window, inputs, restart)[:, lo:lo + 2]

    def _target_tensor(self, t_start, t_end):
        return self.decoder._target_tensor(t_start, t_end)

    def smoothed(self, max_state_bytes=2 ** 31):
        """This filter followed by a backward pass over the recorded run (`BayesianSmoother`): every window is decoded from
        ALL the windows of its run, not only from those up to it.  `max_state_bytes`: what the smoother may keep on the
        device between the two passes."""
        return BayesianSmoother(self, max_state_bytes)


class BayesianSmoother(HistoryDecoder):
    """A `BayesianFilter` run forward and then backward over a recorded run (forward-backward smoothing): the posterior of
    window t given every window of the run, p(x_t | k_1..k_T), where the filter gives p(x_t | k_1..k_t).  The forward pass is
    the filter's with the log posterior l_t of every window kept (`torch.ops.riab.bayes_filter_keep`); the backward pass
    (`torch.ops.riab.bayes_smooth`, csrc/riab_bayes_smooth.hip: two kernels per window issued by one native call per batch)
    carries beta_t(j) ~ p(k_t+1..k_T | x_t = j) from the last window to the first and never crosses a restart or a NaN window,
    as the filter never does.  Rows of the outputs as the filter's; row 4 is the filter's, log p(k_t | k_<t).

    Between the passes the l of every window stays on the device, float32 (T', Jp, Bp), and so does the log likelihood when
    both fit in `max_state_bytes`; when they do not, the log likelihood is recomputed batch by batch on the way back, and when
    l alone does not fit either, the agents are run in blocks of a multiple of 64 columns that do.  Columns are independent:
    the blocks have the bits of one block."""

    target = "pos"

    def __init__(self, filt, max_state_bytes=2 ** 31):
        if isinstance(max_state_bytes, bool) or int(max_state_bytes) != max_state_bytes or int(max_state_bytes) < 1:
            raise ValueError(f"max_state_bytes must be a positive integer, got {max_state_bytes}")
        self.filter, self.decoder, self.max_state_bytes = filt, filt.decoder, int(max_state_bytes)
        self.window = filt.window

    def _populations(self):
        return self.decoder._populations()

    def _target_tensor(self, t_start, t_end):
        return self.decoder._target_tensor(t_start, t_end)

    def column_blocks(self, n_windows, Bp):
        """(whether the log likelihood is kept, [(first column, end)]) of a run of `n_windows` windows over `Bp` columns"""
        Jp = int(self.decoder.S.shape[0])
        per_column = 4 * int(n_windows) * Jp                     # the l of every window, one column
        if 2 * per_column * Bp <= self.max_state_bytes:
            return True, [(0, Bp)]
        if per_column * Bp <= self.max_state_bytes:
            return False, [(0, Bp)]
        cols = self.max_state_bytes // per_column // 64 * 64
        if cols < 64:
            raise ValueError(f"smoothing {n_windows} windows over {Jp} bins keeps {per_column * min(64, Bp)} bytes for a block of "
                             f"{min(64, Bp)} agents, max_state_bytes is {self.max_state_bytes}: raise it, or smooth fewer "
                             "windows at a time")
        return False, [(c, min(c + cols, Bp)) for c in range(0, Bp, cols)]

    def _smooth_block(self, runs, window, flags, keep_loglik):
        """Forward, then backward, over the runs' windows for the columns the tensors hold -> float32 (T', 6, B)"""
        filt, dec = self.filter, self.decoder
        dev, B, Jp = runs[0][0][0].device, int(runs[0][0][0].shape[2]), int(dec.S.shape[0])
        tau = np.float32(_check_window(window) * dec.dt)
        bias = filt._lik_bias(window)
        ny, nx = filt.grid_shape
        tables = (filt._taps32, filt.mixing, filt.prior, filt.inv_norm, dec.centres)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        step = max(1, min(65535, FILTER_LOGLIK_BYTES // (4 * Jp * B)))
        if filt._max_windows_per_call is not None:
            step = max(1, min(step, int(filt._max_windows_per_call)))

        def loglik_of(xs, o):
            x = [t[o:o + step].to(torch.float32) if t.dtype == torch.uint8 else t[o:o + step] * float(tau) for t in xs]
            return torch.ops.riab.feedforward(x, dec.log_rates, bias, _L.ACTIVATIONS["linear"], [0.0, 0.0, 0.0, 0.0])

        tmp, ws = new(Jp, B), new(_ops.bayes_filter_workspace_floats(Jp, B))
        batches = []                                             # (inputs, offset, l, the filter's outputs, loglik, flags)
        for xs, w0, n in runs:
            for o in range(0, n, step):
                loglik = loglik_of(xs, o)
                m = int(loglik.shape[0])
                ells, filtered = new(m, Jp, B), new(m, _L.BAYES_OUT_ROWS, B)
                fl = None if flags is None else flags[w0 + o:w0 + o + m]
                torch.ops.riab.bayes_filter_keep(loglik, dec.n_bins, ny, nx, *tables, fl, not batches, ells, tmp, ws, filtered)
                batches.append((xs, o, ells, filtered, loglik if keep_loglik else None, fl))
        beta, ws = new(Jp, B), new(_ops.bayes_smooth_workspace_floats(Jp, B))
        outs = [None] * len(batches)
        for i in reversed(range(len(batches))):
            xs, o, ells, filtered, loglik, fl = batches[i]
            batches[i] = None
            outs[i] = torch.empty_like(filtered)
            torch.ops.riab.bayes_smooth(loglik_of(xs, o) if loglik is None else loglik, ells, filtered, dec.n_bins, ny, nx, *tables,
                                        fl, i == len(outs) - 1, beta, tmp, ws, outs[i])
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _smooth_runs(self, runs, window, flags, n_windows, Bp):
        keep, blocks = self.column_blocks(n_windows, Bp)
        if len(blocks) == 1:
            return self._smooth_block(runs, window, flags, keep)
        out = torch.empty((n_windows, _L.BAYES_OUT_ROWS, Bp), dtype=torch.float32, device=runs[0][0][0].device)
        for c0, c1 in blocks:
            part = [([x[:, :, c0:c1].contiguous() for x in xs], w0, n) for xs, w0, n in runs]
            out[:, :, c0:c1] = self._smooth_block(part, window, None if flags is None else flags[:, c0:c1].contiguous(), keep)
        return out

    def smooth_inputs_tensor(self, inputs, window=1, restart=None):
        """The smoother over inputs that are not in a history, as `BayesianFilter.filter_inputs_tensor` takes them: a list of
        uint8 count or float32 rate tensors `[T][n_l][Bp]`, the consecutive windows of ONE run, all of it -> float32
        `[T][6][Bp]`.  `restart`: bool or uint8 tensor (T, Bp) or None."""
        dec = self.decoder
        inputs = list(inputs)
        if len(inputs) != len(dec.widths) or any(int(x.shape[1]) != w for x, w in zip(inputs, dec.widths)):
            raise ValueError(f"this decoder takes {len(dec.widths)} input tensors (T, n_l, Bp) of widths {dec.widths}")
        T, Bp = int(inputs[0].shape[0]), int(inputs[0].shape[2])
        if T == 0:
            return torch.empty((0, _L.BAYES_OUT_ROWS, Bp), dtype=torch.float32, device=inputs[0].device)
        flags = None
        if restart is not None:
            if tuple(restart.shape) != (T, Bp):
                raise ValueError(f"restart must be ({T}, {Bp}): one flag per window and column, got {tuple(restart.shape)}")
            flags = (restart != 0).to(torch.uint8).contiguous()
        return self._smooth_runs([(inputs, 0, T)], window, flags, T, Bp)

    def decode_all_tensor(self, t_start=None, t_end=None, window=None, inputs="spikes", restart=None):
        """Every output of the consecutive windows `BayesianFilter.decode_all_tensor` decodes (the same rows, the same counts,
        the same `restart`), smoothed over the whole run: float32 `[T'][6][Bp]`, rows 0-1 the smoothed posterior mean, 2-3
        the centre of the smoothed MAP bin, 4 the filter's log p(k_t | k_<t), 5 the smoothed MAP probability."""
        agent, window, n_windows, flags, runs = self.filter._runs(t_start, t_end, window, inputs, restart)
        if n_windows == 0:
            return torch.empty((0, _L.BAYES_OUT_ROWS, agent._Bp), dtype=torch.float32, device=agent._device)
        return self._smooth_runs(runs, window, flags, n_windows, agent._Bp)

    def decode_tensor(self, t_start=None, t_end=None, window=None, inputs="spikes", estimate="mean", restart=None):
        """The smoothed position of every window: float32 `[T'][2][Bp]`, the posterior mean (estimate="mean") or the MAP
        bin's centre ("map")."""
        if estimate not in ("mean", "map"):
            raise ValueError(f"estimate must be 'mean' or 'map', got {estimate!r}")
        lo = OUT_ROWS[estimate][0]
        return self.decode_all_tensor(t_start, t_end, window, inputs, restart)[:, lo:lo + 2]


def _check_window(window):
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= MAX_WINDOW:
        raise ValueError(f"window must be an integer in 1..{MAX_WINDOW} rows, got {window}")
    return int(window)


def _spike_history(p, stop):
    if not p.save_spikes or len(p._hist_sp) == 0:
        raise ValueError(f"{p.name}: no recorded spikes to decode from (update() with save_history and save_spikes on "
                         "fills the spike history)")
    if stop > len(p._hist_sp):
        raise ValueError(f"rows up to {stop} asked for, but {p.name}'s spike history has {len(p._hist_sp)} rows")
    return p._hist_sp


def fit_bayesian_decoder(populations, tuning="history", bin_size=0.05, t_start=None, t_end=None, spikes=False,
                         prior="uniform", rate_floor=1e-2, window=1):
    """A `BayesianDecoder` of the populations (1..8, of one Agent).  tuning="history": the tuning curves are the rate maps of
    the rows `get_history_slice(t_start, t_end)` (both None: every row) at bins `bin_size` wide — of the recorded rates, or
    with spikes=True of the recorded spikes divided by dt — and a bin never visited is not admissible.  tuning="groundtruth":
    `get_state_tensor(evaluate_at="all")` on the environment's own grid (Environment.dx; `bin_size` is not used), every bin
    admissible.  prior: "uniform" over the admissible bins or "occupancy" (the visits per bin; history tuning only).
    `rate_floor` (Hz): the least rate a tuning curve is given.  `window`: the rows per decoding window (1..255)."""
    if tuning not in ("history", "groundtruth"):
        raise ValueError(f"tuning must be 'history' or 'groundtruth', got {tuning!r}")
    if prior not in ("uniform", "occupancy"):
        raise ValueError(f"prior must be 'uniform' or 'occupancy', got {prior!r}")
    if prior == "occupancy" and tuning != "history":
        raise ValueError("prior='occupancy' needs tuning='history': ground-truth tuning has no visits to count")
    if not float(rate_floor) > 0:
        raise ValueError(f"rate_floor must be positive, got {rate_floor}")
    window = _check_window(window)
    populations, agent = _check_populations(populations)
    dev, dt = agent._device, float(agent.dt)
    if tuning == "groundtruth":
        env = agent.Environment
        shape = tuple(int(s) for s in env.discrete_coords.shape[:2])
        J = shape[0] * shape[1]
        if J > MAX_BINS:
            raise ValueError(f"the environment's grid has {J} bins, a Bayesian decoder takes 1..{MAX_BINS}: use a larger dx")
        curves = [p.get_state_tensor(evaluate_at="all")[:, :J].to(torch.float64) for p in populations]
        centres = torch.from_numpy(np.ascontiguousarray(np.asarray(env.flattened_discrete_coords, dtype=np.float64).T))
        return BayesianDecoder.from_tuning(curves, centres, dt, rate_floor=rate_floor, window=window, populations=populations,
                                           grid_shape=shape, tuning=tuning, prior=prior, bin_width=float(env.dx))
    centres, ny, nx = grid_centres(agent.Environment.extent, bin_size)
    if ny * nx > MAX_BINS:
        raise ValueError(f"bins of {bin_size} make a grid of {ny * nx} bins, a Bayesian decoder takes 1..{MAX_BINS}: use larger bins")
    start, stop = _rows(agent, populations, t_start, t_end)
    curves, zero, visits = [], None, None
    for p in populations:
        hist = _spike_history(p, stop) if spikes else p._hist_fr
        maps, zero, visits = rate_map_tensors(agent, hist, int(p.n), bin_size, start, stop, True)
        curves.append((maps / dt if spikes else maps).reshape(int(p.n), ny * nx))
    return BayesianDecoder.from_tuning(curves, torch.from_numpy(centres), dt, admissible=~zero.reshape(-1),
                                       prior_weights=visits.reshape(-1) if prior == "occupancy" else None,
                                       rate_floor=rate_floor, window=window, populations=populations, grid_shape=(ny, nx),
                                       tuning=tuning, prior=prior, bin_width=float(bin_size))
