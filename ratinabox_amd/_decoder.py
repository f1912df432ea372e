"""Linear (ridge) decoders fitted and run where the history lives.

The reference decodes position by copying `history["firingrate"]` and `history["pos"]` to the host and fitting
`sklearn.linear_model.Ridge` (tests/test_advanced.py::test_decoding_position, demos/decoding_position_example).  Here the
trajectory rows `[T][8][Bp]` and the populations' rows `[T][n][Bp]` sit in `DeviceHistory` chunks; this module walks the
chunks and hands each piece to `torch.ops.riab.history_moments` (csrc/riab_decoder.hip, float64 matrix cores), which adds
the moment matrix of z = [rates ; target ; 1] into one float64 (m, m) tensor: X^T X, X^T y, the column sums and the
sample count of every (step, agent) sample in one pass.  The ridge system is then solved once, in float64, with
torch.linalg on the same device; predictions go through the existing `riab_feedforward` many-row entry point.  Nothing
is stacked, concatenated or copied to the host on the way to the fit."""
import numpy as np
import torch

from . import _lib as _L
from . import ops as _ops  # noqa: F401  (registers torch.ops.riab.history_moments / feedforward)
from ._ratemap import MAX_QUADS, history_pieces

TARGETS = {"pos": (_L.H_POS_X, _L.H_POS_Y), "vel": (_L.H_VEL_X, _L.H_VEL_Y), "head_direction": (_L.H_HD_X, _L.H_HD_Y)}
MAX_POPULATIONS = 8


class MomentLayout:
    """What the rows and columns of a moment matrix mean: z = [widths[0] rates ; ... ; D target rows ; 1]."""

    def __init__(self, widths, target="pos", populations=None, n_dropped=None, rows=None):
        if target not in TARGETS:
            raise ValueError(f"target must be one of {sorted(TARGETS)}, got {target!r}")
        self.widths = [int(w) for w in widths]
        self.n = sum(self.widths)
        self.target = target
        self.target_rows = TARGETS[target]
        self.D = len(self.target_rows)
        self.m = self.n + self.D + 1
        self.populations = None if populations is None else list(populations)
        self.n_dropped = n_dropped   # int64 (1,) tensor on the moments' device, or None
        self.rows = rows             # (start, stop, stride) of the history rows, or None


def _settled(agent):
    agent._sync_plan()
    agent._settle_plan()
    agent._check_pipeline()


def _check_populations(populations, spikes=False):
    populations = list(populations)
    if spikes:
        raise NotImplementedError("spikes as decoder inputs are not built: the moments are taken of the rate history")
    if not 1 <= len(populations) <= MAX_POPULATIONS:
        raise ValueError(f"a decoder takes 1..{MAX_POPULATIONS} populations, got {len(populations)}")
    agent = populations[0].Agent
    if any(p.Agent is not agent for p in populations):
        raise ValueError("the populations of a decoder must belong to one Agent (their rows are samples of its trajectory)")
    return populations, agent


def _rows(agent, populations, t_start, t_end):
    """(start, stop) of the rows asked for, checked against every history."""
    _settled(agent)
    for p in populations:
        if len(p._hist_fr) == 0:
            raise ValueError(f"{p.name}: no recorded rates to decode from (update() with save_history on fills the history)")
    total = len(agent._hist)
    start, stop = 0, total
    if t_start is not None or t_end is not None:
        start, stop = agent._history_rows(t_start, t_end)
        if t_end is None:
            stop = total
    for p in populations:
        if stop > len(p._hist_fr) or stop > total:
            raise ValueError(f"rows [{start}, {stop}) asked for, but {p.name}'s history has {len(p._hist_fr)} rows and the "
                             f"trajectory's {total}: a decoder needs every population's rates at every row")
    return start, stop


def _max_rows(Bp):
    return max(1, MAX_QUADS // max(1, Bp // 4))


def history_moments_tensor(populations, target="pos", t_start=None, t_end=None, stride=1, spikes=False):
    """(M float64 (m, m) device tensor, MomentLayout): the sum of z z^T, z = [rates of populations[0] ; ... ; target ; 1],
    over every (step, agent) sample of every `stride`-th row of `Agent.get_history_slice(t_start, t_end)` (both None: the
    whole history).  Samples whose target is not finite (a ThetaSequenceAgent outside a sweep) are left out and counted
    in `layout.n_dropped`.  Moments are additive: the M of two shards or of two time windows may be summed.
    target: "pos", "vel" or "head_direction"."""
    if target not in TARGETS:
        raise ValueError(f"target must be one of {sorted(TARGETS)}, got {target!r}")
    if int(stride) < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    populations, agent = _check_populations(populations, spikes)
    start, stop = _rows(agent, populations, t_start, t_end)
    dev = agent._device
    n_dropped = torch.zeros(1, dtype=torch.int64, device=dev)
    layout = MomentLayout([p.n for p in populations], target, populations, n_dropped, (start, stop, int(stride)))
    M = torch.zeros((layout.m, layout.m), dtype=torch.float64, device=dev)
    hists = [agent._hist] + [p._hist_fr for p in populations]
    for first, length in history_pieces([h.filled for h in hists], start, stop, stride, _max_rows(agent._Bp)):
        views = [h.chunks[c][r:r + length] for h, (c, r) in zip(hists, first)]
        torch.ops.riab.history_moments(views[1:], views[0], list(layout.target_rows), int(stride), agent._B, M, n_dropped)
    return M, layout


class HistoryDecoder:
    """What every decoder fitted from the device history shares: the populations it reads, the trajectory rows it was
    fitted to, and `decode` / `error` on top of the subclass's `decode_tensor`.  A subclass sets `target` and provides
    `_populations()` (or raises: a decoder built from bare arrays has none) and `decode_tensor(t_start, t_end)` ->
    float32 `[T][D][Bp]`."""

    target = "pos"

    def _populations(self):
        raise NotImplementedError

    def decode_tensor(self, t_start=None, t_end=None):
        raise NotImplementedError

    def _pieces_of_rates(self, t_start, t_end):
        """(agent, [views of every population's rows, one list per piece lying in ONE chunk of each history])"""
        pops = self._populations()
        agent = pops[0].Agent
        start, stop = _rows(agent, pops, t_start, t_end)
        hists = [p._hist_fr for p in pops]
        return agent, [[h.chunks[c][r:r + length] for h, (c, r) in zip(hists, first)]
                       for first, length in history_pieces([h.filled for h in hists], start, stop, 1, _max_rows(agent._Bp))]

    def _joined(self, agent, parts):
        D = len(TARGETS[self.target])
        if not parts:
            return torch.empty((0, D, agent._Bp), dtype=torch.float32, device=agent._device)
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    def decode(self, t_start=None, t_end=None):
        """`decode_tensor` on the host: NumPy (T, B, D), or (T, D) for one agent."""
        agent = self._populations()[0].Agent
        a = self.decode_tensor(t_start, t_end)[:, :, :agent._B].permute(0, 2, 1).cpu().numpy()
        return a[:, 0] if agent._B == 1 else a

    def _target_tensor(self, t_start, t_end):
        pops = self._populations()
        agent = pops[0].Agent
        start, stop = _rows(agent, pops, t_start, t_end)
        h = agent._hist
        rows = list(TARGETS[self.target])
        parts = [h.chunks[c][r:r + length][:, rows] for ((c, r),), length in history_pieces([h.filled], start, stop)]
        return self._joined(agent, parts)

    def error(self, t_start=None, t_end=None):
        """Mean Euclidean distance between the decoded and the recorded target over the rows, per agent: float64 (B,)
        device tensor (rows whose target is not finite are left out of the mean)."""
        agent = self._populations()[0].Agent
        d = self.decode_tensor(t_start, t_end).to(torch.float64) - self._target_tensor(t_start, t_end).to(torch.float64)
        return torch.sqrt((d * d).sum(dim=1))[:, :agent._B].nanmean(dim=0)


class LinearDecoder(HistoryDecoder):
    """sklearn.linear_model.Ridge(alpha) with an intercept, solved from a moment matrix in float64 on its device:
    xbar = s / N, ybar = sum y / N, A = G - N xbar xbar^T + alpha I, W = A^-1 (C - N xbar ybar^T), b = ybar - xbar W.
    `coef_` (D, n) and `intercept_` (D,) are float64 tensors on the moments' device."""

    def __init__(self, coef, intercept, layout, alpha, moments, n_samples, n_dropped):
        self.coef_, self.intercept_ = coef, intercept
        self.layout, self.alpha, self.moments = layout, float(alpha), moments
        self.target = layout.target
        self.n_samples, self.n_dropped = int(n_samples), int(n_dropped)
        self._tables = None

    @classmethod
    def from_moments(cls, M, layout, alpha=0.01):
        if not float(alpha) >= 0:
            raise ValueError(f"alpha must be >= 0, got {alpha}")
        if M.dtype != torch.float64 or tuple(M.shape) != (layout.m, layout.m):
            raise ValueError(f"the moments must be a float64 tensor ({layout.m}, {layout.m})")
        n, D = layout.n, layout.D
        N = M[-1, -1]
        if not float(N) >= 1:
            raise ValueError("the moments hold no sample")
        xbar, ybar = M[-1, :n] / N, M[-1, n:n + D] / N
        A = M[:n, :n] - N * torch.outer(xbar, xbar)
        A.diagonal().add_(float(alpha))
        W = torch.linalg.solve(A, M[:n, n:n + D] - N * torch.outer(xbar, ybar))     # (n, D)
        dropped = 0 if layout.n_dropped is None else int(layout.n_dropped.item())
        return cls(W.T.contiguous(), ybar - xbar @ W, layout, alpha, M, round(float(N)), dropped)

    # ---- running the decoder over history rows (riab_feedforward, linear activation) -------------------------------
    def _populations(self):
        if self.layout.populations is None:
            raise ValueError("this decoder was built from bare moments: it has no populations to read rates from")
        return self.layout.populations

    def _device_tables(self, dev):
        """(W^T per population, float32 (n_l, 32) zero padded as riab_feedforward takes them; bias float32 (D,))"""
        if self._tables is None:
            wts, k = [], 0
            for w in self.layout.widths:
                wt = torch.zeros((w, 32), dtype=torch.float32, device=dev)
                wt[:, :self.layout.D] = self.coef_[:, k:k + w].T.to(torch.float32)
                wts.append(wt)
                k += w
            self._tables = (wts, self.intercept_.to(torch.float32).contiguous())
        return self._tables

    def decode_tensor(self, t_start=None, t_end=None):
        """The decoded target of the history rows `get_history_slice(t_start, t_end)` (both None: every row): float32
        `[T][D][Bp]` on the device, out[t][d][b] = sum_k coef_[d][k] rates[t][k][b] + intercept_[d]."""
        agent, pieces = self._pieces_of_rates(t_start, t_end)
        wts, bias = self._device_tables(agent._device)
        return self._joined(agent, [torch.ops.riab.feedforward(views, wts, bias, _L.ACTIVATIONS["linear"], [0.0, 0.0, 0.0, 0.0])
                                    for views in pieces])

    def as_layer(self, params={}):
        """The decoder as a live FeedForwardLayer (linear activation, n = D, the populations as inputs, `w` and `biases`
        set): the decoded target becomes a population like any other, with history, simulate() and step plans."""
        from .Neurons import FeedForwardLayer
        pops = self._populations()
        if len({p.name for p in pops}) != len(pops):
            raise ValueError("FeedForwardLayer keys its inputs by name: give the populations distinct names")
        coef = self.coef_.cpu().numpy()
        p = {"n": self.layout.D, "input_layers": pops, "activation_function": {"activation": "linear"},
             "biases": self.intercept_.cpu().numpy().copy(), "name": f"Decoded_{self.target}"}
        p.update(params)
        layer = FeedForwardLayer(pops[0].Agent, p)
        k = 0
        for pop in pops:
            w = np.ascontiguousarray(coef[:, k:k + int(pop.n)])
            layer.inputs[pop.name]["w"], layer.inputs[pop.name]["w_init"] = w, w.copy()
            k += int(pop.n)
        return layer


def fit_linear_decoder(populations, target="pos", t_start=None, t_end=None, stride=1, alpha=0.01, spikes=False):
    """`LinearDecoder.from_moments(*history_moments_tensor(populations, target, t_start, t_end, stride), alpha)`."""
    if not float(alpha) >= 0:
        raise ValueError(f"alpha must be >= 0, got {alpha}")
    M, layout = history_moments_tensor(populations, target, t_start, t_end, stride, spikes)
    return LinearDecoder.from_moments(M, layout, alpha)
