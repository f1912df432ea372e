"""Empirical rate maps and the occupancy heatmap, computed where the history lives.

The reference bins `history["pos"]` against `history["firingrate"]` on the host (Neurons.py:377-398, 479-490;
Agent.py:951-956; utils.py:544-589).  Here the trajectory rows `[T][8][Bp]` and a population's rows `[T][n][Bp]` sit in
`DeviceHistory` chunks; this module walks the chunks and hands each piece to the two kernels of csrc/riab_ratemap.hip
(`torch.ops.riab.history_bin_index`, `torch.ops.riab.history_rate_map`), which accumulate into one set of buffers.
Nothing is stacked, concatenated or copied to the host."""
import numpy as np
import torch

from . import _lib as _L
from . import ops as _ops  # noqa: F401  (registers torch.ops.riab.history_*)
from . import utils

MAX_QUADS = (1 << 31) - 2   # riab_history_*: T * B / 4 of one call stays below 2^31 - 1


def history_pieces(filled, start, stop, stride=1, max_rows=None):
    """The rows range(start, stop, stride) of several histories of the same steps whose chunk boundaries need not
    coincide, as pieces that lie in ONE chunk of each: a list of (first rows, length) where `first rows` is one (chunk,
    row in it) per history and the piece's rows 0, stride, 2 stride, ... < length are the selected ones — the stride
    keeps its phase across chunk and piece boundaries.  `filled`: the rows used per chunk, one list per history
    (DeviceHistory.filled); `max_rows`: the longest piece one call takes."""
    start, stop, stride = int(start), int(stop), int(stride)
    if stride < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    if start < 0 or stop > min(sum(f) for f in filled):
        raise ValueError(f"rows [{start}, {stop}) are not in every history ({[sum(f) for f in filled]} rows)")
    limit = None if max_rows is None else max(1, int(max_rows))
    out = []
    idx = [0] * len(filled)    # current chunks
    base = [0] * len(filled)   # global row of their first rows
    g = start
    while g < stop:
        for h, f in enumerate(filled):
            while g >= base[h] + f[idx[h]]:
                base[h] += f[idx[h]]
                idx[h] += 1
        end = min([stop] + [base[h] + f[idx[h]] for h, f in enumerate(filled)])
        if limit is not None:
            end = min(end, g + limit)
        length = (end - 1 - g) // stride * stride + 1     # up to the last selected row of [g, end)
        out.append(([(idx[h], g - base[h]) for h in range(len(filled))], length))
        g += (length - 1) + stride                        # the next selected row
    return out


def history_segments(filled_a, filled_p, start, stop):
    """The rows [start, stop) of two histories of the same steps whose chunk boundaries need not coincide, as pieces
    that lie in ONE chunk of each: a list of (agent chunk, first row in it, population chunk, first row in it, length).
    `filled_a` / `filled_p`: the rows used per chunk (DeviceHistory.filled)."""
    return [(ca, ra, cp, rp, n) for ((ca, ra), (cp, rp)), n in history_pieces([filled_a, filled_p], start, stop)]


def _edge_tensors(extent, dx):
    ex, ey = utils.histogram_bin_edges(extent, dx)
    if len(ex) < 2 or len(ey) < 2:
        raise ValueError("the grid has no bins")
    return torch.from_numpy(ex), torch.from_numpy(ey), len(ex) - 1, len(ey) - 1


def _pieces(length, Bp):
    """(offset, rows) pieces of a segment, each within what one call of the library takes."""
    step = max(1, MAX_QUADS // max(1, Bp // 4))
    return [(o, min(step, length - o)) for o in range(0, length, step)]


def position_heatmap_tensor(agent, dx, start, stop):
    """Occupancy counts int64 (ny, nx) on the device of rows [start, stop) of `agent`'s trajectory history."""
    ex, ey, nx, ny = _edge_tensors(agent.Environment.extent, dx)
    h = agent._hist
    counts = torch.zeros((ny, nx), dtype=torch.int64, device=agent._device)
    for ca, ra, _cp, _rp, n in history_segments(h.filled, h.filled, start, stop):
        for o, k in _pieces(n, agent._Bp):
            torch.ops.riab.history_bin_index(h.chunks[ca][ra + o:ra + o + k], ex, ey, agent._B, counts)
    return counts


def rate_map_tensors(agent, pop_hist, n, dx, start, stop, norm_by_bincount):
    """(maps float64 (n, ny, nx), zero_bins bool (ny, nx), counts int64 (ny, nx)) on the device: rows [start, stop) of
    the population history `pop_hist` ([T][n][Bp] chunks, fp32 rates or uint8 spikes) binned against the same rows of
    `agent`'s trajectory."""
    ex, ey, nx, ny = _edge_tensors(agent.Environment.extent, dx)
    h = agent._hist
    dev = agent._device
    counts = torch.zeros((ny, nx), dtype=torch.int64, device=dev)
    sums = torch.zeros((int(n), ny, nx), dtype=torch.float64, device=dev)
    for ca, ra, cp, rp, length in history_segments(h.filled, pop_hist.filled, start, stop):
        for o, k in _pieces(length, agent._Bp):
            ids = torch.ops.riab.history_bin_index(h.chunks[ca][ra + o:ra + o + k], ex, ey, agent._B, counts)
            torch.ops.riab.history_rate_map(pop_hist.chunks[cp][rp + o:rp + o + k], ids, sums)
    maps, zero = torch.ops.riab.history_rate_map_finish(sums, counts, bool(norm_by_bincount))
    return maps, zero, counts


def history_rows(times, dt, t_start, t_end):
    """Agent.get_history_slice's (startid, endid) (reference Agent.py:1068-1091) from the list of recorded times."""
    t = np.asarray(times, dtype=float)
    if len(t) == 0:
        return 0, 0
    t_start = t_start or t[0]
    t_end = t_end or t[-1]
    return int(np.nanargmin(np.abs(t - t_start))), int(np.nanargmin(np.abs(t - t_end)))
