"""Empirical rate maps from a recorded run, computed on the device: 1024 agents explore a room for a while, PlaceCells
and GridCells record their rates, and `get_rate_map()` bins the whole history (every agent pooled) into one map per
cell — next to the ground-truth map of the same cells, with the correlation between the two.

    python examples/rate_map_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
np.random.seed(0)

Env = riab.Environment()                     # (dx 0.01: the ground truth is evaluated on a 100 x 100 grid)
Ag = riab.Agent(Env, {"n_agents": 1024, "dt": 0.05})
PCs = riab.PlaceCells(Ag, {"n": 64, "widths": 0.15, "wall_geometry": "euclidean"})
GCs = riab.GridCells(Ag, {"n": 32, "gridscale": 0.4})
Ag.simulate(steps)
torch.cuda.synchronize()

occupancy = Ag.get_position_heatmap(dx=0.05)
print(f"{steps} steps x {Ag.n_agents} agents: {int(occupancy.sum())} samples on a {occupancy.shape[1]} x {occupancy.shape[0]} grid, "
      f"{int((occupancy == 0).sum())} empty bins, busiest bin {int(occupancy.max())}")

for N in (PCs, GCs):
    t0 = time.perf_counter()
    maps, zero_bins = N.get_rate_map(method="history", bin_size=0.05)
    dt = time.perf_counter() - t0
    truth, _ = N.get_rate_map(method="groundtruth")                  # (n, 100, 100) on the environment's grid
    k = truth.shape[1] // maps.shape[1]
    coarse = truth.reshape(N.n, maps.shape[1], k, maps.shape[2], k).mean(axis=(2, 4))   # ... averaged over each 5 cm bin
    seen = ~zero_bins
    corr = np.corrcoef(maps[:, seen].reshape(-1), coarse[:, seen].reshape(-1))[0, 1]
    spikes, _ = N.get_rate_map(spikes=True, norm_by_bincount=False)
    print(f"{N.name}: {N.n} maps of {maps.shape[1:]} from {len(N._hist_fr) - 1} recorded rows in {dt * 1e3:.1f} ms; correlation "
          f"with the ground truth {corr:.4f}; {int(spikes.sum())} spikes binned")
    assert corr > 0.95
