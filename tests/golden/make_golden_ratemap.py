"""Generate tests/golden/ratemap_reference.npz by IMPORTING THE REFERENCE and calling its own
utils.bin_data_for_histogramming, the way make_golden_theta.py drives the phase-precessing cells.

Runs only in the build container (needs /root/reference); the .npz file is data (inputs + the reference's outputs) and
is committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_ratemap.py [--out DIR]

One reference agent, T_STEPS steps at dt 50 ms in a 2 x 1 room with a wall, 6 PlaceCells + 4 GridCells (Agent.update();
N.update()).  A device history holds fp32 rows, so the recorded positions and rates are rounded to float32 HERE and the
reference's binning is run on those values widened back to float64: what is stored is exactly what a replay bins.

  pos (T, 2) float32, fr (T, 10) float32, spikes (T, 10) bool, t (T,) float64, extent (4,)
  for dx in 0.05 ("05"), 0.1 ("10"):
    rate_norm_<dx> / rate_sum_<dx> (10, ny, nx)   bin_data_for_histogramming(pos, extent, dx, weights=fr[:, c],
                                                  norm_by_bincount=True / False)
    spike_norm_<dx> / spike_sum_<dx>              the same with the spikes as weights
    zero_bins_<dx> (ny, nx) bool                  its return_zero_bins
    heatmap_<dx> (ny, nx)                         bin_data_for_histogramming(pos, extent, dx): Agent.plot_position_heatmap's"""
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from ratinabox import utils  # noqa: E402
from ratinabox.Environment import Environment  # noqa: E402
from ratinabox.Agent import Agent  # noqa: E402
from ratinabox.Neurons import PlaceCells, GridCells  # noqa: E402

T_STEPS = 2000


def main(dest):
    np.random.seed(20)
    Env = Environment({"aspect": 2, "scale": 1})
    Env.add_wall([[1.0, 0.0], [1.0, 0.5]])
    Ag = Agent(Env, {"dt": 0.05})
    PCs = PlaceCells(Ag, {"n": 6, "widths": 0.15})
    GCs = GridCells(Ag, {"n": 4, "gridscale": 0.4})
    for _ in range(T_STEPS):
        Ag.update()
        PCs.update()
        GCs.update()
    pos = np.array(Ag.history["pos"], dtype=np.float64).astype(np.float32)
    fr = np.concatenate((np.array(PCs.history["firingrate"]), np.array(GCs.history["firingrate"])), axis=1).astype(np.float32)
    sp = np.concatenate((np.array(PCs.history["spikes"]), np.array(GCs.history["spikes"])), axis=1).astype(bool)
    out = dict(pos=pos, fr=fr, spikes=sp, t=np.array(Ag.history["t"], dtype=np.float64),
               extent=np.array(Env.extent, dtype=np.float64))
    p64 = pos.astype(np.float64)
    for tag, dx in (("05", 0.05), ("10", 0.1)):
        for name, w in (("rate", fr.astype(np.float64)), ("spike", sp.astype(np.float64))):
            norm, summed = [], []
            for c in range(w.shape[1]):
                m, zero = utils.bin_data_for_histogramming(data=p64, extent=Env.extent, dx=dx, weights=w[:, c],
                                                           norm_by_bincount=True, return_zero_bins=True)
                norm.append(m)
                summed.append(utils.bin_data_for_histogramming(data=p64, extent=Env.extent, dx=dx, weights=w[:, c]))
            out[f"{name}_norm_{tag}"], out[f"{name}_sum_{tag}"] = np.array(norm), np.array(summed)
        out[f"zero_bins_{tag}"] = np.array(zero)
        out[f"heatmap_{tag}"] = np.array(utils.bin_data_for_histogramming(data=p64, extent=Env.extent, dx=dx))
        print(f"dx {dx}: maps {out[f'rate_norm_{tag}'].shape}, {int(out[f'zero_bins_{tag}'].sum())} empty bins, "
              f"busiest bin {int(out[f'heatmap_{tag}'].max())} samples")
    path = os.path.join(dest, "ratemap_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE)
